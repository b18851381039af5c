"""GPU: BeamCTCDecoder with an ARPA language model (lr_ctc_beam_lm_decode) against exhaustive enumeration and the
float64 restatement beam_lm_ref of tests/test_beam_lm_cpu.py.

Tolerances as tests/test_gpu_beam.py: 1e-5 on the exhaustive shapes, 2e-4 plus 1e-6 of the score's magnitude
elsewhere (fp32 masses; the OOV term alone is -1000 * alpha)."""
import numpy as np
import pytest
import torch

from tests.test_beam_cpu import softmax_frames
from tests.test_beam_lm_cpu import (LABELS, TOY, Dict, RefLM, beam_lm_ref, enumerate_lm, pseudo_corpus, two_gram,
                                    write_arpa)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need an MI355X"
  return torch.device("cuda:0")


def model_labels():
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.decoder import ctc_labels
  return ctc_labels(default_char2idx())


def run(dec, probs, sizes):
  """-> per utterance [(ids, offsets, score)] as decode_ids returns them, best first."""
  ids, off, lens, sc = (x.cpu() for x in dec.decode_ids(probs, sizes))
  out = []
  for b in range(ids.shape[0]):
    s = sc[b].tolist()
    assert s == sorted(s), "scores must ascend"
    beams = []
    for r in range(ids.shape[1]):
      n_ = int(lens[b, r])
      if s[r] == float("inf"):
        assert n_ == 0 and (ids[b, r] == -1).all() and (off[b, r] == -1).all()
        continue
      assert (ids[b, r, n_:] == -1).all() and (off[b, r, n_:] == -1).all()
      beams.append((tuple(ids[b, r, :n_].tolist()), tuple(off[b, r, :n_].tolist()), s[r]))
    out.append(beams)
  return out


def assert_agrees_lm(got, probs_np, sizes, W, n, cutoff_prob, lm, dic, alpha, beta, tol=2e-4, rel=1e-6):
  """tests/test_gpu_beam.py's rules against beam_lm_ref: top-1 ids and offsets identical where the restatement's
  rank-1/rank-2 margin exceeds 1e-3; every returned string the restatement also holds within tol + rel*|score|."""
  checked, wants = 0, []
  for b, beams in enumerate(got):
    want = beam_lm_ref(probs_np[b], int(sizes[b]), W, n, lm, dic, alpha, beta, cutoff_prob)
    wants.append(want)
    assert len(beams) == len(want), (b, len(beams), len(want))
    margin = want[1][2] - want[0][2] if len(want) > 1 else np.inf
    if margin > 1e-3:
      assert beams[0][0] == want[0][0] and beams[0][1] == want[0][1], b
      checked += 1
    ref = {w[0]: w[2] for w in want}
    for ids, _, s in beams:
      if ids in ref:
        assert abs(s - ref[ids]) < tol + rel * abs(ref[ids]), (b, ids, s, ref[ids])
  return checked, wants


def scored_words(ids, labels):
  """Words of a labelling that carry a term: runs of word characters ended by a space or by the end."""
  n, run = 0, 0
  for c in ids:
    l = labels[c]
    if l == " ":
      n += run > 0
      run = 0
    elif len(l) == 1 and c != 0:
      run += 1
    else:
      run = 0
  return n + (run > 0)


def spoken_frames(rng, texts, T, C, labels, noise=0.3, strength=(3.0, 6.0)):
  """Model-like frames that spell `texts`: per character a run of 1-2 frames peaked at its class (with probability
  `noise` a random letter gets a rival peak of 0.8-1.1 times the strength), blanks between, a blank-peaked tail;
  Gaussian logits around the peaks."""
  cls = {l: i for i, l in enumerate(labels)}
  letters = [cls[ch] for ch in "abcdefghijklmnopqrstuvwxyz"]
  x = rng.standard_normal((len(texts), T, C)) * 0.8
  for b, text in enumerate(texts):
    t = 0
    for ch in text:
      if t >= T:
        break
      c = cls[ch]
      rival = int(rng.choice(letters)) if ch != " " and rng.random() < noise else -1
      for _ in range(int(rng.integers(1, 3))):
        if t < T:
          s = rng.uniform(*strength)
          x[b, t, c] += s
          if rival >= 0:
            x[b, t, rival] += s * rng.uniform(0.8, 1.1)
          t += 1
      for _ in range(int(rng.integers(0, 2))):
        if t < T:
          x[b, t, 0] += rng.uniform(*strength)
          t += 1
    x[b, t:, 0] += 4.0
  x = np.exp(x - x.max(2, keepdims=True))
  return (x / x.sum(2, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def lm3(tmp_path_factory):
  """A 3-gram over a seeded pseudo-word corpus, written at test time; its corpus for the frames."""
  words, sents = pseudo_corpus(11, n_words=3000, n_sent=4000)
  path = write_arpa(str(tmp_path_factory.mktemp("lm") / "corpus3.arpa"), sents, 3)
  from lipreading_amd.lm import read_arpa
  lm = RefLM(read_arpa(path))
  return path, lm, Dict(lm, model_labels()), sents


@pytest.mark.parametrize("which", ["toy3", "two2"])
@pytest.mark.parametrize("alpha,beta", [(0.0, 0.0), (0.5, 1.0), (2.0, -0.5)])
@pytest.mark.parametrize("labels,T,seed", [(LABELS, 3, 20), (LABELS, 3, 22), (LABELS[:4], 4, 21),
                                           (LABELS[:4], 5, 23)])
def test_exhaustive_shapes(dev, tmp_path, which, alpha, beta, labels, T, seed):
  """W = 128 holds every labelling that stays in the dictionary (49 with <EOS> at T = 3, 75 without at T = 5)."""
  from lipreading_amd.decoder import BeamCTCDecoder
  if which == "toy3":
    path = tmp_path / "toy.arpa"
    path.write_text(TOY)
    path = str(path)
  else:
    path = two_gram(tmp_path)
  from lipreading_amd.lm import read_arpa
  lm = RefLM(read_arpa(path))
  dic = Dict(lm, labels)
  rng = np.random.default_rng(seed)
  B = 4
  p = np.stack([softmax_frames(rng, T, len(labels)) for _ in range(B)])
  dec = BeamCTCDecoder(labels, lm_path=path, alpha=alpha, beta=beta, beam_width=128, cutoff_top_n=len(labels))
  got = run(dec, torch.tensor(p, device=dev), None)
  for b in range(B):
    want = enumerate_lm(p[b], labels, lm, dic, alpha, beta)
    assert len(want) <= 128
    assert {g[0] for g in got[b]} == {w[0] for w in want}
    ref = dict(want)
    for r, (ids, _, s) in enumerate(got[b]):
      sep = all(abs(want[r][1] - want[q][1]) > 1e-4 for q in (r - 1, r + 1) if 0 <= q < len(want))
      if sep:
        assert ids == want[r][0], (b, r)
      assert abs(s - ref[ids]) < 1e-5 + 1e-6 * abs(ref[ids]), (b, ids, s, ref[ids])


@pytest.mark.parametrize("cutoff_prob", [1.0, 0.99])
@pytest.mark.parametrize("W,n", [(8, 40), (100, 40), (128, 64)])
def test_against_restatement(dev, lm3, cutoff_prob, W, n):
  from lipreading_amd.decoder import BeamCTCDecoder
  path, lm, dic, sents = lm3
  labels = model_labels()
  rng = np.random.default_rng(100 * W + n)
  B, T, C = 32, 75, len(labels)
  texts = [" ".join(sents[int(i)]) for i in rng.integers(0, len(sents), B)]
  p = spoken_frames(rng, texts, T, C, labels)
  sizes = rng.integers(40, T + 1, B)
  sizes[0], sizes[1] = T, 0
  pd, sd = torch.tensor(p, device=dev), torch.tensor(sizes, device=dev)
  alpha, beta = 0.8, 1.5
  dec = BeamCTCDecoder(labels, lm_path=path, alpha=alpha, beta=beta, beam_width=W, cutoff_top_n=n,
                       cutoff_prob=cutoff_prob)
  got = run(dec, pd, sd)
  checked, wants = assert_agrees_lm(got, p, sizes, W, n, cutoff_prob, lm, dic, alpha, beta)
  assert checked >= B // 2
  assert got[1] == [((), (), 0.0)]
  # the data exercise the feature
  two = sum(scored_words(g[0][0], labels) >= 2 for g in got if g)
  assert two > B // 2, two
  plain = BeamCTCDecoder(labels, beam_width=W, cutoff_top_n=n, cutoff_prob=cutoff_prob).decode_ids(pd, sd)
  plain_top = [tuple(plain[0][b, 0, :int(plain[2][b, 0])].tolist()) for b in range(B)]
  assert sum(plain_top[b] != got[b][0][0] for b in range(B) if got[b]) > 0


def test_readable_case(dev, tmp_path):
  """The acoustics favour "teh cat"; the language model returns "the cat"."""
  from lipreading_amd.decoder import BeamCTCDecoder
  labels = model_labels()
  sents = [["the", "cat"]] * 40 + [["the", "dog"]] * 30 + [["a", "cat"]] * 20 + [["teh"]]
  path = write_arpa(str(tmp_path / "cat.arpa"), sents, 3)
  cls = {l: i for i, l in enumerate(labels)}
  C = len(labels)
  frames = []

  def frame(main, alt=None):
    f = np.full(C, 0.05 / (C - 2), np.float64)
    f[cls[main] if main != "_" else 0] = 0.55 if alt else 0.95
    if alt:
      f[cls[alt]] = 0.40
    return f / f.sum()

  for main, alt in [("t", None), ("e", "h"), ("h", "e"), (" ", None), ("c", None), ("a", None), ("t", None)]:
    frames += [frame(main, alt), frame("_")]
  p = torch.tensor(np.asarray(frames, np.float32)[None], device=dev)
  plain = BeamCTCDecoder(labels, beam_width=16, cutoff_top_n=8).decode(p)[0][0][0]
  with_lm = BeamCTCDecoder(labels, lm_path=path, alpha=1.0, beta=0.0, beam_width=16, cutoff_top_n=8).decode(p)
  assert plain == "teh cat"
  assert with_lm[0][0][0] == "the cat"
  from lipreading_amd.lm import read_arpa
  lm = RefLM(read_arpa(path))
  want = beam_lm_ref(p[0].cpu().numpy(), p.shape[1], 16, 8, lm, Dict(lm, labels), 1.0, 0.0)
  assert "".join(labels[c] for c in want[0][0]) == "the cat"


def test_higher_order_long_input_and_a_large_table(dev, tmp_path):
  """A 5-gram of a few hundred thousand n-grams at T = 1000: the lookups stay exact past the toy sizes."""
  from lipreading_amd.decoder import BeamCTCDecoder
  from lipreading_amd.lm import read_arpa
  words, sents = pseudo_corpus(12, n_words=5000, n_sent=30000, zipf=1.05)
  path = write_arpa(str(tmp_path / "big5.arpa.gz"), sents, 5)
  m = read_arpa(path)
  assert m.order == 5 and sum(m.counts) > 300000, m.counts
  lm = RefLM(m)
  labels = model_labels()
  dic = Dict(lm, labels)
  rng = np.random.default_rng(13)
  B, T, C, W, n = 4, 1000, len(labels), 32, 20
  texts = []
  for _ in range(B):
    s = []
    while len(" ".join(s)) < 500:
      s += sents[int(rng.integers(0, len(sents)))]
    texts.append(" ".join(s))
  p = spoken_frames(rng, texts, T, C, labels, noise=0.1)
  sizes = np.array([1000, 999, 640, 1])
  alpha, beta = 0.7, 1.0
  dec = BeamCTCDecoder(labels, lm_path=path, alpha=alpha, beta=beta, beam_width=W, cutoff_top_n=n)
  got = run(dec, torch.tensor(p, device=dev), torch.tensor(sizes, device=dev))
  checked, wants = assert_agrees_lm(got, p, sizes, W, n, 1.0, lm, dic, alpha, beta)
  assert checked >= 2
  assert scored_words(got[0][0][0], labels) > 20
