"""GPU: BeamCTCDecoder with hotwords (lr_ctc_beam_bias_decode, lr_ctc_beam_lm_bias_decode) against exhaustive
enumeration and the float64 restatement beam_bias_ref of tests/beam_bias_cases.py.

Tolerances as tests/test_gpu_beam.py and tests/test_gpu_beam_lm.py: 1e-5 (plus 1e-6 of the score's magnitude with a
language model) on the exhaustive shapes, 2e-4 (plus 1e-6 relative with a language model) elsewhere; the bonus is a
handful of fp32 additions of weights of order 10 and adds no more than the relative term covers."""
import warnings

import numpy as np
import pytest
import torch

from tests import beam_bias_cases as K
from tests.test_beam_cpu import softmax_frames
from tests.test_beam_lm_cpu import LABELS, TOY, Dict, RefLM, write_arpa
from tests.test_gpu_beam_lm import run, spoken_frames

pytestmark = pytest.mark.gpu

L28 = K.TRAP_LABELS   # _, ' ', a..z


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need an MI355X"
  return torch.device("cuda:0")


def decoder(labels, phrases, anchor, **kw):
  """A BeamCTCDecoder for phrases given as [(class ids, weight)]."""
  from lipreading_amd.decoder import BeamCTCDecoder
  hot = [("".join(labels[c] for c in q), w) for q, w in phrases]
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")   # hotwords a language model cannot reach are part of some cases
    return BeamCTCDecoder(labels, hotwords=hot, hotword_anchor=anchor >= 0, **kw)


def check_exhaustive(got, want, rel):
  assert len(want) <= 128
  assert {g[0] for g in got} == {w[0] for w in want}
  ref = dict(want)
  for r, (ids, _, s) in enumerate(got):
    sep = all(abs(want[r][1] - want[q][1]) > 1e-4 for q in (r - 1, r + 1) if 0 <= q < len(want))
    if sep:
      assert ids == want[r][0], r
    assert abs(s - ref[ids]) < 1e-5 + rel * abs(ref[ids]), (ids, s, ref[ids])


# labels whose class 1 is ' ' (the anchor) for the four-class shapes
@pytest.mark.parametrize("labels,T,seed,phrases,anchor", [
    (["_", "a", "b"], 6, 30, [((1, 2), 2.0), ((1, 2, 1), 3.5), ((2, 1, 2), 1.25)], -1),
    (["_", "a", "b"], 5, 31, [((2,), 0.75), ((1, 1), 4.0)], -1),
    (["_", " ", "a", "b"], 4, 32, [((2, 3), 2.0), ((3,), 0.5), ((2, 1, 3), 6.0)], 1),
    (["_", " ", "a", "b"], 4, 33, [((2, 3), 2.0), ((3,), 0.5), ((2, 1, 3), 6.0)], -1),
])
def test_exhaustive_shapes(dev, labels, T, seed, phrases, anchor):
  """W = 128 holds every labelling (C = 4 has 148 at T = 5, so T = 4 there); the device against the enumeration and
  the restatement."""
  rng = np.random.default_rng(seed)
  B, C = 4, len(labels)
  p = np.stack([softmax_frames(rng, T, C) for _ in range(B)])
  got = run(decoder(labels, phrases, anchor, beam_width=128, cutoff_top_n=C), torch.tensor(p, device=dev), None)
  bias = K.Bias(phrases, anchor)
  for b in range(B):
    want = K.enumerate_bias(p[b], bias)
    check_exhaustive(got[b], want, 0.0)
    rest = K.beam_bias_ref(p[b], T, 128, C, bias)
    assert {g[0] for g in got[b]} == {w[0] for w in rest}
    ref = {w[0]: w[2] for w in rest}
    for ids, _, s in got[b]:
      assert abs(s - ref[ids]) < 1e-5, (b, ids, s, ref[ids])


@pytest.mark.parametrize("alpha,beta", [(0.5, 1.0), (2.0, -0.5)])
def test_exhaustive_shapes_with_the_toy_language_model(dev, tmp_path, alpha, beta):
  from lipreading_amd.lm import read_arpa
  path = tmp_path / "toy.arpa"
  path.write_text(TOY)
  labels = LABELS[:4]
  lm = RefLM(read_arpa(str(path)))
  dic = Dict(lm, labels)
  phrases = [((2, 3), 3.0), ((3, 3, 1, 2), 5.0), ((3, 2), 4.0)]   # ab, "bb a", ba (no vocabulary prefix)
  B, T, C = 4, 5, len(labels)
  rng = np.random.default_rng(34)
  p = np.stack([softmax_frames(rng, T, C) for _ in range(B)])
  dec = decoder(labels, phrases, 1, lm_path=str(path), alpha=alpha, beta=beta, beam_width=128, cutoff_top_n=C)
  got = run(dec, torch.tensor(p, device=dev), None)
  bias = K.Bias(phrases, 1)
  for b in range(B):
    want = K.enumerate_bias(p[b], bias, labels=labels, lm=lm, dic=dic, alpha=alpha, beta=beta)
    check_exhaustive(got[b], want, 1e-6)


def assert_agrees_bias(got, probs_np, sizes, W, n, cutoff_prob, bias, tol, rel, **lm_kw):
  """tests/test_gpu_beam.py::assert_agrees and tests/test_gpu_beam_lm.py::assert_agrees_lm against beam_bias_ref:
  top-1 ids and offsets identical where the restatement's rank-1/rank-2 margin exceeds 1e-3; every returned string
  the restatement also holds within tol + rel * |score|."""
  checked = 0
  for b, beams in enumerate(got):
    want = K.beam_bias_ref(probs_np[b], int(sizes[b]), W, n, bias, cutoff_prob, **lm_kw)
    assert len(beams) == len(want), (b, len(beams), len(want))
    if not want:   # the dictionary left no hypothesis, here and there
      continue
    margin = want[1][2] - want[0][2] if len(want) > 1 else np.inf
    if margin > 1e-3:
      assert beams[0][0] == want[0][0] and beams[0][1] == want[0][1], b
      checked += 1
    ref = {w[0]: w[2] for w in want}
    for ids, _, s in beams:
      if ids in ref:
        assert abs(s - ref[ids]) < tol + rel * abs(ref[ids]), (b, ids, s, ref[ids])
  return checked


WORDS = ["pan", "panel", "channel", "an", "nel", "ban", "man", "a", "plan", "el"]
HOT = [("pan", 10.0), ("panel", 6.0), ("an", 2.5), ("nel", 4.0), ("channel pan", 12.0), ("a", 0.5)]


@pytest.fixture(scope="module")
def word_lm(tmp_path_factory):
  """A bigram over WORDS, written at test time."""
  from lipreading_amd.lm import read_arpa
  rng = np.random.default_rng(40)
  sents = [[WORDS[int(i)] for i in rng.integers(0, len(WORDS), int(rng.integers(2, 6)))] for _ in range(200)]
  path = write_arpa(str(tmp_path_factory.mktemp("lm") / "words.arpa"), sents, 2)
  lm = RefLM(read_arpa(path))
  return path, lm, Dict(lm, L28)


@pytest.mark.parametrize("cutoff_prob", [1.0, 0.99])
@pytest.mark.parametrize("W,n", [(1, 1), (16, 8), (128, 64)])
@pytest.mark.parametrize("mode", ["anchored", "anywhere", "lm"])
def test_against_restatement(dev, word_lm, mode, W, n, cutoff_prob):
  rng = np.random.default_rng(100 * W + n + len(mode))
  B, T, C = 4, 40, len(L28)
  texts = [" ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), 4)) for _ in range(B)]
  # one hypothesis under the dictionary dies with its first wrong letter: clean frames there, rivals elsewhere
  p = spoken_frames(rng, texts, T, C, L28, noise=0.0 if mode == "lm" and W == 1 else 0.5)
  sizes = np.array([T, 33, 40, 27])
  anchor = -1 if mode == "anywhere" else 1
  phrases = [(K.spell_ids(t), w) for t, w in HOT]
  bias = K.Bias(phrases, anchor)
  kw, lm_kw, tol, rel = {}, {}, 2e-4, 0.0
  if mode == "lm":
    path, lm, dic = word_lm
    kw = dict(lm_path=path, alpha=0.8, beta=1.5)
    lm_kw, rel = dict(lm=lm, dic=dic, alpha=0.8, beta=1.5), 1e-6
  dec = decoder(L28, phrases, anchor, beam_width=W, cutoff_top_n=n, cutoff_prob=cutoff_prob, **kw)
  got = run(dec, torch.tensor(p, device=dev), torch.tensor(sizes, device=dev))
  checked = assert_agrees_bias(got, p, sizes, W, n, cutoff_prob, bias, tol, rel, **lm_kw)
  assert checked >= B // 2
  # the data exercise the feature: some returned hypothesis carries a bonus
  assert any(bias.bonus_end(g[0]) > 0 for beams in got for g in beams)


def zero_class_probs(rng, B, T, C, z):
  p = np.stack([softmax_frames(rng, T, C, scale=2.0) for _ in range(B)])
  p[:, :, z] = 0.0
  return (p / p.sum(2, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("anchor", [True, False])
@pytest.mark.parametrize("with_lm", [False, True])
def test_hotwords_that_cannot_occur_change_nothing(dev, word_lm, anchor, with_lm):
  """Hotwords spelled only in a class of probability zero: the bonus is 0 everywhere, so ids, offsets, lens and the
  scores' bits are those of the search without hotwords."""
  from lipreading_amd.decoder import BeamCTCDecoder
  rng = np.random.default_rng(50)
  B, T, C = 4, 40, len(L28)
  z = L28.index("z")
  assert not any("z" in w for w in WORDS)
  if with_lm:
    texts = [" ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), 4)) for _ in range(B)]
    p = spoken_frames(rng, texts, T, C, L28)
    p[:, :, z] = 0.0
    p = (p / p.sum(2, keepdims=True)).astype(np.float32)
  else:
    p = zero_class_probs(rng, B, T, C, z)
  kw = dict(beam_width=32, cutoff_top_n=C)
  if with_lm:
    kw.update(lm_path=word_lm[0], alpha=0.8, beta=1.5)
  pd = torch.tensor(p, device=dev)
  sizes = torch.tensor([T, 31, 0, 40], device=dev)
  want = BeamCTCDecoder(L28, **kw).decode_ids(pd, sizes)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    got = BeamCTCDecoder(L28, hotwords=["z", ("zz", 3.0), "zzz"], hotword_anchor=anchor, **kw).decode_ids(pd, sizes)
  for a, b in zip(want[:3], got[:3]):
    assert torch.equal(a, b)
  assert torch.equal(want[3].view(torch.int32), got[3].view(torch.int32))
  assert int(want[2][0, 0]) > 0


def test_traps_through_decode(dev):
  from lipreading_amd.decoder import BeamCTCDecoder
  C = len(L28)
  p = torch.tensor(K.homophene_frames()[None], device=dev)
  assert BeamCTCDecoder(L28, beam_width=8, cutoff_top_n=C).decode(p)[0][0][0] == "ban"
  strings, offsets = BeamCTCDecoder(L28, beam_width=8, cutoff_top_n=C, hotwords=["pan"]).decode(p)
  want = K.beam_bias_ref(p[0].cpu().numpy(), p.shape[1], 8, C, K.Bias([(K.spell_ids("pan"), 10.0)], 1))
  assert strings[0][0] == "pan" and offsets[0][0].tolist() == list(want[0][1])
  # beam_width 2: 'p' outlives the first frame only through the partial credit
  q = torch.tensor(K.pruned_prefix_frames()[None], device=dev)
  assert BeamCTCDecoder(L28, beam_width=2, cutoff_top_n=C).decode(q)[0][0] == ["ban", "man"]
  assert BeamCTCDecoder(L28, beam_width=2, cutoff_top_n=C, hotwords=["pan"]).decode(q)[0][0][0] == "pan"
  want = K.beam_bias_ref(q[0].cpu().numpy(), q.shape[1], 2, C, K.Bias([(K.spell_ids("pan"), 10.0)], 1))
  got = BeamCTCDecoder(L28, beam_width=2, cutoff_top_n=C, hotwords=["pan"]).decode(q)[0][0]
  assert got == ["".join(L28[c] for c in w[0]) for w in want]


def test_anchor_on_channel(dev):
  from lipreading_amd.decoder import BeamCTCDecoder
  C = len(L28)
  p = torch.tensor(K.channel_frames()[None], device=dev)
  kw = dict(beam_width=8, cutoff_top_n=C)
  assert BeamCTCDecoder(L28, **kw).decode(p)[0][0][0] == "chanmel"
  assert BeamCTCDecoder(L28, hotwords=["ann"], hotword_anchor=False, **kw).decode(p)[0][0][0] == "channel"
  assert BeamCTCDecoder(L28, hotwords=["ann"], hotword_anchor=True, **kw).decode(p)[0][0][0] == "chanmel"
  # the driver's labels carry multi-character classes too: the anchor is still the ' ' class, by index
  labels = L28 + ["<EOS>"]
  p2 = torch.cat((p, torch.zeros_like(p[:, :, :1])), dim=2)
  assert BeamCTCDecoder(labels, hotwords=["ann"], hotword_anchor=False, **kw).decode(p2)[0][0][0] == "channel"


def test_input_handling_and_independence(dev):
  from lipreading_amd.decoder import BeamCTCDecoder
  rng = np.random.default_rng(60)
  B, T, C = 8, 40, len(L28)
  texts = [" ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), 4)) for _ in range(B)]
  p = spoken_frames(rng, texts, T, C, L28, noise=0.5)
  sizes = np.array([40, 0, 17, 1, 33, 40, 0, 25])
  kw = dict(beam_width=16, cutoff_top_n=20, hotwords=[h for h, _ in HOT])
  pd, sd = torch.tensor(p, device=dev), torch.tensor(sizes, device=dev)
  want = BeamCTCDecoder(L28, **kw).decode_ids(pd, sd)
  assert any(K.Bias([(K.spell_ids(t), w) for t, w in HOT], 1).bonus_end(
      tuple(want[0][b, 0, :int(want[2][b, 0])].tolist())) > 0 for b in range(B))
  # frames past sizes hold NaN and are never read; empty rows are the empty hypothesis
  q = p.copy()
  for b, n in enumerate(sizes):
    q[b, n:] = np.nan
  dirty = BeamCTCDecoder(L28, **kw).decode_ids(torch.tensor(q, device=dev), sd)
  for a, b in zip(want, dirty):
    assert torch.equal(a, b)
  for b in (1, 6):
    assert int(want[2][b, 0]) == 0 and float(want[3][b, 0]) == 0.0 and torch.isinf(want[3][b, 1:]).all()
  # a strided view: the same bits
  pt = pd.transpose(0, 1).contiguous().transpose(0, 1)
  assert not pt.is_contiguous()
  for a, b in zip(want, BeamCTCDecoder(L28, **kw).decode_ids(pt, sd)):
    assert torch.equal(a, b)
  # log-probabilities: another fp32 input, the same hypotheses at the top, scores to rounding
  got_log = BeamCTCDecoder(L28, log_probs_input=True, **kw).decode_ids(torch.log(pd), sd)
  live = [b for b in range(B) if sizes[b] > 0]
  for b in live:
    n_ = int(want[2][b, 0])
    assert int(got_log[2][b, 0]) == n_ and torch.equal(want[0][b, 0, :n_], got_log[0][b, 0, :n_])
    assert abs(float(want[3][b, 0]) - float(got_log[3][b, 0])) < 1e-4
  # B = 1 is the same row inside B = 8
  for b in (0, 2, 4):
    one = BeamCTCDecoder(L28, **kw).decode_ids(pd[b:b + 1], sd[b:b + 1])
    for a, x in zip(want, one):
      assert torch.equal(a[b:b + 1], x)
