"""GPU: BeamCTCDecoder / lr_ctc_beam_decode (CTC prefix beam search, no language model) against exhaustive
enumeration, the float64 restatement of tests/test_beam_cpu.py and the greedy decoder.

Tolerances: scores are fp32 log-sum-exps accumulated over many frames against a float64 restatement: 1e-5 on the
exhaustive shapes (T <= 6), 2e-4 at T = 75, and 2e-4 plus 1e-6 of the score's magnitude at T = 1000."""
import numpy as np
import pytest
import torch

from tests.test_beam_cpu import beam_ref, enumerate_labellings, softmax_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need an MI355X"
  return torch.device("cuda:0")


def labels_for(C):
  # with a ' ' label: GreedyDecoder keeps the reference's IndexError for label sets without one (decoder.py:174)
  return ["_", " "] + [chr(ord("!") + i) for i in range(C - 2)]


def run_beam(probs, sizes, W, n, cutoff_prob=1.0, log_input=False, blank=0):
  """-> per utterance [(ids tuple, offsets tuple, -log P)] as returned by decode_ids, best first."""
  from lipreading_amd.decoder import BeamCTCDecoder
  dec = BeamCTCDecoder(labels_for(probs.shape[2]), cutoff_top_n=n, cutoff_prob=cutoff_prob, beam_width=W,
                       blank_index=blank, log_probs_input=log_input)
  ids, off, lens, sc = (x.cpu() for x in dec.decode_ids(probs, sizes))
  out = []
  for b in range(ids.shape[0]):
    s = sc[b].tolist()
    assert s == sorted(s), "scores must ascend"
    beams = []
    for r in range(ids.shape[1]):
      n_ = int(lens[b, r])
      if r > 0 and n_ == 0 and s[r] == float("inf"):
        assert (ids[b, r] == -1).all() and (off[b, r] == -1).all()
        continue
      assert (ids[b, r, n_:] == -1).all() and (off[b, r, n_:] == -1).all()
      beams.append((tuple(ids[b, r, :n_].tolist()), tuple(off[b, r, :n_].tolist()), s[r]))
    out.append(beams)
  return out


def peaked_probs(rng, B, T, C):
  """Model-like frames: one dominant class per frame, in runs, blank-heavy."""
  x = rng.standard_normal((B, T, C)) * 0.8
  for b in range(B):
    t = 0
    while t < T:
      run = int(rng.integers(1, 5))
      c = 0 if rng.random() < 0.5 else int(rng.integers(1, C))
      x[b, t:t + run, c] += rng.uniform(3.0, 7.0)
      t += run
  x = np.exp(x - x.max(2, keepdims=True))
  return (x / x.sum(2, keepdims=True)).astype(np.float32)


def assert_agrees(got, probs_np, sizes, W, n, cutoff_prob, log_input=False, tol=2e-4, rel=0.0):
  """item 2's rules: top-1 ids and offsets identical where the restatement's rank-1/rank-2 margin exceeds 1e-3; every
  returned beam whose string the restatement also holds has its score within tol + rel * |score|."""
  checked = 0
  for b, beams in enumerate(got):
    want = beam_ref(probs_np[b], int(sizes[b]), W, n, cutoff_prob, log_input=log_input)
    assert len(beams) == len(want), (b, len(beams), len(want))
    margin = want[1][2] - want[0][2] if len(want) > 1 else np.inf
    if margin > 1e-3:
      assert beams[0][0] == want[0][0] and beams[0][1] == want[0][1], b
      checked += 1
    ref = {w[0]: w[2] for w in want}
    for ids, _, s in beams:
      if ids in ref:
        assert abs(s - ref[ids]) < tol + rel * abs(ref[ids]), (b, ids, s, ref[ids])
  return checked


@pytest.mark.parametrize("C,T,seed", [(2, 6, 10), (3, 5, 11), (4, 4, 12)])
def test_exhaustive_shapes(dev, C, T, seed):
  rng = np.random.default_rng(seed)
  B = 4
  p = np.stack([softmax_frames(rng, T, C) for _ in range(B)])
  got = run_beam(torch.tensor(p, device=dev), None, W=128, n=C)
  for b in range(B):
    want = enumerate_labellings(p[b])
    assert len(want) <= 128
    assert {g[0] for g in got[b]} == {w[0] for w in want}
    ref = dict(want)
    for r, (ids, _, s) in enumerate(got[b][:10]):
      # rank order where the enumeration separates neighbours clearly
      sep = all(abs(want[r][1] - want[q][1]) > 1e-4 for q in (r - 1, r + 1) if 0 <= q < len(want))
      if sep:
        assert ids == want[r][0], (b, r)
      assert abs(s - ref[ids]) < 1e-5, (b, ids, s, ref[ids])


@pytest.mark.parametrize("kind", ["softmax", "peaked"])
@pytest.mark.parametrize("cutoff_prob", [1.0, 0.99])
@pytest.mark.parametrize("W,n", [(1, 1), (1, 40), (8, 1), (8, 40), (8, 64), (100, 40), (100, 64), (128, 1),
                                 (128, 40), (128, 64)])
def test_against_restatement(dev, kind, cutoff_prob, W, n):
  rng = np.random.default_rng(1000 * W + n + (7 if kind == "peaked" else 0))
  B, T, C = 32, 75, 65
  p = peaked_probs(rng, B, T, C) if kind == "peaked" else \
      np.stack([softmax_frames(rng, T, C, scale=2.0) for _ in range(B)])
  sizes = rng.integers(40, T + 1, B)
  sizes[0] = T
  got = run_beam(torch.tensor(p, device=dev), torch.tensor(sizes, device=dev), W, n, cutoff_prob)
  checked = assert_agrees(got, p, sizes, W, n, cutoff_prob)
  assert checked >= B // 2


def test_reduces_to_greedy_on_golden(dev, golden_greedy):
  from lipreading_amd.decoder import BeamCTCDecoder, GreedyDecoder
  g = golden_greedy
  labels = list(g["labels"])
  assert len(set(labels)) == len(labels)
  lp = torch.tensor(g["lp"], device=dev)
  for sizes in (torch.tensor(g["sizes"], device=dev), None):
    s_g, o_g = GreedyDecoder(labels).decode(lp, sizes)
    s_b, o_b = BeamCTCDecoder(labels, beam_width=1, cutoff_top_n=1, log_probs_input=True).decode(lp, sizes)
    assert [s[0] for s in s_b] == [s[0] for s in s_g]
    for b in range(len(s_g)):
      assert o_b[b][0].dtype == torch.int32
      np.testing.assert_array_equal(o_b[b][0].numpy(), o_g[b][0].numpy())
  s_b, _ = BeamCTCDecoder(labels, beam_width=1, cutoff_top_n=1, log_probs_input=True).decode(
      lp, torch.tensor(g["sizes"], device=dev))
  assert [s[0] for s in s_b] == list(g["strings"])


def test_reduces_to_greedy_with_ties(dev):
  from lipreading_amd.decoder import BeamCTCDecoder, GreedyDecoder
  gen = torch.Generator().manual_seed(7)
  B, T, C = 48, 75, 65
  labels = labels_for(C)
  # small integers: many exact argmax ties, frequent repeats and blanks
  p = torch.randint(0, 4, (B, T, C), generator=gen).float()
  p[:, :, 0] += torch.randint(0, 2, (B, T), generator=gen).float() * 2
  p = p / p.sum(-1, keepdim=True)
  sizes = torch.randint(0, T + 1, (B,), generator=gen)
  pd, sd = p.to(dev), sizes.to(dev)
  s_g, o_g = GreedyDecoder(labels).decode(pd, sd)
  s_b, o_b = BeamCTCDecoder(labels, beam_width=1, cutoff_top_n=1).decode(pd, sd)
  assert [s[0] for s in s_b] == [s[0] for s in s_g]
  for b in range(B):
    np.testing.assert_array_equal(o_b[b][0].numpy(), o_g[b][0].numpy())


def test_sizes_zero_and_frames_past_sizes_are_never_read(dev):
  from lipreading_amd.decoder import BeamCTCDecoder
  rng = np.random.default_rng(3)
  B, T, C = 6, 40, 65
  p = peaked_probs(rng, B, T, C)
  sizes = np.array([0, 40, 17, 1, 0, 33])
  dec = BeamCTCDecoder(labels_for(C), beam_width=16, cutoff_top_n=20)
  clean = dec.decode(torch.tensor(p, device=dev), torch.tensor(sizes, device=dev))
  q = p.copy()
  for b, n in enumerate(sizes):
    q[b, n:] = np.nan
  dirty = dec.decode(torch.tensor(q, device=dev), torch.tensor(sizes, device=dev))
  assert clean[0] == dirty[0]
  for b in range(B):
    for x, y in zip(clean[1][b], dirty[1][b]):
      assert torch.equal(x, y)
  for b in (0, 4):
    assert clean[0][b] == [''] * 16
    assert all(o.numel() == 0 for o in clean[1][b])
  ids, off, lens, sc = dec.decode_ids(torch.tensor(q, device=dev), torch.tensor(sizes, device=dev))
  assert int(lens[0, 0]) == 0 and float(sc[0, 0]) == 0.0 and (lens[0, 1:] == 0).all()
  assert torch.isinf(sc[0, 1:]).all()


def test_log_input_and_strided_views(dev):
  from lipreading_amd.decoder import BeamCTCDecoder
  rng = np.random.default_rng(4)
  B, T, C = 16, 75, 65
  p = torch.tensor(peaked_probs(rng, B, T, C), device=dev)
  sizes = torch.tensor(rng.integers(30, T + 1, B), device=dev)
  kw = dict(beam_width=32, cutoff_top_n=40)
  want = BeamCTCDecoder(labels_for(C), **kw).decode_ids(p, sizes)
  got_log = BeamCTCDecoder(labels_for(C), log_probs_input=True, **kw).decode_ids(torch.log(p), sizes)
  pt = p.transpose(0, 1).contiguous().transpose(0, 1)   # (B,T,C) view with stride_t = B*C, stride_b = C
  assert not pt.is_contiguous()
  got_view = BeamCTCDecoder(labels_for(C), **kw).decode_ids(pt, sizes)
  for got in (got_log, got_view):
    for a, b in zip(want[:3], got[:3]):
      assert torch.equal(a, b)
  assert torch.equal(want[3], got_view[3])
  # log(p) is a different fp32 input: same hypotheses, scores to rounding
  fin = torch.isfinite(want[3])
  assert (want[3][fin] - got_log[3][fin]).abs().max().item() < 1e-4


def test_decode_contract(dev):
  from lipreading_amd.decoder import BeamCTCDecoder
  rng = np.random.default_rng(5)
  B, T, C, W = 3, 20, 65, 5
  p = torch.tensor(peaked_probs(rng, B, T, C), device=dev)
  dec = BeamCTCDecoder(labels_for(C), beam_width=W)
  strings, offsets = dec.decode(p)
  ids, off, lens, _ = (x.cpu() for x in dec.decode_ids(p))
  assert len(strings) == B and all(len(s) == W for s in strings)
  for b in range(B):
    for r in range(W):
      n = int(lens[b, r])
      assert strings[b][r] == ''.join(dec.int_to_char[i] for i in ids[b, r, :n].tolist())
      assert offsets[b][r].dtype == torch.int32
      assert offsets[b][r].tolist() == off[b, r, :n].tolist()


def test_long_sequences(dev):
  rng = np.random.default_rng(6)
  B, T, C, W, n = 4, 1000, 65, 128, 40
  p = peaked_probs(rng, B, T, C)
  sizes = np.array([1000, 999, 640, 1])
  got = run_beam(torch.tensor(p, device=dev), torch.tensor(sizes, device=dev), W, n)
  # fp32 rounding grows with the score's magnitude (hundreds of nats at T = 1000): 2e-4 plus 1e-6 relative
  assert_agrees(got, p, sizes, W, n, 1.0, tol=2e-4, rel=1e-6)


def test_ctc_cer_with_one_hypothesis_equals_greedy_cer(dev, tmp_path):
  from lipreading_amd import dataset as DS
  from lipreading_amd import train as T
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synthetic/nano", n_videos=3, captions_per_video=6, seed=1)
  tr, _, _ = DS.split_dataset(root, "synthetic/nano", 0.8, np.random.RandomState(123456))
  ds = DS.FrameCaptionDataset(root, "synthetic/nano", "train", tr)
  loader = DS.make_loader(ds, 4, make_collate_fn(dev))
  torch.manual_seed(123456)
  enc = VideoEncoder(204, 48, rnn_type='LSTM', bidirectional=True, enable_ctc=True,
                     vocab_size=len(ds.char2idx), char2idx=ds.char2idx).to(dev)
  opt = FusedAdam(FlatParameters(enc), lr=2e-3)
  for _ in range(6):
    T.train(enc, None, loader, opt, dev, ds.char2idx, grad_norm=50)
  labels = ctc_labels(ds.char2idx)
  assert len(set(labels)) == len(labels)
  want = T.greedy_cer(enc, loader, dev, ds.char2idx)
  one = BeamCTCDecoder(labels, beam_width=1, cutoff_top_n=1, log_probs_input=True)
  assert T.ctc_cer(enc, loader, dev, ds.char2idx, one) == want
  wide = BeamCTCDecoder(labels, beam_width=16, cutoff_top_n=8, log_probs_input=True)
  assert 0.0 <= T.ctc_cer(enc, loader, dev, ds.char2idx, wide) <= 2.0
