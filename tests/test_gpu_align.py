"""GPU: lr_ctc_align / align.CTCAligner against the float32 restatement of tests/align_cases.py — every comparison
with it is `==` —, against the greedy decoder and the CTC loss, on planted segmentations, on strided layouts and bad
inputs, and through train.align_loader and the driver's --align."""
import json

import numpy as np
import pytest
import torch

from lipreading_amd import _C, lm
from lipreading_amd.data import EOS, default_char2idx
from lipreading_amd.decoder import ctc_labels
from tests import align_cases as A

pytestmark = pytest.mark.gpu

LABELS = ctc_labels(default_char2idx())     # 65 classes, blank at 0
ROLES = lm.class_roles(LABELS, 0)
C = len(LABELS)
LOSS_TOL = 1e-4    # the loss tolerance of tests/test_gpu_ctc.py (the loss kernel's fast exp / log)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda")


@pytest.fixture(scope="module")
def aligner():
  from lipreading_amd.align import CTCAligner
  return CTCAligner(LABELS)


def device_outputs(aligner, dev, lp, sizes, targets, target_lens):
  out = aligner.align_ids(torch.from_numpy(lp).to(dev), None if sizes is None else torch.from_numpy(sizes).to(dev),
                          torch.from_numpy(targets).to(dev), torch.from_numpy(target_lens).to(dev))
  return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal(got, want, what=""):
  assert sorted(got) == sorted(want)
  for k in want:
    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
    bad = np.argwhere(got[k] != want[k])
    assert bad.size == 0, (what, k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def crossed_batch(T, Ls, seed):
  """Every L of `Ls` x the three value families x (plain, doubled) targets; ragged sizes; junk ids past the lengths."""
  rng = np.random.RandomState(seed)
  W = max(max(Ls), 1)
  lps, sizes, targets, lens = [], [], [], []
  for L in Ls:
    for _, family in A.FAMILIES:
      for doubled in (False, True):
        lps.append(family(rng, (T, C)))
        sizes.append(T if len(sizes) % 3 else rng.randint(1, T + 1))
        row = rng.randint(-5, 10 ** 6, size=W)
        row[:L] = A.random_target(rng, L, C, 0, doubled)
        targets.append(row)
        lens.append(L)
  return (np.stack(lps), np.array(sizes, np.int32), np.stack(targets).astype(np.int32), np.array(lens, np.int32))


# ---- 1: crossed shapes --------------------------------------------------------------------------------------------
ALL_L = (0, 1, 2, 31, 32, 33, 75)


@pytest.mark.parametrize("T", (1, 2, 16, 17, 33, 75, 76))
@pytest.mark.parametrize("Ls", (ALL_L[:4], ALL_L[:5], ALL_L), ids=("one_wave_31", "two_waves_32", "multi_wave_75"))
def test_crossed_shapes_equal_the_restatement(dev, aligner, T, Ls):
  """The kernel is chosen by the target WIDTH: 31 is the widest the one-wave kernel takes, 32 the narrowest of the
  multi-wave one.  Integer values put ties everywhere: the tie-break test."""
  lp, sizes, targets, lens = crossed_batch(T, Ls, seed=100 * T + len(Ls))
  want = A.expected(lp, sizes, targets, lens, 0, ROLES)
  got = device_outputs(aligner, dev, lp, sizes, targets, lens)
  assert_equal(got, want, (T, Ls))
  feasible = int((want["status"] == 0).sum())
  print("T=%d widths<=%d: %d aligned, %d infeasible" % (T, max(Ls), feasible, int((want["status"] == 1).sum())))
  assert feasible >= 3                                        # L = 0 always aligns
  if T < 31:
    assert (want["status"] == A.INFEASIBLE).any()


# ---- 2: large shapes ----------------------------------------------------------------------------------------------
def table_threshold(width):
  """The first T at which the back-pointer table of a `width`-token target leaves LDS for the workspace."""
  lib = _C.lib()
  for T in range(1, 2049):
    if lib.lr_ctc_align_workspace_bytes(1, T, C, width) > 16:
      return T
  return None


def large_case(T, L, seed):
  rng = np.random.RandomState(seed)
  lp = np.stack([A.quantised(rng, (T, C)) for _ in range(2)])
  targets = np.stack([A.random_target(rng, L, C, 0, doubled=k == 1) for k in range(2)]).astype(np.int32)
  sizes = np.array([T, max(T - 7, 1)], np.int32)
  return lp, sizes, targets, np.array([L, max(L - 3, 0)], np.int32)


@pytest.mark.parametrize("shape", ("300x128", "2048x256", "1000x31", "below31", "at31", "below40", "at40"))
def test_large_shapes_equal_the_restatement(dev, aligner, shape):
  """(300, 128) and (2048, 256); (1000, 31): the one-wave kernel streaming its rows from global memory; and for the
  one-wave (31) and the multi-wave (40) kernel the last T with the back-pointer table in LDS and the first with it in
  the workspace, found by asking lr_ctc_align_workspace_bytes."""
  if shape[:2] in ("be", "at"):
    L = int(shape[-2:])
    T = table_threshold(L)
    assert T is not None and T > 1
    lib = _C.lib()
    assert lib.lr_ctc_align_workspace_bytes(2, T - 1, C, L) == 16 < lib.lr_ctc_align_workspace_bytes(2, T, C, L)
    T = T - 1 if shape.startswith("below") else T
  else:
    T, L = (int(x) for x in shape.split("x"))
  lp, sizes, targets, lens = large_case(T, L, seed=T + L)
  want = A.expected(lp, sizes, targets, lens, 0, ROLES)
  assert (want["status"] == 0).all()
  assert_equal(device_outputs(aligner, dev, lp, sizes, targets, lens), want, (shape, T, L))


# ---- 3: against kernels the project already trusts ----------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 2, 75, 200))
def test_aligning_the_greedy_transcript_gives_the_greedy_path(dev, T):
  """Target = the greedy transcript: the argmax path is then the best path (no ties on random reals), so tok_start
  equals the greedy offsets and frame_token follows the per-frame argmax."""
  from lipreading_amd.align import CTCAligner
  from lipreading_amd.decoder import GreedyDecoder
  labels = ['_'] + list("abcdefg") + [' ']
  rng = np.random.RandomState(T)
  lp_h = A.log_softmax(rng, (6, T, len(labels)))
  sizes_h = np.array([T, T, max(T - 1, 1), max(T // 2, 1), T, 1], np.int32)
  lp, sizes = torch.from_numpy(lp_h).to(dev), torch.from_numpy(sizes_h).to(dev)
  ids, off, lens = GreedyDecoder(labels).decode_ids(lp, sizes)
  out = CTCAligner(labels).align_ids(lp, sizes, ids, lens)   # (-1 past the lengths: never read)
  ids, off, lens = ids.cpu().numpy(), off.cpu().numpy(), lens.cpu().numpy()
  out = {k: v.cpu().numpy() for k, v in out.items()}
  assert (out["status"] == 0).all()
  amax = lp_h.argmax(-1)
  for b in range(6):
    n, L = int(sizes_h[b]), int(lens[b])
    assert (out["tok_start"][b, :L] == off[b, :L]).all()
    ft = out["frame_token"][b, :n]
    assert ((ft < 0) == (amax[b, :n] == 0)).all()
    assert all(ids[b, ft[t]] == amax[b, t] for t in range(n) if ft[t] >= 0)
    assert out["total"][b] == pytest.approx(float(lp_h[b, :n].max(-1).astype(np.float64).sum()), rel=1e-5)


def test_total_is_bounded_by_the_ctc_likelihood(dev, aligner):
  """The best path's probability is one term of the sum the loss takes: total <= -nll."""
  from lipreading_amd.ctc import ctc_loss_with_status
  rng = np.random.RandomState(5)
  T, B, W = 75, 8, 30
  lp = A.log_softmax(rng, (B, T, C))
  lens = np.array([30, 30, 12, 1, 0, 25, 30, 7], np.int32)
  sizes = np.array([50, 60, 75, 75, 75, 75, 75, 75], np.int32)   # ascending, as the loss asks
  targets = np.stack([np.array(A.random_target(rng, W, C, 0, doubled=b % 2 == 1)) for b in range(B)]).astype(np.int32)
  got = device_outputs(aligner, dev, lp, sizes, targets, lens)
  assert (got["status"] == 0).all()
  d = lambda a: torch.from_numpy(a).to(dev)
  _, _, nll = ctc_loss_with_status(d(lp), d(targets).long() - 1, d(sizes), d(lens), 'sum')
  nll = nll.cpu().numpy()
  for b in range(B):
    tol = LOSS_TOL * max(1.0, abs(float(nll[b])) / 10)
    print("sample %d: total %.6f  -nll %.6f" % (b, got["total"][b], -nll[b]))
    assert got["total"][b] <= -nll[b] + tol


# ---- 4: planted segmentation --------------------------------------------------------------------------------------
def test_planted_segmentation_is_recovered(dev, aligner):
  """-1/64 on the planted class, -9 elsewhere: any other path loses at least 9 - 1/64 on some frame."""
  plans = (("hi there", [(2, 5), (5, 9), (12, 13), (13, 20), (20, 21), (25, 30), (30, 31), (31, 40)], 44),
           ("aab  c", [(0, 1), (2, 3), (3, 4), (4, 6), (7, 8), (8, 30)], 30),
           ("", [], 9))
  T = 44
  lp = np.full((len(plans), T, C), -9.0, np.float32)
  for b, (text, spans, n) in enumerate(plans):
    cls = np.zeros(T, np.int64)
    for ch, (s, e) in zip(text, spans):
      cls[s:e] = LABELS.index(ch)
    lp[b, np.arange(T), cls] = -1.0 / 64
  sizes = torch.tensor([p[2] for p in plans], dtype=torch.int32, device=dev)
  recs = aligner.align(torch.from_numpy(lp).to(dev), sizes, [p[0] for p in plans])
  for rec, (text, spans, n) in zip(recs, plans):
    assert rec["status"] == 0 and rec["total"] == -n / 64.0
    assert [(c, s, e) for c, s, e, _ in rec["chars"]] == [(ch, s, e) for ch, (s, e) in zip(text, spans)]
    assert [p for _, _, _, p in rec["chars"]] == [-(e - s) / 64.0 for s, e in spans]
    assert all(type(s) is int and type(e) is int for _, s, e, _ in rec["chars"] + rec["words"])
  w = recs[0]["words"]
  assert [(x[0], x[1], x[2]) for x in w] == [("hi", 2, 9), ("there", 13, 40)]
  assert w[0][3] == -7 / 64.0 and w[1][3] == -(7 + 1 + 5 + 1 + 9) / 64.0
  assert [(x[0], x[1], x[2]) for x in recs[1]["words"]] == [("aab", 0, 4), ("c", 8, 30)]
  assert recs[2]["words"] == [] and recs[2]["chars"] == []
  assert aligner.seconds(w[1][1]) == 13 / 29.97 and aligner.seconds(2997) == 100.0
  with pytest.raises(KeyError):
    aligner.align(torch.from_numpy(lp).to(dev), sizes, ["ok", "não", ""])


# ---- 5: layout and bounds -----------------------------------------------------------------------------------------
def test_strided_layouts_give_the_same_outputs(dev, aligner):
  lp, sizes, targets, lens = crossed_batch(33, (0, 2, 9, 31), seed=9)
  want = A.expected(lp, sizes, targets, lens, 0, ROLES)
  B = lp.shape[0]
  d = lambda a: torch.from_numpy(a).to(dev)
  tbc = d(lp).transpose(0, 1).contiguous()                       # (T, B, C) in memory
  big = torch.randn(2 * B + 1, 33 + 5, C + 3, device=dev)        # a slice with odd strides on both axes
  big[1::2, :33, :C][:B] = d(lp)
  views = dict(transposed=tbc.transpose(0, 1), sliced=big[1::2, :33, :C][:B])
  assert views["transposed"].stride() == (C, B * C, 1) and views["sliced"].stride(0) == 2 * 38 * (C + 3)
  for name, v in views.items():
    out = aligner.align_ids(v, d(sizes), d(targets), d(lens))
    assert_equal({k: x.cpu().numpy() for k, x in out.items()}, want, name)


def test_bad_samples_touch_only_themselves_and_guards_stay(dev):
  """Bad ids and lengths set their own sample's status; the neighbours equal the restatement; guard words around
  every output buffer stay untouched (the raw entry point on buffers with 64 guard words either side)."""
  lib = _C.lib()
  T, W = 40, 12
  lp, sizes, targets, lens = crossed_batch(T, (0, 3, W), seed=3)
  B = lp.shape[0]
  assert lens[6] == 3 and lens[12] == W
  targets[6, 0] = 0          # the blank inside the length
  targets[8, 2] = C          # past the classes
  targets[12, 1] = -3
  lens[2], lens[9] = W + 1, -1
  sizes[5], sizes[11] = 0, T + 1
  targets[13, :3] = (7, 7, 7)
  lens[13], sizes[13] = 3, 4   # three equal characters need five frames
  want = A.expected(lp, sizes, targets, lens, 0, ROLES)
  assert sorted(set(want["status"].tolist())) == [-2, -1, 0, 1]
  assert want["status"][[6, 8, 12]].tolist() == [-1] * 3 and want["status"][[2, 9, 5, 11]].tolist() == [-2] * 4
  assert want["status"][13] == 1
  G = 64
  shapes = dict(frame_token=(B, T), tok_start=(B, W), tok_end=(B, W), tok_logp=(B, W), word_first=(B, W),
                word_count=(B, W), word_start=(B, W), word_end=(B, W), word_logp=(B, W), n_words=(B,), total=(B,),
                status=(B,))
  bufs = {}
  for k, shp in shapes.items():
    dt = torch.float32 if k in ("tok_logp", "word_logp", "total") else torch.int32
    bufs[k] = torch.full((int(np.prod(shp)) + 2 * G,), 12345, dtype=dt, device=dev)
  d = lambda a: torch.from_numpy(a).to(dev)
  lp_d, sz, tg, tl, roles = d(lp), d(sizes), d(targets), d(lens), torch.tensor(ROLES, dtype=torch.int32, device=dev)
  nbytes = lib.lr_ctc_align_workspace_bytes(B, T, C, W)
  ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
  ptr = lambda k: bufs[k].data_ptr() + 4 * G
  _C.check(lib.lr_ctc_align(lp_d.data_ptr(), T * C, C, sz.data_ptr(), tg.data_ptr(), W, tl.data_ptr(), roles.data_ptr(),
                            0, *[ptr(k) for k in shapes], ws.data_ptr(), nbytes, B, T, C, W, _C.stream_handle()),
           "lr_ctc_align")
  got = {}
  for k, shp in shapes.items():
    host = bufs[k].cpu().numpy()
    assert (host[:G] == 12345).all() and (host[-G:] == 12345).all(), k
    got[k] = host[G:-G].reshape(shp)
  assert_equal(got, want)


# ---- 6: no hidden reads -------------------------------------------------------------------------------------------
def test_align_ids_reads_nothing_back(dev, aligner):
  probe = torch.ones(1, device=dev)
  torch.cuda.set_sync_debug_mode("error")
  try:
    try:
      probe.item()
      honoured = False
    except RuntimeError:
      honoured = True
  finally:
    torch.cuda.set_sync_debug_mode("default")
  if not honoured:
    pytest.skip("this torch build does not honour set_sync_debug_mode('error') on ROCm")
  lp, sizes, targets, lens = crossed_batch(75, (0, 5, 30), seed=6)
  d = lambda a: torch.from_numpy(a).to(dev)
  args = (d(lp), d(sizes), d(targets), d(lens))
  first = aligner.align_ids(*args)           # the role table's upload and the workspace happen once per device / shape
  torch.cuda.set_sync_debug_mode("error")
  try:
    again = aligner.align_ids(*args)
    longs = aligner.align_ids(args[0], args[1].long(), args[2].long(), args[3].long())
  finally:
    torch.cuda.set_sync_debug_mode("default")
  for k in first:
    assert torch.equal(first[k], again[k]) and torch.equal(first[k], longs[k]), k


def test_limits_raise_with_the_shape(dev, aligner):
  lp = torch.zeros(1, 2049, C, device=dev)
  with pytest.raises(ValueError, match="T=2049.*2048"):
    aligner.align_ids(lp, None, torch.ones(1, 4, dtype=torch.int32, device=dev), torch.tensor([4], device=dev))
  with pytest.raises(ValueError, match="width=257.*256"):
    aligner.align_ids(lp[:, :10], None, torch.ones(1, 257, dtype=torch.int32, device=dev), torch.tensor([4], device=dev))


# ---- 7: loop and driver -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
  """A GRU-32 + CTC head trained for one epoch on a synthetic dataview, and its loader (batches of 4)."""
  from lipreading_amd import dataset as DS
  from lipreading_amd import train as T
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  root = str(tmp_path_factory.mktemp("align"))
  DS.write_synthetic_dataview(root, "synthetic/nano", n_videos=3, captions_per_video=6, seed=1)
  tr, _, _ = DS.split_dataset(root, "synthetic/nano", 0.8, np.random.RandomState(123456))
  ds = DS.FrameCaptionDataset(root, "synthetic/nano", "train", tr)
  loader = DS.make_loader(ds, 4, make_collate_fn(dev))
  torch.manual_seed(123456)
  enc = VideoEncoder(204, 32, rnn_type="GRU", bidirectional=True, enable_ctc=True, vocab_size=len(ds.char2idx),
                     char2idx=ds.char2idx).to(dev)
  T.train(enc, None, loader, FusedAdam(FlatParameters(enc), lr=4e-3), dev, ds.char2idx, grad_norm=50)
  return enc, loader, ds.char2idx


def by_hand(enc, loader, dev, c2i, recurrence=None):
  from lipreading_amd.align import CTCAligner
  al = CTCAligner(ctc_labels(c2i))
  recs = []
  enc.eval()
  saved = enc.recurrence
  if recurrence is not None:
    enc.recurrence = recurrence
  try:
    return _by_hand(al, recs, enc, loader, dev)
  finally:
    enc.recurrence = saved


def _by_hand(al, recs, enc, loader, dev):
  with torch.no_grad():
    for frames, frame_lens, chars, char_lens in loader:
      lp = enc(frames.to(dev), frame_lens.to(dev), max_len=int(frame_lens.max()))[0]
      tg = (chars[:, 1:] + 1).to(dev)
      tl = (char_lens - 1).to(dev)
      for b, rec in enumerate(al.records(al.align_ids(lp, frame_lens.to(dev), tg, tl), tg, tl)):
        rec["index"], rec["frames"] = len(recs), int(frame_lens[b])
        recs.append(rec)
  return recs


def test_align_loader_equals_aligning_each_batch_by_hand(dev, trained):
  from lipreading_amd import analysis
  from lipreading_amd import train as T
  enc, loader, c2i = trained
  got = list(T.align_loader(enc, loader, dev, c2i))
  want = by_hand(enc, loader, dev, c2i)
  assert got == want and len(got) == sum(len(b[3]) for b in loader)
  assert [r["index"] for r in got] == list(range(len(got)))
  ok = [r for r in got if r["status"] == 0]
  assert ok
  for r in ok:
    assert r["chars"][-1][0] == EOS                              # the training target ends in '<EOS>' ...
    assert all(EOS not in w[0] and ' ' not in w[0] for w in r["words"])    # ... which belongs to no word
    assert ' '.join(w[0] for w in r["words"]).split() == ''.join(c[0] for c in r["chars"][:-1]).split()
  timings = analysis.word_timings(enc, loader, dev, c2i)
  assert len(timings) == len(got)
  for r, t in zip(got, timings):
    assert (t is None) == (r["status"] != 0)
    if t is not None:
      assert [(w, s * 29.97) for w, s, _, _ in t] == [(w[0], pytest.approx(w[1])) for w in r["words"]]


def test_a_timed_out_batch_is_encoded_again(dev, trained, monkeypatch):
  """The re-encode path without any fault on the GPU: the host-side reader of the fault word answers 'timed out' for
  batch 1 (as tests/test_gpu_edit.py does), and exactly that batch is encoded again with recurrence='f32'."""
  from lipreading_amd import train as T
  enc, loader, c2i = trained
  before = enc.recurrence
  assert before != 'f32'
  seen = {"keep": 0, "modes": []}
  real_keep, real_fwd = T._fault_keep, enc.forward

  def keep(flag2):
    k = real_keep(flag2)
    seen["keep"] += 1
    return torch.zeros_like(k) if seen["keep"] == 2 else k

  def fwd(*a, **kw):
    seen["modes"].append(enc.recurrence)
    return real_fwd(*a, **kw)

  monkeypatch.setattr(T, "_fault_keep", keep)
  monkeypatch.setattr(enc, "forward", fwd)
  got = list(T.align_loader(enc, loader, dev, c2i))
  n = len(loader)
  assert seen["keep"] == n and seen["modes"] == [before, before, 'f32'] + [before] * (n - 2)
  assert enc.recurrence == before
  monkeypatch.undo()
  sizes = [len(b[3]) for b in loader]
  lo, hi = sizes[0], sizes[0] + sizes[1]
  want, again = by_hand(enc, loader, dev, c2i), by_hand(enc, loader, dev, c2i, recurrence='f32')
  assert got[:lo] == want[:lo] and got[hi:] == want[hi:] and got[lo:hi] == again[lo:hi]


def test_driver_writes_one_line_per_validation_utterance(dev, tmp_path):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=10, captions_per_video=6, seed=7)
  path = str(tmp_path / "val_align.jsonl")
  out = driver.run(**driver.parse_flags(["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True",
                                         "--ctc_only=True", "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=1",
                                         "--align=" + path]))
  val = out["loaders"][1]
  n = sum(len(b[3]) for b in val)
  with open(path) as f:
    lines = [json.loads(l) for l in f]
  assert len(lines) == n > 0 and [l["index"] for l in lines] == list(range(n))
  assert out["align"] == dict(path=path, utterances=n, infeasible=sum(l["status"] == 1 for l in lines))
  assert any(l["status"] == 0 for l in lines)
  for l in lines:
    assert set(l) == {"index", "status", "total", "frames", "words", "chars"}
    if l["status"] != 0:
      assert l["words"] == [] and l["chars"] == []
      continue
    assert l["chars"] and l["chars"][-1]["text"] == EOS
    for w in l["words"] + l["chars"]:
      assert 0 <= w["start"] < w["end"] <= l["frames"]
      assert w["start_s"] == w["start"] / 29.97 and w["end_s"] == w["end"] / 29.97
  with pytest.raises(ValueError):
    driver.run(root=root, data="synth/micro", align=path, max_epochs=0)
