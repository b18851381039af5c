"""GPU: lr_ctc_segment / segment.CTCSegmenter against the float32 restatement of tests/segment_cases.py — every
comparison with it is `==` —, against lr_ctc_align with both ends fixed, on bad inputs and strided layouts, past the
limits, and through train.segment_videos and the driver's --segment."""
import ctypes
import json

import numpy as np
import pytest
import torch

from lipreading_amd import _C
from tests import segment_cases as S

pytestmark = pytest.mark.gpu

C = 8
LABELS = ['_'] + [chr(ord('a') + i) for i in range(C - 1)]
ALL_FLAGS = (0, S.FREE_START, S.FREE_END, S.FREE_START | S.FREE_END)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda")


@pytest.fixture(scope="module")
def segmenter():
  from lipreading_amd.segment import CTCSegmenter
  return CTCSegmenter(LABELS)


def plan_of(B, T, Cn, W):
  plan = (ctypes.c_int32 * _C.LR_SEG_PLAN_WORDS)()
  assert _C.lib().lr_ctc_segment_plan(B, T, Cn, W, ctypes.addressof(plan)) == _C.LR_OK
  return list(plan)


def device_outputs(segmenter, dev, flags, lp, sizes, targets, lens, uf=None, uc=None, nu=None):
  d = lambda a: None if a is None else torch.from_numpy(a).to(dev)
  out = segmenter.segment_ids(d(lp), d(sizes), d(targets), d(lens), d(uf), d(uc), d(nu),
                              free_start=bool(flags & S.FREE_START), free_end=bool(flags & S.FREE_END))
  return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal(got, want, what=""):
  assert sorted(got) == sorted(want)
  for k in want:
    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
    bad = np.argwhere(got[k] != want[k])
    assert bad.size == 0, (what, k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


# ---- 1: every output, past the aligner's limits on both axes, across state tiles and frame chunks --------------------------
T1, W1 = 2500, 300
SIZES1, LENS1 = (2500, 2313, 2081), (300, 257, 293)


@pytest.fixture(scope="module")
def crossing_cases():
  """Per family: the batch and, per flag combination, the restatement's outputs (computed once, left unchanged)."""
  own, frames, launches, wgs, _, _ = plan_of(3, T1, C, W1)
  assert T1 % 16 != 0 and T1 > 2048 and W1 > 256
  assert launches >= 2 and min(SIZES1) > frames and wgs >= 2 * 3 and all(2 * L + 1 > own for L in LENS1)
  cases = {}
  for k, (name, family) in enumerate(S.FAMILIES):
    rng = np.random.RandomState(40 + k)
    b = S.batch(rng, family, 3, T1, C, W1, SIZES1, LENS1, 0)
    assert (b[6] >= 6).all()
    cases[name] = (b, {fl: S.expected(b[0], b[2], b[1], b[3], 0, fl, b[4], b[5], b[6]) for fl in ALL_FLAGS})
  return cases


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("name", [n for n, _ in S.FAMILIES])
def test_every_output_equals_the_restatement(dev, segmenter, crossing_cases, name, flags):
  (lp, targets, sizes, lens, uf, uc, nu), wants = crossing_cases[name]
  want = wants[flags]
  assert (want["status"] == 0).all()
  if flags == S.FREE_START | S.FREE_END and name != "integers":
    assert (want["span"][:, 0] > 0).any() or (want["span"][:, 1] < sizes).any()
  got = device_outputs(segmenter, dev, flags, lp, sizes, targets, lens, uf, uc, nu)
  assert_equal(got, want, (name, flags))


# ---- 2: a mid-size lattice -----------------------------------------------------------------------------------------------------
def test_mid_size_lattice_equals_the_restatement(dev, segmenter):
  T, L = 4096, 2048
  rng = np.random.RandomState(2)
  lp, targets, sizes, lens, uf, uc, nu = S.batch(rng, S.FAMILIES[2][1], 1, T, C, L, (T,), (L,), 0)
  flags = S.FREE_START | S.FREE_END
  want = S.expected(lp, sizes, targets, lens, 0, flags, uf, uc, nu)
  assert want["status"][0] == 0
  assert_equal(device_outputs(segmenter, dev, flags, lp, sizes, targets, lens, uf, uc, nu), want)


# ---- 2b: state 2L on every lane a wave owns, and on a tile's first state ----------------------------------------------------
@pytest.mark.parametrize("flags", (0, S.FREE_START | S.FREE_END))
def test_end_state_on_every_wave_and_tile_boundary(dev, segmenter, flags):
  """The end record needs v[t][2L-1] beside v[t][2L], also where 2L is the lowest state a tile or a wave owns and 2L-1
  is recomputed in a halo.  A wave owns fewer than 64 lanes and 2L is even, so 32 consecutive L put 2L on every lane a
  wave can own, its first among them; L = own / 2 and 3 * own / 2 put it on a tile's first state.  Sizes leave the last
  forward launch with every number of steps from 1 up."""
  own, frames, _, _, threads, _ = plan_of(1, 800, C, 400)
  assert own % 2 == 0 and threads >= 64
  Ls = sorted(set([own // 2, 3 * own // 2] + list(range(own // 2 + 1, own // 2 + 32))))
  B, T = len(Ls), 800
  assert max(Ls) <= 400 and T > 2 * frames
  sizes = [T - (7 * b) % frames for b in range(B)]
  rng = np.random.RandomState(21 + flags)
  lp, targets, sizes, lens, uf, uc, nu = S.batch(rng, S.FAMILIES[2][1], B, T, C, 400, sizes, Ls, 0)
  want = S.expected(lp, sizes, targets, lens, 0, flags, uf, uc, nu)
  assert (want["status"] == 0).all()
  ends = want["frame_token"][np.arange(B), want["span"][:, 1] - 1]
  assert (ends == lens - 1).any() and (flags != 0 or (ends == -1).any())   # paths that end in state 2L-1, and in 2L
  assert_equal(device_outputs(segmenter, dev, flags, lp, sizes, targets, lens, uf, uc, nu), want, flags)


# ---- 3: one sample of each status, canaries, NaN where nothing may read ------------------------------------------------------
def test_every_status_in_one_batch_stays_in_bounds(dev):
  lib = _C.lib()
  B, T, W, US = 9, 150, 40, 4
  rng = np.random.RandomState(5)
  lp = S.FAMILIES[0][1](rng, (B, T, C))
  sizes = np.array([150, 90, 150, 0, 151, 120, 120, 120, 7], np.int32)
  lens = np.array([40, 25, 0, 10, 10, W + 1, 10, 12, 5], np.int32)
  targets = np.zeros((B, W), np.int32)
  uf, uc, nu = np.zeros((B, US), np.int32), np.zeros((B, US), np.int32), np.full(B, 2, np.int32)
  for b in range(B):
    L = min(max(int(lens[b]), 0), W)
    targets[b, :L] = S.ac.random_target(rng, L, C, 0, doubled=True)
    targets[b, L:] = rng.randint(-5, 10 ** 6, size=W - L)          # junk past the length: never read
    uf[b, :2], uc[b, :2] = (0, L // 2), (L // 2, L - L // 2)
    if 1 <= sizes[b] < T:
      lp[b, sizes[b]:] = np.nan                                     # frames t >= n: never read
  targets[6, 3] = 0                       # the blank inside the length
  uf[7, 1], uc[7, 1] = 6, 7               # 6 + 7 > 12
  targets[8, :5] = (3, 3, 3, 3, 3)        # five equal tokens need nine frames, there are seven
  nu[1] = US + 1                          # n_utts outside [0, utt_stride]
  flags = S.FREE_START | S.FREE_END
  want = S.expected(lp, sizes, targets, lens, 0, flags, uf, uc, nu)
  assert want["status"].tolist() == [0, -2, 0, -2, -2, -2, -1, -3, 1]
  shapes = dict(frame_token=(B, T), tok_start=(B, W), tok_end=(B, W), tok_logp=(B, W), utt_start=(B, US), utt_end=(B, US),
                utt_frames=(B, US), utt_logp=(B, US), utt_worst=(B, US), span=(B, 2), total=(B,), status=(B,))
  G = 64
  bufs = {}
  for k, shp in shapes.items():
    dt = torch.float32 if k in ("tok_logp", "utt_logp", "total") else torch.int32
    bufs[k] = torch.full((int(np.prod(shp)) + 2 * G,), 12345, dtype=dt, device=dev)
  d = lambda a: torch.from_numpy(a).to(dev)
  lp_d, sz, tg, tl, uf_d, uc_d, nu_d = d(lp), d(sizes), d(targets), d(lens), d(uf), d(uc), d(nu)
  nbytes = lib.lr_ctc_segment_workspace_bytes(B, T, C, W)
  ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
  ptr = lambda k: bufs[k].data_ptr() + 4 * G
  _C.check(lib.lr_ctc_segment(lp_d.data_ptr(), T * C, C, sz.data_ptr(), tg.data_ptr(), W, tl.data_ptr(), uf_d.data_ptr(),
                              uc_d.data_ptr(), US, nu_d.data_ptr(), 0, flags, *[ptr(k) for k in shapes], ws.data_ptr(),
                              nbytes, B, T, C, W, _C.stream_handle()), "lr_ctc_segment")
  got = {}
  for k, shp in shapes.items():
    host = bufs[k].cpu().numpy()
    assert (host[:G] == 12345).all() and (host[-G:] == 12345).all(), k
    got[k] = host[G:-G].reshape(shp)
  assert_equal(got, want)


# ---- 4: the transposed view of a (T, B, C) tensor goes in as it is ---------------------------------------------------------------
def test_time_major_view_gives_the_same_outputs(dev, segmenter):
  rng = np.random.RandomState(8)
  T, W = 700, 200
  lp, targets, sizes, lens, uf, uc, nu = S.batch(rng, S.FAMILIES[0][1], 2, T, C, W, (700, 655), (200, 181), 0)
  d = lambda a: torch.from_numpy(a).to(dev)
  tbc = d(lp).transpose(0, 1).contiguous()            # (T, B, C)
  view = tbc.transpose(0, 1)
  assert not view.is_contiguous() and view.stride(2) == 1
  seen = {}
  from lipreading_amd import _host
  real = _host.log_probs_3d
  try:
    _host.log_probs_3d = lambda x, *a: seen.setdefault("lp", real(x, *a))
    out = segmenter.segment_ids(view, d(sizes), d(targets), d(lens), d(uf), d(uc), d(nu))
  finally:
    _host.log_probs_3d = real
  assert seen["lp"].data_ptr() == tbc.data_ptr()       # no copy
  want = S.expected(lp, sizes, targets, lens, 0, 3, uf, uc, nu)
  assert_equal({k: v.cpu().numpy() for k, v in out.items()}, want)


def test_timed_call_gives_the_same_outputs(dev, segmenter):
  """lr_ctc_segment_phases (tools/bench_segment.py) is the same launches with events between them."""
  rng = np.random.RandomState(9)
  lp, targets, sizes, lens, uf, uc, nu = S.batch(rng, S.FAMILIES[2][1], 2, 200, C, 50, (200, 131), (50, 17), 0)
  d = lambda a: torch.from_numpy(a).to(dev)
  args = (d(lp), d(sizes), d(targets), d(lens), d(uf), d(uc), d(nu))
  plain = segmenter.segment_ids(*args)
  ms = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
  timed = segmenter._segment_ids(*args, True, True, phase_ms=ms)
  assert all(0.0 < x < 1000.0 for x in ms)
  for k in plain:
    assert torch.equal(plain[k], timed[k]), k


# ---- 5: both flags clear: lr_ctc_align's outputs, GPU against GPU ---------------------------------------------------------------
def test_fixed_ends_equal_the_aligner_on_the_device(dev, segmenter):
  from lipreading_amd.align import CTCAligner
  T, W = 300, 60
  for k, (name, family) in enumerate(S.FAMILIES):
    rng = np.random.RandomState(60 + k)
    lp, targets, sizes, lens, _, _, _ = S.batch(rng, family, 3, T, C, W, (300, 287, 120), (60, 41, 0), 0)
    d = lambda a: torch.from_numpy(a).to(dev)
    seg = segmenter.segment_ids(d(lp), d(sizes), d(targets), d(lens), free_start=False, free_end=False)
    ali = CTCAligner(LABELS).align_ids(d(lp), d(sizes), d(targets), d(lens))
    assert (ali["status"] == 0).all()
    for key in ("frame_token", "tok_start", "tok_end", "tok_logp", "total", "status"):
      assert torch.equal(seg[key], ali[key]), (name, key)
    assert seg["span"].tolist() == [[0, int(n)] for n in sizes]


# ---- 6: L == 0 and n == 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_empty_targets_and_single_frames(dev, segmenter, flags):
  rng = np.random.RandomState(70 + flags)
  B, T, W = 6, 37, 3
  lp = S.FAMILIES[2][1](rng, (B, T, C))
  sizes = np.array([37, 1, 1, 1, 20, 2], np.int32)
  lens = np.array([0, 0, 1, 2, 0, 1], np.int32)           # (n = 1, L = 2) cannot be spelt
  targets = np.array([[1, 2, 3]] * B, np.int32)
  uf, uc, nu = np.zeros((B, 2), np.int32), np.zeros((B, 2), np.int32), np.full(B, 2, np.int32)
  uc[:, 1] = lens
  want = S.expected(lp, sizes, targets, lens, 0, flags, uf, uc, nu)
  assert want["status"].tolist() == [0, 0, 0, 1, 0, 0]
  assert_equal(device_outputs(segmenter, dev, flags, lp, sizes, targets, lens, uf, uc, nu), want, flags)
  no_utts = device_outputs(segmenter, dev, flags, lp, sizes, targets, lens)
  assert_equal(no_utts, {k: v for k, v in want.items() if not k.startswith("utt_")}, flags)


# ---- 7: past the limits nothing is launched -------------------------------------------------------------------------------------------
def test_past_the_limits(dev, segmenter):
  lib = _C.lib()
  one = torch.ones(1, 4, dtype=torch.int32, device=dev)
  n4 = torch.tensor([4], dtype=torch.int32, device=dev)
  lp = torch.zeros(1, 64, C, device=dev)
  canary = torch.full((4096,), 12345, dtype=torch.int32, device=dev)
  p = canary.data_ptr()
  for T, W in ((_C.LR_SEG_MAX_T + 1, 4), (64, _C.LR_SEG_MAX_TOKENS + 1)):
    assert lib.lr_ctc_segment(lp.data_ptr(), T * C, C, None, one.data_ptr(), 4, n4.data_ptr(), None, None, 0, None, 0, 3,
                              p, p, p, p, None, None, None, None, None, p, p, p, p, 1 << 40, 1, T, C, W,
                              _C.stream_handle()) == _C.LR_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert (canary == 12345).all()
  with pytest.raises(ValueError, match="T=65537.*65536 frames"):
    segmenter.segment_ids(torch.zeros(1, 1, C, device=dev).expand(1, 65537, C), None, one, n4)
  with pytest.raises(ValueError, match="width=16385.*16384 target tokens"):
    segmenter.segment_ids(lp, None, torch.ones(1, 16385, dtype=torch.int32, device=dev), n4)


# ---- 8: whole videos: train.segment_videos and the driver's --segment --------------------------------------------------------------
def test_driver_segments_every_validation_video(dev, tmp_path, monkeypatch):
  from lipreading_amd import analysis
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  from lipreading_amd import train as T
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/six", n_videos=6, captions_per_video=6, seed=11)
  path = str(tmp_path / "val_segments.jsonl")
  # six videos, a third of them for training: two validation videos
  out = driver.run(**driver.parse_flags(["--root=" + root, "--data=synth/six", "--batch_size=4", "--enable_ctc=True",
                                         "--ctc_only=True", "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=1",
                                         "--train_split=0.34", "--segment=" + path]))
  with open(path) as f:
    lines = [json.loads(l) for l in f]
  assert len(lines) == 2
  vids = sorted(DS.gen_vid_ids(root, "synth/six", np.random.RandomState(0)))
  enc, c2i = out["encoder"], out["char2idx"]
  both = list(T.segment_videos(enc, vids, dev, c2i, 4))
  assert [r["video"] for r in both] == ["vid%04d" % v for v in range(6)]
  assert len(lines) == out["segment"]["videos"] >= 1 and out["segment"]["path"] == path
  by_name = {r["video"]: r for r in both}
  for l in lines:
    assert json.loads(json.dumps(by_name[l["video"]])) == l          # the same records from the same encoder
  assert out["segment"]["captions"] == sum(len(l["captions"]) for l in lines)
  for vid, r in zip(vids, both):
    clips = DS.VideoClips(vid, c2i)
    assert r["status"] == 0 and len(r["captions"]) == len(clips) > 0              # one entry per kept caption
    assert r["frames"] == sum(f.shape[0] for f in clips.frames)
    assert r["tokens"] == sum(len(c) + 1 for c in clips.captions)
    assert 0 <= r["span"][0] < r["span"][1] <= r["frames"]
    at = r["span"][0]
    for cap, text, (s0, e0) in zip(r["captions"], clips.captions, clips.s_e):
      assert cap["text"] == text and (cap["old_start_s"], cap["old_end_s"]) == (s0, e0)
      assert at <= cap["start"] < cap["end"] <= r["span"][1]                       # inside the stream, and ordered
      at = cap["end"]
      assert 0 < cap["frames"] <= cap["end"] - cap["start"] and 0.0 < cap["confidence"] <= 1.0
      sc, ec = cap["start_clip"], cap["end_clip"]
      assert cap["new_start_s"] == clips.s_e[sc][0] + cap["start_frame"] / 29.97
      assert cap["new_end_s"] == clips.s_e[ec][0] + (cap["end_frame"] + 1) / 29.97
      assert 0 <= cap["start_frame"] < clips.frames[sc].shape[0] and 0 <= cap["end_frame"] < clips.frames[ec].shape[0]
  shifts = analysis.caption_shifts(both)
  assert [s["captions"] for s in shifts] == [len(r["captions"]) for r in both]
  assert all(s["max_shift_s"] >= s["median_shift_s"] >= 0.0 for s in shifts)
  with pytest.raises(ValueError):
    driver.run(root=root, data="synth/six", segment=path, max_epochs=0)
  # a video past the limits, and one that keeps no clip, are reported with a status and their old times, not raised
  from lipreading_amd import segment as SG
  monkeypatch.setattr(SG, "MAX_T", both[0]["frames"] - 1)
  long, = T.segment_videos(enc, vids[:1], dev, c2i, 4)
  assert long["status"] == SG.TOO_LONG and (long["frames"], long["tokens"]) == (both[0]["frames"], both[0]["tokens"])
  assert long["total"] is None and long["span"] is None
  assert long["captions"] == [{k: c[k] for k in ("index", "text", "old_start_s", "old_end_s")} for c in both[0]["captions"]]
  monkeypatch.undo()
  none, = T.segment_videos(enc, vids[:1], dev, c2i, 4, threshold=50.0)
  assert none == dict(video="vid0000", status=SG.NO_CLIPS, frames=0, tokens=0, total=None, span=None, captions=[])
  assert analysis.caption_shifts([long, none]) == [
      dict(video="vid0000", status=SG.TOO_LONG, captions=len(long["captions"]), median_shift_s=None, max_shift_s=None,
           low_confidence=len(long["captions"])),
      dict(video="vid0000", status=SG.NO_CLIPS, captions=0, median_shift_s=None, max_shift_s=None, low_confidence=0)]
