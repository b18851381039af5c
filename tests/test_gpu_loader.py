"""GPU: lr_lip_crop_collate_u8 against the per-sample launches it replaces, and loader.PrefetchLoader against the plain
BatchLoader — bit for bit, through train() and greedy_cer(), and not slower.  The yardstick is always the existing
path (data.make_collate_fn / make_pixel_collate_fn / lr_lip_crop_u8), never the new code."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _caption(rng, n):
  return np.array([1] + list(rng.randint(4, 64, n)) + [2])


def _landmark_dataset(n, seed, lens=None):
  rng = np.random.RandomState(seed)
  lens = np.sort(rng.randint(12, 30, n)) if lens is None else lens
  return [(rng.randn(int(t), 68, 3) * 40 + 100, _caption(rng, rng.randint(2, 6))) for t in lens]


def _pixel_dataset(n, seed, hw=(48, 64), lens=None):
  rng = np.random.RandomState(seed)
  H, W = hw
  lens = np.sort(rng.randint(12, 30, n)) if lens is None else lens
  out = []
  for t in lens:
    t = int(t)
    lmk = np.zeros((t, 68, 3))
    lmk[:, :, 0] = rng.uniform(0.1, 0.9, (t, 68)) * W
    lmk[:, :, 1] = rng.uniform(0.1, 0.9, (t, 68)) * H
    lmk[:, 48:68, 0] = rng.uniform(0.35, 0.65, (t, 20)) * W
    lmk[:, 48:68, 1] = rng.uniform(0.55, 0.8, (t, 20)) * H
    out.append(((rng.randint(0, 256, (t, 3, H, W)).astype(np.uint8), lmk), _caption(rng, rng.randint(2, 6))))
  return out


def _loaders(dev, ds, batch, pixels, depth, size=32, workers=2):
  from lipreading_amd.data import make_collate_fn, make_pixel_collate_fn
  from lipreading_amd.dataset import make_loader
  collate = make_pixel_collate_fn(dev, size=size) if pixels else make_collate_fn(dev)
  plain = make_loader(ds, batch, collate)
  fast = make_loader(ds, batch, collate, prefetch=depth, device=dev, pixels=pixels, size=size, workers=workers)
  return plain, fast


def _assert_same_batch(got, want, where):
  assert len(got) == len(want) == 4
  for i, (a, b) in enumerate(zip(got, want)):
    assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, (where, i, a.dtype, b.dtype, a.shape,
                                                                               b.shape, a.device, b.device)
    assert torch.equal(a, b), (where, i)


# ---- 7: the kernel = the launches it replaces, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("S", [32, 96, 36, 30])   # 16 / 16 / 4 / 1 pixels per store
@pytest.mark.parametrize("hw", [(96, 96), (120, 160)])
@pytest.mark.parametrize("B", [1, 5, 32])
def test_collate_kernel_equals_per_sample_launches(dev, B, hw, S):
  from lipreading_amd import _C
  from lipreading_amd.landmarks import _mouth
  L = _C.lib()
  H, W = hw
  rng = np.random.RandomState(1000 * B + H + S)
  t_max = 7
  if B == 1:
    lens = np.array([t_max])
  else:
    lens = rng.randint(1, t_max + 1, B)
    lens[0], lens[-1] = 1, t_max                   # a 1-frame sample and a sample of full t_max
  rows = int(lens.sum())
  frames = rng.randint(0, 256, (rows, 3, H, W)).astype(np.uint8)
  lm = np.zeros((rows, 68, 3), np.float32)
  lm[:, :, 0] = rng.uniform(20, W - 20, (rows, 68))
  lm[:, :, 1] = rng.uniform(20, H - 20, (rows, 68))
  lm[:, 48:68, 0] = rng.uniform(0.4 * W, 0.6 * W, (rows, 20))
  lm[:, 48:68, 1] = rng.uniform(0.6 * H, 0.75 * H, (rows, 20))
  lm[1::5, 48:68, 0] = rng.uniform(-5, 12, lm[1::5, 48:68, 0].shape)   # windows hanging over the left edge
  lm[2::5, 48:68, :2] = 50.0                                          # degenerate boxes -> minimum side
  lm[0, 48:68, 0] = rng.uniform(W - 10, W + 6, 20)                    # and one over the right edge
  offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  frames_d, lmk_d = torch.from_numpy(frames).to(dev), torch.from_numpy(lm).to(dev)
  off_d, lens_d = torch.from_numpy(offsets).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
  # the yardstick: a zeroed batch filled by the existing per-sample entry point
  want = torch.zeros((B, t_max, 3, S, S), dtype=torch.uint8, device=dev)
  for b in range(B):
    lo, n = int(offsets[b]), int(lens[b])
    _C.check(L.lr_lip_crop_u8(frames_d[lo:lo + n].data_ptr(), lmk_d[lo:lo + n].data_ptr(), want[b].data_ptr(), n, H, W,
                              S, 68, _mouth.start, _mouth.stop, 0.3, _C.stream_handle()), "lr_lip_crop_u8")
  guard = 4096
  raw = torch.full((want.numel() + 2 * guard,), 0xFF, dtype=torch.uint8, device=dev)
  out = raw[guard:guard + want.numel()].view(want.shape)       # guard is a multiple of 16: the vector path runs
  _C.check(L.lr_lip_crop_collate_u8(frames_d.data_ptr(), lmk_d.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(),
                                    out.data_ptr(), B, t_max, H, W, S, 68, _mouth.start, _mouth.stop, 0.3,
                                    _C.stream_handle()), "lr_lip_crop_collate_u8")
  torch.cuda.synchronize()
  assert torch.equal(out, want), "differs in %d bytes" % int((out != want).sum())
  assert bool((raw[:guard] == 0xFF).all()) and bool((raw[guard + want.numel():] == 0xFF).all())
  assert int(want[0, 0].max()) > 0                              # the comparison is not of two empty batches
  # an unaligned out takes the scalar path: same bytes
  raw.fill_(0xFF)
  out1 = raw[guard + 1:guard + 1 + want.numel()].view(want.shape)
  _C.check(L.lr_lip_crop_collate_u8(frames_d.data_ptr(), lmk_d.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(),
                                    out1.data_ptr(), B, t_max, H, W, S, 68, _mouth.start, _mouth.stop, 0.3,
                                    _C.stream_handle()), "lr_lip_crop_collate_u8")
  torch.cuda.synchronize()
  assert torch.equal(out1, want)
  assert bool((raw[:guard + 1] == 0xFF).all()) and bool((raw[guard + 1 + want.numel():] == 0xFF).all())


def test_collate_kernel_clamps_a_length_beyond_t_max_and_rejects_bad_arguments(dev):
  from lipreading_amd import _C
  from lipreading_amd.landmarks import _mouth
  L = _C.lib()
  rng = np.random.RandomState(4)
  H = W = 40
  S, t_max = 16, 3
  lens = np.array([5, 2], np.int32)                # sample 0 claims 5 frames (and has them): only 3 may be written
  frames = torch.from_numpy(rng.randint(0, 256, (7, 3, H, W)).astype(np.uint8)).to(dev)
  lm = np.zeros((7, 68, 3), np.float32)
  lm[:, 48:68, :2] = rng.uniform(10, 30, (7, 20, 2))
  lmk = torch.from_numpy(lm).to(dev)
  off = torch.tensor([0, 5], dtype=torch.int64, device=dev)
  want = torch.zeros((2, t_max, 3, S, S), dtype=torch.uint8, device=dev)
  for b, (lo, n) in enumerate(((0, 3), (5, 2))):
    _C.check(L.lr_lip_crop_u8(frames[lo:lo + n].data_ptr(), lmk[lo:lo + n].data_ptr(), want[b].data_ptr(), n, H, W, S,
                              68, _mouth.start, _mouth.stop, 0.3, _C.stream_handle()), "lr_lip_crop_u8")
  guard = 4096
  raw = torch.full((want.numel() + 2 * guard,), 0xFF, dtype=torch.uint8, device=dev)
  out = raw[guard:guard + want.numel()].view(want.shape)
  lens_d = torch.from_numpy(lens).to(dev)
  args = (frames.data_ptr(), lmk.data_ptr(), off.data_ptr(), lens_d.data_ptr(), out.data_ptr())
  _C.check(L.lr_lip_crop_collate_u8(*args, 2, t_max, H, W, S, 68, _mouth.start, _mouth.stop, 0.3, _C.stream_handle()),
           "lr_lip_crop_collate_u8")
  torch.cuda.synchronize()
  assert torch.equal(out, want)
  assert bool((raw[:guard] == 0xFF).all()) and bool((raw[guard + want.numel():] == 0xFF).all())
  s = _C.stream_handle()
  assert L.lr_lip_crop_collate_u8(*args, 0, t_max, H, W, S, 68, 48, 68, 0.3, s) == _C.LR_ERR_INVALID_ARG
  assert L.lr_lip_crop_collate_u8(*args, 2, t_max, H, W, S, 68, 48, 69, 0.3, s) == _C.LR_ERR_INVALID_ARG
  assert L.lr_lip_crop_collate_u8(args[0], None, *args[2:], 2, t_max, H, W, S, 68, 48, 68, 0.3, s) == _C.LR_ERR_INVALID_ARG


# ---- 8: the loader = the plain loader, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("pixels", [False, True])
def test_prefetch_loader_equals_the_plain_loader(dev, pixels, depth):
  ds = _pixel_dataset(23, seed=11) if pixels else _landmark_dataset(23, seed=11)
  plain, fast = _loaders(dev, ds, 4, pixels, depth)
  assert len(fast) == len(plain) == 6
  for epoch in range(2):
    n = 0
    for k, (got, want) in enumerate(zip(fast, plain)):
      _assert_same_batch(got, want, (epoch, k))
      assert got[0].is_cuda and not got[1].is_cuda and not got[2].is_cuda and not got[3].is_cuda
      n += 1
    assert n == 6
  fast.close()


# ---- 9: batches stay valid while the ring is recycled --------------------------------------------------------------
@pytest.mark.parametrize("pixels", [False, True])
def test_held_batches_stay_valid_while_the_consumer_stream_is_busy(dev, pixels):
  from lipreading_amd import _C
  L = _C.lib()
  ds = _pixel_dataset(41, seed=13) if pixels else _landmark_dataset(41, seed=13)
  plain, fast = _loaders(dev, ds, 4, pixels, depth=1)      # two slots for eleven batches: every slot is reused often
  held = []
  it = iter(fast)
  while True:
    # the consumer's stream is busy in front of every __next__ (a stand-in for the step that is still running)
    _C.check(L.lr_debug_busy(48, 32 * 1024, 350, _C.stream_handle()), "lr_debug_busy")
    try:
      held.append(next(it))
    except StopIteration:
      break
  assert len(held) == len(plain) == 11
  torch.cuda.synchronize()
  for k, (got, want) in enumerate(zip(held, plain)):       # compared only now: an early recycle shows here
    _assert_same_batch(got, want, k)
  # and abandoning a pass half-way leaves a loader that starts clean
  for got in fast:
    break
  for k, (got, want) in enumerate(zip(fast, plain)):
    _assert_same_batch(got, want, k)
  fast.close()


# ---- 10 / 11: training and scoring through it change nothing -------------------------------------------------------
def _train_run(dev, ds, loader, pixels, epochs, graphs_on, size=32):
  from lipreading_amd import train as T
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  c2i = default_char2idx()
  torch.manual_seed(2024)
  if pixels:
    from lipreading_amd.frontend import ConvFrontend3D, PixelLipReader, feature_dim
    enc = VideoEncoder(feature_dim(size, size), 32, rnn_type="GRU", bidirectional=True, enable_ctc=True, vocab_size=64,
                       char2idx=c2i)
    model = PixelLipReader(enc, ConvFrontend3D())
  else:
    model = VideoEncoder(204, 32, rnn_type="GRU", bidirectional=True, enable_ctc=True, vocab_size=64, char2idx=c2i)
  model = model.to(dev).train()
  opt = FusedAdam(FlatParameters(model), lr=1e-3)
  graphs = T.StepGraphs(warmup=1, enabled=graphs_on)
  # grad_norm=None: the clip's sum of squares is a float-atomic reduction over workgroups (lr_sumsq: one atomic per
  # workgroup), so once clipping engages two runs of the PLAIN path differ in the last bits (measured: identical
  # gradients, different weights after the first clipped step; DESIGN.md "Prefetching loader").  Without the clip the
  # step is deterministic, and only then does a control of two plain runs say anything about the loader.
  losses = [T.train(model, None, loader, opt, dev, c2i, grad_norm=None, graphs=graphs)[1] for _ in range(epochs)]
  if graphs_on:
    assert graphs.captures >= 1 and graphs.replays >= 1      # the step really ran as a hipGraph
  cer = T.greedy_cer(model, loader, dev, c2i)
  model.train()
  return losses, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, cer


@pytest.mark.parametrize("regime", ["R", "X"])
def test_training_through_the_prefetch_loader_changes_nothing(dev, regime):
  """Regime R: landmarks, hipGraphs on; regime X: pixels at a small crop size, eager.  Two runs over the plain loader
  are the control (the step is deterministic: test_step_graphs_replay_is_bit_identical_to_eager); the prefetched run
  must then equal them exactly — per-epoch losses, final state_dict, and greedy CER."""
  pixels = regime == "X"
  lens = np.repeat([21, 24, 27, 30], 4)[:15]                  # few distinct batch shapes (graphs replay), ragged end
  ds = _pixel_dataset(15, seed=17, lens=lens) if pixels else _landmark_dataset(15, seed=17, lens=lens)
  epochs = 4
  plain, fast = _loaders(dev, ds, 4, pixels, depth=2)
  a = _train_run(dev, ds, plain, pixels, epochs, graphs_on=not pixels)
  b = _train_run(dev, ds, plain, pixels, epochs, graphs_on=not pixels)
  c = _train_run(dev, ds, fast, pixels, epochs, graphs_on=not pixels)
  fast.close()
  print("regime %s losses: plain %r | plain again %r | prefetch %r" % (regime, a[0], b[0], c[0]))
  assert all(np.isfinite(a[0]))
  control = a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
  assert control, "FINDING: two runs over the PLAIN loader differ (%r vs %r): the step is not deterministic" % (a[0], b[0])
  assert c[0] == a[0], (c[0], a[0])
  for k in a[1]:
    assert torch.equal(c[1][k], a[1][k]), k
  assert c[2] == a[2] == b[2]                                 # 11: greedy_cer over the two loaders


# ---- 12: not slower -------------------------------------------------------------------------------------------------
def _bench_tool():
  spec = importlib.util.spec_from_file_location("bench_loader", os.path.join(ROOT, "tools", "bench_loader.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_prefetched_loop_is_not_slower_than_the_plain_loop_at_the_bench_shape(dev):
  """Regime X at B = 32, S = 96, T = 75, the three-arm protocol of tools/bench_loader.py at reduced length.  The
  prefetched loop's median may not exceed the plain loop's median by more than the plain arm's own min-max spread."""
  tool = _bench_tool()
  res = tool.time_arms("X", dev, batch=32, n_batches=5, repeats=5, size=96, hw=96, depth=2, workers=2)
  print("ms per step:", {k: res[k] for k in ("plain", "prefetch", "resident")})
  plain, fast = res["plain"], res["prefetch"]
  assert fast["median"] <= plain["median"] + (plain["max"] - plain["min"]), res


def test_collate_kernel_is_not_slower_than_the_launches_it_replaces(dev):
  tool = _bench_tool()
  res = tool.time_kernel(dev, batch=32, size=96, hw=96, reps=10)
  print(res)
  new, old = res["collate_one_launch_ms"], res["per_sample_launches_ms"]
  assert new["median"] <= old["median"] + (old["max"] - old["min"]), res
