"""GPU: lr_lip_crop_collate_aug_u8 / lr_collate_pad_aug_f32 and PrefetchLoader(augment=...).  The yardstick is always
existing code (lr_lip_crop_collate_u8, the un-augmented loader) or the numpy restatement (tests/augment_cases.py), never
the new code.  The kernel is a pure function of its inputs — the host draws — so all but the shift/zoom comparison are
exact.  The host side is tests/test_augment_cpu.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import augment_cases as AC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096                                       # a multiple of 16: an aligned out takes the vector path

GRID = dict(S=[32, 96, 36, 30],                    # 16 / 16 / 4 / 1 pixels per store
            hw=[(96, 96), (120, 160)], B=[1, 5, 32])


def grid(fn):
  for name in ("S", "hw", "B"):
    fn = pytest.mark.parametrize(name, GRID[name])(fn)
  return fn


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _spec(text, seed=0):
  from lipreading_amd.augment import AugmentSpec
  return AugmentSpec.parse(text, seed=seed)


class Case(object):
  """One point of the grid on the device.  The frame and landmark buffers carry one spare row behind the last sample,
  so that no map value the tests use could leave the allocation even if it were not clamped."""

  def __init__(self, dev, B, hw, S):
    self.dev, self.B, self.hw, self.S, self.t_max = dev, B, hw, S, AC.T_MAX
    self.frames, self.lm, self.offsets, self.lens = AC.ragged_case(B, hw, S)
    spare_f = np.concatenate([self.frames, np.full_like(self.frames[:1], 0x55)])
    spare_l = np.concatenate([self.lm, self.lm[:1]])
    self.frames_d, self.lmk_d = torch.from_numpy(spare_f).to(dev), torch.from_numpy(spare_l).to(dev)
    self.off_d = torch.from_numpy(self.offsets).to(dev)
    self.lens_d = torch.from_numpy(self.lens.astype(np.int32)).to(dev)
    self.shape = (B, self.t_max, 3, S, S)
    self.numel = int(np.prod(self.shape))

  def _guarded(self, launch, misalign):
    raw = torch.full((self.numel + 2 * GUARD + 16,), 0xFF, dtype=torch.uint8, device=self.dev)
    lo = GUARD + misalign
    out = raw[lo:lo + self.numel].view(self.shape)
    assert out.data_ptr() % 16 == misalign
    launch(out)
    torch.cuda.synchronize()
    assert bool((raw[:lo] == 0xFF).all()) and bool((raw[lo + self.numel:] == 0xFF).all()), "wrote outside out"
    return out.clone()

  def plain(self, misalign=0):
    """The yardstick: lr_lip_crop_collate_u8."""
    from lipreading_amd import _C
    from lipreading_amd.landmarks import _mouth
    H, W = self.hw
    return self._guarded(lambda out: _C.check(_C.lib().lr_lip_crop_collate_u8(
        self.frames_d.data_ptr(), self.lmk_d.data_ptr(), self.off_d.data_ptr(), self.lens_d.data_ptr(), out.data_ptr(),
        self.B, self.t_max, H, W, self.S, 68, _mouth.start, _mouth.stop, 0.3, _C.stream_handle()),
        "lr_lip_crop_collate_u8"), misalign)

  def augmented(self, clip, tmap, misalign=0):
    from lipreading_amd import _C
    from lipreading_amd.landmarks import _mouth
    H, W = self.hw
    clip_d = torch.from_numpy(np.ascontiguousarray(clip, dtype=np.float32)).to(self.dev)
    tmap_d = torch.from_numpy(np.ascontiguousarray(tmap, dtype=np.int32)).to(self.dev)
    return self._guarded(lambda out: _C.check(_C.lib().lr_lip_crop_collate_aug_u8(
        self.frames_d.data_ptr(), self.lmk_d.data_ptr(), self.off_d.data_ptr(), self.lens_d.data_ptr(),
        clip_d.data_ptr(), tmap_d.data_ptr(), out.data_ptr(), self.B, self.t_max, H, W, self.S, 68, _mouth.start,
        _mouth.stop, 0.3, _C.stream_handle()), "lr_lip_crop_collate_aug_u8"), misalign)

  def real(self):
    """bool [B][t_max]: the frames inside a sample's length."""
    return torch.from_numpy(np.arange(self.t_max)[None, :] < self.lens[:, None]).to(self.dev)


# ---- 1: identity ----------------------------------------------------------------------------------------------------
@grid
def test_identity_records_give_the_plain_kernels_bytes(dev, B, hw, S):
  c = Case(dev, B, hw, S)
  want = c.plain()
  assert int(want[0, 0].max()) > 0 and not bool(want[~c.real()].any())
  clip, tmap = AC.identity_records(c.lens)
  for misalign in (0, 1):
    got = c.augmented(clip, tmap, misalign)
    assert torch.equal(got, want), "differs in %d bytes (misalign %d)" % (int((got != want).sum()), misalign)
  assert torch.equal(c.plain(1), want)


# ---- 2: flip only ---------------------------------------------------------------------------------------------------
@grid
def test_flip_alone_mirrors_the_columns(dev, B, hw, S):
  c = Case(dev, B, hw, S)
  want = torch.flip(c.plain(), dims=[-1])          # (padding is zeros either way round)
  clip, tmap = AC.identity_records(c.lens)
  clip[:, 3] = 1.0
  for misalign in (0, 1):
    got = c.augmented(clip, tmap, misalign)
    assert torch.equal(got, want), "differs in %d bytes (misalign %d)" % (int((got != want).sum()), misalign)
    assert not bool(got[~c.real()].any())
  # and a per-clip flip touches the flipped clips only
  if B > 1:
    clip[::2, 3] = 0.0
    got = c.augmented(clip, tmap)
    assert torch.equal(got[1::2], want[1::2]) and torch.equal(got[::2], c.plain()[::2])


# ---- 3 / 5: map only ------------------------------------------------------------------------------------------------
def _mapped(c, base, tmap):
  """base[b, tmap] where the map is >= 0 (clamped to the sample), zeros where it is -1 and past the length."""
  want = torch.zeros_like(base)
  for b in range(c.B):
    lo, n = int(c.offsets[b]), int(c.lens[b])
    for t in range(n):
      m = int(tmap[lo + t])
      if m >= 0:
        want[b, t] = base[b, min(m, n - 1)]
  return want


@grid
def test_a_drawn_frame_map_gathers_and_masks_whole_frames(dev, B, hw, S):
  c = Case(dev, B, hw, S)
  base = c.plain()
  clip, _ = AC.identity_records(c.lens)
  for seed in range(64):                           # (short clips: take a draw that has what the test is about)
    _, tmap = _spec("tjitter=0.3,tmask=2x3", seed=seed).draw(0, np.arange(B), c.lens)
    if not np.array_equal(tmap, AC.identity_records(c.lens)[1]) and (
        B == 1 or ((tmap < 0).any() and (np.diff(tmap) == 0).any())):     # masked frames and doubled ones
      break
  else:
    raise AssertionError("no draw of 64 moves a frame")
  assert tmap.shape == (int(c.lens.sum()),)
  want = _mapped(c, base, tmap)
  for misalign in (0, 1):
    got = c.augmented(clip, tmap, misalign)
    assert torch.equal(got, want), "differs in %d bytes (misalign %d)" % (int((got != want).sum()), misalign)
  for b in range(B):
    lo, n = int(c.offsets[b]), int(c.lens[b])
    for t in range(c.t_max):
      if t >= n or tmap[lo + t] < 0:
        assert not bool(got[b, t].any()), (b, t)


@grid
def test_a_map_value_past_the_sample_reads_its_last_frame(dev, B, hw, S):
  c = Case(dev, B, hw, S)
  base = c.plain()
  clip, tmap = AC.identity_records(c.lens)
  b = int(np.argmax(c.lens[:-1])) if B > 1 else 0  # not the last sample of the buffer (B = 1: the spare row is behind it)
  lo, n = int(c.offsets[b]), int(c.lens[b])
  assert n > 1
  tmap[lo] = n                                     # one past the sample: an unclamped read would take the next sample's
  want = base.clone()
  want[b, 0] = base[b, n - 1]
  for misalign in (0, 1):
    got = c.augmented(clip, tmap, misalign)
    assert torch.equal(got, want), "differs in %d bytes (misalign %d)" % (int((got != want).sum()), misalign)
  if B > 1:
    assert not torch.equal(base[b + 1, 0], base[b, n - 1])   # what an unclamped read would have produced is another frame


# ---- 4: shift and zoom against the numpy restatement ------------------------------------------------------------------
@grid
@pytest.mark.parametrize("flip", [False, True])
def test_shift_and_zoom_match_the_numpy_restatement(dev, B, hw, S, flip):
  """Bar: max difference <= 1 LSB and fewer than 1e-3 of the pixels differing — the project's bar for the crop against
  its numpy oracle (test_lip_crop_matches_oracle); the restatement's own freedom (an a + b * c rounded once or twice)
  stays inside it (test_fused_and_plain_arithmetic_of_the_restatement_stay_within_the_gpu_tests_bar)."""
  c = Case(dev, B, hw, S)
  spec = _spec("shift=0.15,zoom=0.25" + (",flip=1" if flip else ""), seed=7 * B + S)
  clip, tmap = spec.draw(0, np.arange(B), c.lens)
  assert np.array_equal(tmap, AC.identity_records(c.lens)[1]) and (clip[:, 3] == float(flip)).all()
  assert (clip[:, 2] != 1).all() and (clip[:, :2] != 0).all()
  want = AC.augmented_batch(c.frames, c.lm, c.offsets, c.lens, clip, tmap, c.t_max, S)
  real = int(c.lens.sum()) * 3 * S * S
  for misalign in (0, 1):
    got = c.augmented(clip, tmap, misalign).cpu().numpy()
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float((diff > 0).sum()) / real
    print("B %d hw %r S %d flip %d misalign %d: max %d, differing %.3g" % (B, hw, S, flip, misalign, diff.max(), share))
    assert diff.max() <= 1 and share < 1e-3
    assert not got[~c.real().cpu().numpy()].any()
  # and it is not the un-augmented crop
  assert not np.array_equal(got, c.plain().cpu().numpy())


# ---- 6: the landmark entry point --------------------------------------------------------------------------------------
@pytest.mark.parametrize("feat", [204, 7])
@pytest.mark.parametrize("B", [1, 5, 32])
def test_landmark_entry_point_equals_the_numpy_gather(dev, B, feat):
  from lipreading_amd import _C
  L = _C.lib()
  rng = np.random.RandomState(31 * B + feat)
  t_max = 9
  lens = rng.randint(1, t_max + 1, B)
  lens[-1] = t_max
  if B > 1:
    lens[0] = 1
  rows = int(lens.sum())
  packed = rng.randn(rows + 1, feat).astype(np.float32)        # one spare row, as in Case
  offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  _, tmap = _spec("tjitter=0.3,tmask=2x3", seed=feat).draw(0, np.arange(B), lens)
  b = B // 2
  tmap[int(offsets[b])] = int(lens[b])                          # past the sample: clamped
  want = np.zeros((B, t_max, feat), np.float32)
  for i in range(B):
    lo, n = int(offsets[i]), int(lens[i])
    for t in range(n):
      m = int(tmap[lo + t])
      if m >= 0:
        want[i, t] = packed[lo + min(m, n - 1)]
  d = lambda a: torch.from_numpy(a).to(dev)
  packed_d, off_d, lens_d, tmap_d = d(packed), d(offsets), d(lens.astype(np.int32)), d(tmap)
  guard = 1024
  raw = torch.full((want.size + 2 * guard,), float("nan"), dtype=torch.float32, device=dev)
  raw.view(torch.int32).fill_(-1)
  out = raw[guard:guard + want.size].view(want.shape)
  _C.check(L.lr_collate_pad_aug_f32(packed_d.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(), tmap_d.data_ptr(),
                                    out.data_ptr(), B, t_max, feat, _C.stream_handle()), "lr_collate_pad_aug_f32")
  torch.cuda.synchronize()
  assert out.cpu().numpy().tobytes() == want.tobytes()
  ints = raw.view(torch.int32)
  assert bool((ints[:guard] == -1).all()) and bool((ints[guard + want.size:] == -1).all())
  # the identity map gives lr_collate_pad_f32's bytes
  ident = d(AC.identity_records(lens)[1])
  plain = torch.empty_like(out)
  _C.check(L.lr_collate_pad_f32(packed_d.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(), plain.data_ptr(), B, t_max,
                                feat, _C.stream_handle()), "lr_collate_pad_f32")
  _C.check(L.lr_collate_pad_aug_f32(packed_d.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(), ident.data_ptr(),
                                    out.data_ptr(), B, t_max, feat, _C.stream_handle()), "lr_collate_pad_aug_f32")
  torch.cuda.synchronize()
  assert torch.equal(out, plain)
  s = _C.stream_handle()
  assert L.lr_collate_pad_aug_f32(packed_d.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(), None, out.data_ptr(), B,
                                  t_max, feat, s) == _C.LR_ERR_INVALID_ARG


def test_bad_arguments_are_rejected_on_the_device_too(dev):
  from lipreading_amd import _C
  L = _C.lib()
  c = Case(dev, 5, (96, 96), 32)
  clip, tmap = AC.identity_records(c.lens)
  clip_d, tmap_d = torch.from_numpy(clip).to(dev), torch.from_numpy(tmap).to(dev)
  out = torch.empty(c.shape, dtype=torch.uint8, device=dev)
  ptrs = [c.frames_d.data_ptr(), c.lmk_d.data_ptr(), c.off_d.data_ptr(), c.lens_d.data_ptr(), clip_d.data_ptr(),
          tmap_d.data_ptr(), out.data_ptr()]
  s = _C.stream_handle()
  tail = (5, c.t_max, 96, 96, 32, 68, 48, 68, 0.3, s)
  assert L.lr_lip_crop_collate_aug_u8(*ptrs, *tail) == 0
  for i in (4, 5):                                 # NULL clip_aug / tmap
    args = list(ptrs)
    args[i] = None
    assert L.lr_lip_crop_collate_aug_u8(*args, *tail) == _C.LR_ERR_INVALID_ARG
  assert L.lr_lip_crop_collate_aug_u8(*ptrs, 0, c.t_max, 96, 96, 32, 68, 48, 68, 0.3, s) == _C.LR_ERR_INVALID_ARG
  assert L.lr_lip_crop_collate_aug_u8(*ptrs, 5, c.t_max, 96, 96, 32, 68, 48, 69, 0.3, s) == _C.LR_ERR_INVALID_ARG
  torch.cuda.synchronize()


# ---- 7: the loader ----------------------------------------------------------------------------------------------------
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


POLICY = "flip=0.5,shift=0.08,zoom=0.1,tjitter=0.05,tmask=2x10"


def _prefetch(dev, ds, batch, pixels, depth=2, workers=2, size=32, augment=None):
  from lipreading_amd.dataset import make_loader
  return make_loader(ds, batch, None, prefetch=depth, device=dev, pixels=pixels, size=size, workers=workers,
                     augment=augment)


def _entry_point_batch(dev, ds, lo, hi, pixels, size, spec, pass_no):
  """What the C entry point gives for samples [lo, hi) on spec.draw's records of `pass_no`."""
  from lipreading_amd import _C
  from lipreading_amd.landmarks import _mouth
  L = _C.lib()
  seqs = [ds[i][0] for i in range(lo, hi)]
  lens = np.array([len(s[0]) if pixels else len(s) for s in seqs], dtype=np.int64)
  clip, tmap = spec.draw(pass_no, range(lo, hi), lens)
  offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  off_d, lens_d, tmap_d = d(offsets), d(lens.astype(np.int32)), d(tmap)
  B, t_max = hi - lo, int(lens.max())
  if pixels:
    frames = d(np.concatenate([s[0] for s in seqs]))
    lmk = d(np.concatenate([np.asarray(s[1], dtype=np.float32) for s in seqs]))
    H, W = frames.shape[2], frames.shape[3]
    out = torch.empty((B, t_max, 3, size, size), dtype=torch.uint8, device=dev)
    _C.check(L.lr_lip_crop_collate_aug_u8(frames.data_ptr(), lmk.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(),
                                          d(clip).data_ptr(), tmap_d.data_ptr(), out.data_ptr(), B, t_max, H, W, size, 68,
                                          _mouth.start, _mouth.stop, 0.3, _C.stream_handle()),
             "lr_lip_crop_collate_aug_u8")
  else:
    packed = d(np.concatenate([np.asarray(s, dtype=np.float32).reshape(len(s), 204) for s in seqs]))
    out = torch.empty((B, t_max, 204), dtype=torch.float32, device=dev)
    _C.check(L.lr_collate_pad_aug_f32(packed.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(), tmap_d.data_ptr(),
                                      out.data_ptr(), B, t_max, 204, _C.stream_handle()), "lr_collate_pad_aug_f32")
    out = out.reshape(B, t_max, 68, 3)
  torch.cuda.synchronize()
  return out, (clip, tmap)


def _assert_same_meta(got, want, where):
  assert len(got) == len(want) == 4
  for i, (a, b) in enumerate(zip(got, want)):
    assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, (where, i, a.dtype, b.dtype, a.shape,
                                                                               b.shape, a.device, b.device)
    if i:
      assert torch.equal(a, b), (where, i)          # frame_lens, chars, char_lens


@pytest.mark.parametrize("pixels", [False, True])
def test_augmented_prefetch_loader(dev, pixels):
  ds = _pixel_dataset(23, seed=11) if pixels else _landmark_dataset(23, seed=11)
  spec = _spec(POLICY, seed=5)
  clean = _prefetch(dev, ds, 4, pixels)
  one = _prefetch(dev, ds, 4, pixels, depth=1, workers=1, augment=spec)
  two = _prefetch(dev, ds, 4, pixels, depth=3, workers=4, augment=_spec(POLICY, seed=5))
  assert len(one) == len(two) == len(clean) == len(one.plain()) == 6
  touched = 0
  for p in range(3):
    assert one.pass_no == two.pass_no == p
    n = 0
    for k, (a, b, want) in enumerate(zip(one, two, clean)):
      _assert_same_meta(a, want, (p, k, "one"))
      _assert_same_meta(b, want, (p, k, "two"))
      assert a[0].is_cuda and not a[1].is_cuda and not a[2].is_cuda and not a[3].is_cuda
      assert torch.equal(a[0], b[0]), (p, k)        # one seed, whatever the depth and the workers
      lo, hi = one.host.plan[k]
      direct, _ = _entry_point_batch(dev, ds, lo, hi, pixels, 32, spec, p)
      assert torch.equal(a[0], direct), (p, k)      # the C entry point on spec.draw's records of this pass
      touched += int(not torch.equal(a[0], want[0]))
      n += 1
    assert n == 6
  assert touched >= 12                              # the augmentation reached the batches
  first = [x[0].clone() for x in _at_pass(one, 0)]
  second = [x[0].clone() for x in _at_pass(one, 1)]
  assert any(not torch.equal(a, b) for a, b in zip(first, second))      # two passes differ
  assert all(torch.equal(a, b[0]) for a, b in zip(first, _at_pass(two, 0)))
  # plain(): the un-augmented loader bit for bit, and the pass number stays
  one.set_pass(4)
  for _ in range(2):
    n = 0
    for k, (got, want) in enumerate(zip(one.plain(), clean)):
      _assert_same_meta(got, want, ("plain", k))
      assert torch.equal(got[0], want[0]), k
      n += 1
    assert n == 6 and one.pass_no == 4
  for got in one:                                   # an abandoned augmented pass takes its number
    break
  assert one.pass_no == 5
  for x in (one, two, clean):
    x.close()


def _at_pass(loader, n):
  loader.set_pass(n)
  return list(loader)


# ---- 8: training through it -------------------------------------------------------------------------------------------
def _train_run(dev, loader, pixels, epochs, graphs_on, size=32):
  """tests/test_gpu_loader.py's _train_run protocol (grad_norm=None: the clipped step is not run-to-run deterministic,
  DESIGN.md "Prefetching loader"), returning what this file asserts on."""
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
  losses, skipped = [], 0
  for _ in range(epochs):
    losses.append(T.train(model, None, loader, opt, dev, c2i, grad_norm=None, graphs=graphs)[1])
    skipped += T.last_epoch_stats["skipped"]
  if graphs_on:
    assert graphs.captures >= 1 and graphs.replays >= 1      # the step really ran as a hipGraph
  state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
  return dict(losses=losses, state=state, skipped=skipped, captures=graphs.captures)


@pytest.mark.parametrize("regime", ["R", "X"])
def test_training_through_the_augmented_loader(dev, regime):
  """Regime R: landmarks, hipGraphs on (the frame map alone applies); regime X: pixels at a small crop size, eager."""
  pixels = regime == "X"
  lens = np.repeat([21, 24, 27, 30], 4)[:15]                  # few distinct batch shapes (graphs replay), ragged end
  ds = _pixel_dataset(15, seed=17, lens=lens) if pixels else _landmark_dataset(15, seed=17, lens=lens)
  epochs = 4
  clean = _prefetch(dev, ds, 4, pixels)
  base = _train_run(dev, clean, pixels, epochs, graphs_on=not pixels)
  clean.close()
  runs = []
  for _ in range(2):
    loader = _prefetch(dev, ds, 4, pixels, augment=_spec(POLICY, seed=3))
    runs.append(_train_run(dev, loader, pixels, epochs, graphs_on=not pixels))
    assert loader.pass_no == epochs
    loader.close()
  a, b = runs
  print("regime %s losses: clean %r | augmented %r | augmented again %r" % (regime, base["losses"], a["losses"],
                                                                           b["losses"]))
  assert all(np.isfinite(a["losses"])) and all(np.isfinite(base["losses"]))
  assert a["losses"] == b["losses"]
  for k in a["state"]:
    assert torch.equal(a["state"][k], b["state"][k]), k
  assert a["skipped"] == b["skipped"] == base["skipped"] == 0
  assert a["captures"] == b["captures"] == base["captures"]   # the batch shapes are the un-augmented loader's
  assert all(x != y for x, y in zip(a["losses"], base["losses"]))   # the augmentation reached the model


# ---- 9 / 10: not slower -------------------------------------------------------------------------------------------------
def _bench_tool():
  spec = importlib.util.spec_from_file_location("bench_loader", os.path.join(ROOT, "tools", "bench_loader.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_augmenting_kernel_is_not_slower_than_the_plain_one_on_the_same_bytes(dev):
  """B = 32, T = 75, 96 x 96 -> 96, device events, arms alternated in one call, 10 repeats.  With a policy that touches
  the same bytes per frame as the plain launch (no zoom, no masks) the extra work is one 16-byte record per sample and
  one int32 per frame: the augmenting launch's median may not exceed the plain launch's by more than the plain arm's own
  min-max spread.  Zoom widens the gather's footprint and masks remove work: timed and printed, not asserted."""
  tool = _bench_tool()
  assert tool.SAME_BYTES_POLICY == "flip=0.5,shift=0.08,tjitter=0.05"
  res = tool.time_kernel(dev, batch=32, size=96, hw=96, reps=10, augment=_spec(tool.SAME_BYTES_POLICY, seed=1))
  other = tool.time_kernel(dev, batch=32, size=96, hw=96, reps=10,
                           augment=_spec("flip=0.5,shift=0.08,tjitter=0.05,zoom=0.1,tmask=2x10", seed=1))
  for name, r in (("same bytes", res), ("zoom and masks (not asserted)", other)):
    print(name, {k: r[k] for k in ("collate_one_launch_ms", "augmented_one_launch_ms", "masked_frames")})
  assert res["masked_frames"] == 0 and res["augmented_one_launch_ms"]["n"] == res["collate_one_launch_ms"]["n"] == 10
  new, old = res["augmented_one_launch_ms"], res["collate_one_launch_ms"]
  assert new["median"] <= old["median"] + (old["max"] - old["min"]), res


def test_augmented_loop_is_not_slower_than_the_prefetched_loop(dev):
  """Regime X at the reduced length of test_prefetched_loop_is_not_slower_than_the_plain_loop_at_the_bench_shape: the
  augmented loader's median may not exceed the prefetched loader's by more than that arm's own min-max spread.  Regime
  R's step is host-bound (0.44 ms) and the draws run on worker threads under the GIL: measured and printed."""
  tool = _bench_tool()
  spec = _spec(POLICY, seed=1)
  res = tool.time_arms("X", dev, batch=32, n_batches=5, repeats=5, size=96, hw=96, depth=2, workers=2, augment=spec)
  print("X ms per step:", {k: res[k] for k in ("plain", "prefetch", "augmented", "resident")})
  r = tool.time_arms("R", dev, batch=32, n_batches=200, repeats=5, depth=2, workers=2, augment=spec)
  print("R ms per step (not asserted):", {k: r[k] for k in ("plain", "prefetch", "augmented", "resident")})
  print("host ms per batch in AugmentSpec.draw:", tool.time_draw(spec))
  fast, aug = res["prefetch"], res["augmented"]
  assert aug["median"] <= fast["median"] + (fast["max"] - fast["min"]), res
