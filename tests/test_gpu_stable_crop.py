"""GPU: lr_lip_stable_collate_u8, landmarks.lip_crop_stable, make_pixel_collate_fn(crop="stable") and
PrefetchLoader(crop="stable").  The yardstick is the numpy restatement (tests/stable_crop_cases.py) or existing code
(lr_lip_crop_collate_u8, today's loaders), never the new code.  The pose has one right answer and is compared bit for
bit; pixels against the restatement carry the project's bar for the crop (<= 1 LSB, fewer than 1e-3 of the real pixels
differing: the restatement's own freedom stays inside it, tests/test_stable_crop_cpu.py); everything the kernel
promises about itself (flip, frame map, padding) is exact.  The host side is tests/test_stable_crop_cpu.py."""
import numpy as np
import pytest
import torch

from tests import stable_crop_cases as SC

pytestmark = pytest.mark.gpu

GUARD = 4096                                       # a multiple of 256: an aligned out takes the vector path
EXTENT = 1.5                                       # (no test depends on the driver's default)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _spec(text, seed=0):
  from lipreading_amd.augment import AugmentSpec
  return AugmentSpec.parse(text, seed=seed)


class Case(object):
  """One batch on the device.  The frame and landmark buffers carry one spare row behind the last sample, so that no
  map value the tests use could leave the allocation even if it were not clamped.  out, pose and the workspace lie
  between guard bytes, which every call checks."""

  def __init__(self, dev, data, S, t_max=SC.T_MAX):
    self.dev, self.S, self.t_max = dev, S, t_max
    self.frames, self.lm, self.offsets, self.lens = data
    self.B, self.rows = len(self.lens), int(self.lens.sum())
    self.hw = self.frames.shape[2:]
    spare_f = np.concatenate([self.frames, np.full_like(self.frames[:1], 0x55)])
    spare_l = np.concatenate([self.lm, self.lm[:1]])
    self.frames_d, self.lmk_d = torch.from_numpy(spare_f).to(dev), torch.from_numpy(spare_l).to(dev)
    self.off_d = torch.from_numpy(self.offsets).to(dev)
    self.lens_d = torch.from_numpy(self.lens.astype(np.int32)).to(dev)
    self.shape = (self.B, t_max, 3, S, S)
    self.numel = int(np.prod(self.shape))
    self.real_px = self.rows * 3 * S * S

  def _guarded_u8(self, n, misalign=0):
    raw = torch.full((n + 2 * GUARD + 16,), 0xFF, dtype=torch.uint8, device=self.dev)
    lo = GUARD + misalign
    assert raw.data_ptr() % 256 == 0
    return raw, raw[lo:lo + n]

  @staticmethod
  def _intact(raw, view):
    lo = view.data_ptr() - raw.data_ptr()
    return bool((raw[:lo] == 0xFF).all()) and bool((raw[lo + view.numel():] == 0xFF).all())

  def stable(self, clip=None, tmap=None, radius=2, extent=EXTENT, misalign=0):
    """-> (out u8 [B][t_max][3][S][S], pose f32 [rows][4]) of one call, guards checked."""
    from lipreading_amd import _C
    L = _C.lib()
    H, W = self.hw
    clip_d = None if clip is None else torch.from_numpy(np.ascontiguousarray(clip, dtype=np.float32)).to(self.dev)
    tmap_d = None if tmap is None else torch.from_numpy(np.ascontiguousarray(tmap, dtype=np.int32)).to(self.dev)
    need = L.lr_lip_stable_workspace_bytes(self.rows, radius)
    assert need >= self.rows * 32
    raw_o, out = self._guarded_u8(self.numel, misalign)
    raw_p, pose = self._guarded_u8(self.rows * 16)
    raw_w, work = self._guarded_u8(need)
    assert out.data_ptr() % 16 == misalign and work.data_ptr() % 16 == 0
    _C.check(L.lr_lip_stable_collate_u8(
        self.frames_d.data_ptr(), self.lmk_d.data_ptr(), self.off_d.data_ptr(), self.lens_d.data_ptr(), _C.ptr(clip_d),
        _C.ptr(tmap_d), out.data_ptr(), pose.data_ptr(), work.data_ptr(), need, self.B, self.rows, self.t_max, H, W,
        self.S, 68, 48, 68, 36, 42, 42, 48, float(extent), int(radius), _C.stream_handle()), "lr_lip_stable_collate_u8")
    torch.cuda.synchronize()
    assert self._intact(raw_o, out), "wrote outside out"
    assert self._intact(raw_p, pose), "wrote outside pose"
    assert self._intact(raw_w, work), "wrote outside the workspace"
    return out.view(self.shape).clone(), pose.view(torch.float32).view(self.rows, 4).clone()

  def box(self, margin=0.3):
    """Existing code: lr_lip_crop_collate_u8."""
    from lipreading_amd import _C
    H, W = self.hw
    out = torch.empty(self.shape, dtype=torch.uint8, device=self.dev)
    _C.check(_C.lib().lr_lip_crop_collate_u8(
        self.frames_d.data_ptr(), self.lmk_d.data_ptr(), self.off_d.data_ptr(), self.lens_d.data_ptr(), out.data_ptr(),
        self.B, self.t_max, H, W, self.S, 68, 48, 68, float(margin), _C.stream_handle()), "lr_lip_crop_collate_u8")
    torch.cuda.synchronize()
    return out

  def real(self):
    """bool [B][t_max]: the frames inside a sample's length."""
    return torch.from_numpy(np.arange(self.t_max)[None, :] < self.lens[:, None]).to(self.dev)


def _bar(c, got, want, what):
  worst, share = SC.within_bar(got.cpu().numpy() if torch.is_tensor(got) else got,
                               want.cpu().numpy() if torch.is_tensor(want) else want, c.real_px)
  print("%s: max %d, differing %.3g" % (what, worst, share))
  assert worst <= 1 and share < 1e-3, (what, worst, share)


# ---- 1 / 2: pose and pixels against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 2, 8])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("hw", [(96, 96), (120, 160)])
@pytest.mark.parametrize("S", [32, 36, 30])                    # 16 / 4 / 1 pixels per store
def test_pose_is_bit_identical_and_pixels_match_the_restatement(dev, S, hw, B, radius):
  c = Case(dev, SC.stable_case(B, hw, S, roll=20.0 if B > 1 or radius else 0.0), S)
  poses = SC.smoothed_poses(c.lm, c.offsets, c.lens, radius)
  spec = _spec("shift=0.15,zoom=0.25" + (",flip=1" if radius == 2 else ""), seed=7 * B + S)
  clip, tmap = spec.draw(0, np.arange(B), c.lens)
  assert (clip[:, 2] != 1).all() and (clip[:, :2] != 0).all() and np.array_equal(tmap, SC.identity_records(c.lens)[1])
  hole = ~c.real()
  plain = None
  for name, (cl, tm) in (("identity", (None, None)), ("drawn", (clip, tmap))):
    want, _ = SC.stable_batch(c.frames, c.lm, c.offsets, c.lens, cl, tm, c.t_max, S, extent=EXTENT, fused=True,
                              poses=poses)
    for misalign in (0, 1):
      got, pose = c.stable(cl, tm, radius=radius, misalign=misalign)
      assert pose.cpu().numpy().tobytes() == poses.tobytes(), "pose differs in %d values" % int(
          (pose.cpu().numpy().view(np.int32) != poses.view(np.int32)).sum())
      _bar(c, got, want, "S %d hw %r B %d radius %d %s misalign %d" % (S, hw, B, radius, name, misalign))
      assert not bool(got[hole].any())                         # padding frames are zeros
      if plain is None:
        plain = got
      elif name == "identity":
        assert torch.equal(got, plain)                         # the 1-pixel stores give the vector stores' bytes
    assert int(got[0, 0].max()) > 0
  assert not torch.equal(got, plain)                           # the record reached the pixels
  # the identity record given explicitly is the NULL record
  ident = SC.identity_records(c.lens)
  assert torch.equal(c.stable(ident[0], ident[1], radius=radius)[0], plain)


def test_masked_frames_are_zero(dev):
  c = Case(dev, SC.stable_case(5, (96, 96), 32, roll=20.0), 32)
  clip, tmap = SC.identity_records(c.lens)
  base, _ = c.stable(clip, tmap)
  lo = int(c.offsets[4])
  tmap[lo + 1] = tmap[lo + 3] = -1
  got, _ = c.stable(clip, tmap)
  want = base.clone()
  want[4, 1] = 0
  want[4, 3] = 0
  assert torch.equal(got, want) and bool(base[4, 1].any())


# ---- 3: against existing code -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("hw", [(96, 96), (120, 160)])
@pytest.mark.parametrize("S", [32, 36, 30])
def test_level_eyes_at_the_box_rules_scale_give_the_box_kernels_crop(dev, S, hw, B):
  c = Case(dev, SC.level_case(B, hw, S, margin=0.3, extent=2.0), S)
  want = c.box(margin=0.3)
  for misalign in (0, 1):
    got, _ = c.stable(radius=0, extent=2.0, misalign=misalign)
    _bar(c, got, want, "S %d hw %r B %d misalign %d against lr_lip_crop_collate_u8" % (S, hw, B, misalign))
    assert not bool(got[~c.real()].any())
  assert len(torch.unique(want)) > 50


# ---- 4: the frame map ---------------------------------------------------------------------------------------------------
def _mapped(c, base, tmap):
  want = torch.zeros_like(base)
  for b in range(c.B):
    lo, n = int(c.offsets[b]), int(c.lens[b])
    for t in range(n):
      m = int(tmap[lo + t])
      if m >= 0:
        want[b, t] = base[b, min(m, n - 1)]
  return want


@pytest.mark.parametrize("S", [32, 36, 30])
@pytest.mark.parametrize("radius", [0, 2])
def test_frame_map_gathers_whole_frames_with_their_own_poses(dev, S, radius):
  c = Case(dev, SC.stable_case(5, (96, 96), S, roll=20.0), S)
  base, base_pose = c.stable(radius=radius)
  clip, ident = SC.identity_records(c.lens)
  # a value past the sample reads the sample's last row and ITS pose, never the next sample's
  b = int(np.argmax(c.lens[:-1]))
  lo, n = int(c.offsets[b]), int(c.lens[b])
  assert n > 1
  tmap = ident.copy()
  tmap[lo] = n
  want = base.clone()
  want[b, 0] = base[b, n - 1]
  for misalign in (0, 1):
    got, pose = c.stable(clip, tmap, radius=radius, misalign=misalign)
    assert torch.equal(got, want), "differs in %d bytes" % int((got != want).sum())
    assert torch.equal(pose, base_pose)                        # the pose belongs to the rows, not to the map
  assert not torch.equal(base[b + 1, 0], base[b, n - 1])
  # a drawn time-jitter map with masks: exactly the identity call's frames at the mapped rows
  for seed in range(64):
    _, tmap = _spec("tjitter=0.3,tmask=2x3", seed=seed).draw(0, np.arange(5), c.lens)
    if (tmap < 0).any() and (np.diff(tmap) == 0).any():
      break
  else:
    raise AssertionError("no draw of 64 masks and doubles a frame")
  got, _ = c.stable(clip, tmap, radius=radius)
  assert torch.equal(got, _mapped(c, base, tmap))


# ---- 5: flip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 36, 30])
def test_flip_is_the_unflipped_output_with_its_columns_reversed(dev, S):
  c = Case(dev, SC.stable_case(5, (120, 160), S, roll=20.0), S)
  clip, tmap = _spec("shift=0.15,zoom=0.25", seed=S).draw(0, np.arange(5), c.lens)
  for rec in (SC.identity_records(c.lens)[0], clip):
    straight, _ = c.stable(rec, tmap)
    flipped = rec.copy()
    flipped[:, 3] = 1.0
    for misalign in (0, 1):
      got, _ = c.stable(flipped, tmap, misalign=misalign)
      assert torch.equal(got, torch.flip(straight, dims=[-1])), (S, misalign)
    flipped[::2, 3] = 0.0                                      # a per-clip flip touches the flipped clips only
    got, _ = c.stable(flipped, tmap)
    assert torch.equal(got[1::2], torch.flip(straight, dims=[-1])[1::2]) and torch.equal(got[::2], straight[::2])


# ---- 6: what the feature is for -------------------------------------------------------------------------------------------
def test_a_mouth_that_opens_and_closes_moves_the_box_crop_and_not_the_stable_one(dev):
  """The mouth points of a clip wobble — the widest and the tallest pair of points move apart and back, frame by frame —
  while their mean and the eyes stay put (the points lie on a 1/1024 grid and move by quarter pixels, so the mean does
  not change by a bit).  radius = 0: nothing is smoothed away."""
  S = 32
  frames, lm, offsets, lens = SC.stable_case(1, (96, 96), S, roll=20.0)
  lm[:, 48:68, :2] = np.round(lm[:, 48:68, :2] * 1024) / 1024
  wob = lm.copy()
  rng = np.random.RandomState(3)
  for n in range(len(lm)):
    for axis in (0, 1):
      v = wob[n, 48:68, axis]
      hi, lo_ = int(np.argmax(v)), int(np.argmin(v))
      if hi == lo_:
        lo_ = (hi + 1) % 20
      delta = np.float32(0.25 * rng.randint(4, 17))             # 1 .. 4 px
      v[hi] += delta
      v[lo_] -= delta
  assert SC.in_exact_range(wob) and not np.array_equal(wob, lm)
  assert np.array_equal(wob[:, :48], lm[:, :48])               # the eyes (and everything else) are where they were
  still, moving = Case(dev, (frames, lm, offsets, lens), S), Case(dev, (frames, wob, offsets, lens), S)
  a, pose_a = still.stable(radius=0)
  b, pose_b = moving.stable(radius=0)
  assert torch.equal(pose_a, pose_b)                           # the mouth mean is held fixed
  _bar(still, b, a, "stable crop, wobbling mouth against still mouth")
  box_a, box_b = still.box(), moving.box()
  changed = float((box_a != box_b).float().mean())
  print("box crop: share of pixels the wobble changed %.3f" % changed)
  assert changed > 0.5                                         # the box follows the mouth


# ---- 7: the grid stride ---------------------------------------------------------------------------------------------------
def test_more_pairs_than_the_grid_cap(dev):
  B, S = 300, 16                                               # 2100 (sample, frame) pairs > 2048 workgroups
  c = Case(dev, SC.stable_case(B, (32, 32), S, roll=20.0), S)
  assert c.B * c.t_max > 2048
  clip, tmap = _spec("shift=0.1,zoom=0.2,flip=0.5", seed=2).draw(0, np.arange(B), c.lens)
  want, poses = SC.stable_batch(c.frames, c.lm, c.offsets, c.lens, clip, tmap, c.t_max, S, extent=EXTENT, radius=2,
                                fused=True)
  for misalign in (0, 1):
    got, pose = c.stable(clip, tmap, radius=2, misalign=misalign)
    assert pose.cpu().numpy().tobytes() == poses.tobytes()
    _bar(c, got, want, "grid stride, misalign %d" % misalign)
    assert not bool(got[~c.real()].any())
    tail = got.view(-1, 3, S, S)[2048:].cpu().numpy()          # the pairs a second trip of the stride makes
    assert tail.any() and np.abs(tail.astype(np.int16) - want.reshape(-1, 3, S, S)[2048:].astype(np.int16)).max() <= 1


# ---- 8: Python, up to the loader ------------------------------------------------------------------------------------------
def test_lip_crop_stable_is_the_batch_entry_for_one_clip(dev):
  from lipreading_amd import landmarks
  c = Case(dev, SC.stable_case(1, (96, 96), 32, roll=20.0), 32)
  want, want_pose = c.stable(radius=2, extent=1.25)
  f, l = torch.from_numpy(c.frames).to(dev), torch.from_numpy(c.lm).to(dev)
  got, pose = landmarks.lip_crop_stable(f, l, size=32, return_pose=True)
  assert got.shape == (c.rows, 3, 32, 32) and got.dtype == torch.uint8 and pose.shape == (c.rows, 4)
  assert torch.equal(got, want[0]) and torch.equal(pose, want_pose)
  assert torch.equal(landmarks.lip_crop_stable(f, l, size=32), got)
  other = landmarks.lip_crop_stable(f, l.double(), size=32, extent=EXTENT, radius=0)
  assert torch.equal(other, c.stable(radius=0)[0][0]) and not torch.equal(other, got)


def _caption(rng, n):
  return np.array([1] + list(rng.randint(4, 64, n)) + [2])


def _pixel_dataset(n, seed, hw=(48, 64)):
  rng = np.random.RandomState(seed)
  H, W = hw
  out = []
  for t in np.sort(rng.randint(12, 30, n)):
    t = int(t)
    lmk = np.zeros((t, 68, 3))
    lmk[:, :, 0] = rng.uniform(0.1, 0.9, (t, 68)) * W
    lmk[:, :, 1] = rng.uniform(0.1, 0.9, (t, 68)) * H
    lmk[:, 48:68, 0] = rng.uniform(0.35, 0.65, (t, 20)) * W
    lmk[:, 48:68, 1] = rng.uniform(0.55, 0.8, (t, 20)) * H
    lmk[:, 36:42, 0], lmk[:, 42:48, 0] = rng.uniform(0.25, 0.35, (t, 6)) * W, rng.uniform(0.65, 0.75, (t, 6)) * W
    lmk[:, 36:48, 1] = rng.uniform(0.3, 0.45, (t, 12)) * H
    out.append(((rng.randint(0, 256, (t, 3, H, W)).astype(np.uint8), lmk), _caption(rng, rng.randint(2, 6))))
  return out


def _same_batches(got, want, where):
  got, want = list(got), list(want)
  assert len(got) == len(want) > 0
  for k, (a, b) in enumerate(zip(got, want)):
    assert len(a) == len(b) == 4
    for i, (x, y) in enumerate(zip(a, b)):
      assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (where, k, i)
      assert torch.equal(x, y), (where, k, i)
  return got


def test_loaders_yield_the_stable_collates_batches(dev):
  from lipreading_amd.data import make_pixel_collate_fn
  from lipreading_amd.dataset import make_loader
  ds = _pixel_dataset(23, seed=11)
  args = dict(device=dev, pixels=True, size=32)
  stable = dict(crop="stable", extent=EXTENT, radius=3)
  collate = make_pixel_collate_fn(dev, size=32, **stable)
  plain = list(make_loader(ds, 4, collate))                    # ONE call of the batch entry per batch
  assert len(plain) == 6 and plain[0][0].shape[2:] == (3, 32, 32) and plain[0][0].dtype == torch.uint8
  # ... which is the C entry point on the ragged upload
  seqs = [ds[i][0] for i in range(4)]
  c = Case(dev, (np.concatenate([s[0] for s in seqs]), np.concatenate([s[1] for s in seqs]).astype(np.float32),
                 np.concatenate([[0], np.cumsum([len(s[0]) for s in seqs])[:-1]]).astype(np.int64),
                 np.array([len(s[0]) for s in seqs], dtype=np.int64)), 32, t_max=max(len(s[0]) for s in seqs))
  assert torch.equal(plain[0][0], c.stable(radius=3)[0])
  pre = make_loader(ds, 4, None, prefetch=2, workers=2, **args, **stable)
  for _ in range(2):                                           # re-iterable, the slots' workspace is reused
    _same_batches(pre, plain, "prefetch")
  spec = _spec("flip=0.5,shift=0.08,zoom=0.1,tjitter=0.05,tmask=2x10", seed=5)
  aug = make_loader(ds, 4, None, prefetch=2, workers=2, augment=spec, **args, **stable)
  first = list(aug)
  assert sum(not torch.equal(a[0], b[0]) for a, b in zip(first, plain)) >= 4    # the augmentation reached the batches
  _same_batches(aug.plain(), plain, "plain pass of the augmented loader")
  # the augmented pass is the C entry point on spec.draw's records
  clip, tmap = spec.draw(0, range(4), c.lens)
  assert torch.equal(first[0][0], c.stable(clip, tmap, radius=3)[0])
  # crop="box" is today's loader, and the stable crop is another crop
  today = list(make_loader(ds, 4, make_pixel_collate_fn(dev, size=32)))
  _same_batches(make_loader(ds, 4, make_pixel_collate_fn(dev, size=32, crop="box")), today, "box collate")
  box = make_loader(ds, 4, None, prefetch=2, workers=2, crop="box", **args)
  _same_batches(box, today, "box prefetch")
  _same_batches(make_loader(ds, 4, None, prefetch=2, workers=2, **args), today, "default prefetch")
  assert not torch.equal(today[0][0], plain[0][0])
  for x in (pre, aug, box):
    x.close()


# ---- 9: bad arguments ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_on_the_device_too(dev):
  from lipreading_amd import _C
  L = _C.lib()
  c = Case(dev, SC.stable_case(5, (96, 96), 32), 32)
  clip, tmap = SC.identity_records(c.lens)
  clip_d, tmap_d = torch.from_numpy(clip).to(dev), torch.from_numpy(tmap).to(dev)
  out = torch.empty(c.shape, dtype=torch.uint8, device=dev)
  pose = torch.empty((c.rows, 4), dtype=torch.float32, device=dev)
  need = L.lr_lip_stable_workspace_bytes(c.rows, 2)
  work = torch.empty(need, dtype=torch.uint8, device=dev)
  ptrs = [c.frames_d.data_ptr(), c.lmk_d.data_ptr(), c.off_d.data_ptr(), c.lens_d.data_ptr(), clip_d.data_ptr(),
          tmap_d.data_ptr(), out.data_ptr(), pose.data_ptr(), work.data_ptr()]
  s = _C.stream_handle()
  good = dict(nbytes=need, B=5, rows=c.rows, t_max=c.t_max, H=96, W=96, S=32, npts=68, lo=48, hi=68, ea_lo=36, ea_hi=42,
              eb_lo=42, eb_hi=48, extent=1.25, radius=2)

  def call(p, **change):
    t = dict(good)
    t.update(change)
    return L.lr_lip_stable_collate_u8(*p, *[t[k] for k in good], s)

  assert call(ptrs) == 0
  no_pose = list(ptrs)
  no_pose[7] = None
  assert call(no_pose) == 0                                    # pose is optional
  both = list(ptrs)
  both[4] = both[5] = None
  assert call(both) == 0                                       # and so are the records, together
  for i in (0, 1, 2, 3, 4, 5, 6, 8):                           # required pointers; clip_aug without tmap and the reverse
    args = list(ptrs)
    args[i] = None
    assert call(args) == _C.LR_ERR_INVALID_ARG, i
  for change in (dict(B=0), dict(rows=0), dict(hi=69), dict(hi=48), dict(ea_hi=36), dict(eb_lo=48, eb_hi=48),
                 dict(eb_hi=69), dict(extent=0.0), dict(extent=-1.0), dict(extent=float("inf")),
                 dict(extent=float("nan")), dict(radius=-1), dict(radius=_C.LR_LIP_STABLE_MAX_RADIUS + 1)):
    assert call(ptrs, **change) == _C.LR_ERR_INVALID_ARG, change
  assert call(ptrs, nbytes=need - 1) == _C.LR_ERR_WORKSPACE
  assert call(ptrs, radius=_C.LR_LIP_STABLE_MAX_RADIUS) == 0
  torch.cuda.synchronize()
