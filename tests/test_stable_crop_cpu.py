"""CPU: the declarations of lr_lip_stable_collate_u8 / lr_lip_stable_workspace_bytes and their derived ctypes
signatures, the argument checks that need no device, the compiled resources of lr_lip_stable.hip, the numpy restatement
the GPU file grades against (tests/stable_crop_cases.py) and the driver's --crop flags.  The device stage is
tests/test_gpu_stable_crop.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from lipreading_amd import _build, _C
from lipreading_amd.augment import AugmentSpec
from tests import stable_crop_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header and bindings --------------------------------------------------------------------------------------------
def _declaration(ret, name):
  text = open(os.path.join(ROOT, "include", "lipreading_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), text)
  assert m, "include/lipreading_hip.h does not declare %s %s" % (ret, name)
  return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
  params = _declaration("int", "lr_lip_stable_collate_u8")
  restype, argtypes = _C.SIGNATURES["lr_lip_stable_collate_u8"]
  assert restype is _C.c_int and len(params) == len(argtypes) == 26
  names = [p.split()[-1].lstrip("*") for p in params]
  assert names == ["frames", "lmk", "offsets", "lens", "clip_aug", "tmap", "out", "pose", "workspace", "workspace_bytes",
                   "B", "rows", "t_max", "H", "W", "S", "npts", "lo", "hi", "ea_lo", "ea_hi", "eb_lo", "eb_hi", "extent",
                   "radius", "stream"]
  import ctypes
  for decl, ctype in zip(params, argtypes):
    if "*" in decl or decl.startswith("lr_stream_t"):
      assert ctype is _C.P, decl
    elif decl.startswith("float"):
      assert ctype is _C.c_float, decl
    elif decl.startswith("size_t"):
      assert ctype is ctypes.c_size_t, decl
    elif decl.startswith("int64_t"):
      assert ctype is ctypes.c_int64, decl
    else:
      assert decl.startswith("int ") and ctype is _C.c_int, decl
  assert _declaration("size_t", "lr_lip_stable_workspace_bytes") == ["int64_t rows", "int radius"]
  assert _C.SIGNATURES["lr_lip_stable_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
  assert _C.LR_LIP_STABLE_MAX_RADIUS == 32


GOOD_TAIL = dict(B=1, rows=1, t_max=1, H=8, W=8, S=4, npts=68, lo=48, hi=68, ea_lo=36, ea_hi=42, eb_lo=42, eb_hi=48,
                 extent=1.25, radius=2)


def _call(L, ptrs, nbytes=4096, stream=None, **change):
  t = dict(GOOD_TAIL)
  t.update(change)
  return L.lr_lip_stable_collate_u8(*ptrs, nbytes, *[t[k] for k in GOOD_TAIL], stream)


BAD = [dict(B=0), dict(rows=0), dict(t_max=0), dict(H=0), dict(W=0), dict(S=0), dict(npts=0), dict(lo=-1), dict(hi=48),
       dict(hi=69), dict(ea_lo=-1), dict(ea_hi=36), dict(ea_hi=69), dict(eb_lo=48, eb_hi=48), dict(eb_hi=69),
       dict(extent=0.0), dict(extent=-1.0), dict(extent=float("inf")), dict(extent=float("nan")), dict(radius=-1),
       dict(radius=33), dict(B=1 << 20, t_max=1 << 12), dict(S=1 << 15), dict(H=1 << 15, W=1 << 15)]


def test_bad_arguments_are_rejected_without_a_device():
  _build.build_library()
  L = _C.lib()
  one = 4096                       # any non-NULL, 16-byte aligned value: the checks return before a pointer is used
  #        frames lmk offsets lens clip_aug tmap out pose workspace
  good = [one] * 9
  for i in (0, 1, 2, 3, 6, 8):     # each required pointer alone
    args = list(good)
    args[i] = None
    assert _call(L, args) == -1, i
  for i in (4, 5):                 # clip_aug without tmap and tmap without clip_aug
    args = list(good)
    args[i] = None
    assert _call(L, args) == -1, i
  for change in BAD:
    assert _call(L, good, **change) == -1, change
  misaligned = list(good)
  misaligned[8] = one + 4
  assert _call(L, misaligned) == -1
  assert _call(L, good, nbytes=16) == _C.LR_ERR_WORKSPACE       # smaller than lr_lip_stable_workspace_bytes
  # the workspace: 0 for what the entry rejects, otherwise room for two poses per row
  assert L.lr_lip_stable_workspace_bytes(0, 2) == 0 and L.lr_lip_stable_workspace_bytes(-5, 2) == 0
  assert L.lr_lip_stable_workspace_bytes(10, -1) == 0 and L.lr_lip_stable_workspace_bytes(10, 33) == 0
  for rows in (1, 7, 2400):
    for radius in (0, 2, 32):
      assert L.lr_lip_stable_workspace_bytes(rows, radius) >= rows * 32


# ---- compiled resources ---------------------------------------------------------------------------------------------
def test_stable_kernels_compile_without_scratch_or_spills_at_eight_waves(tmp_path):
  src = os.path.join(_build.CSRC, "lr_lip_stable.hip")
  res = subprocess.run([_build._hipcc()] + _build._flags(src) +
                       ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o",
                        str(tmp_path / "lr_lip_stable.o")], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-2000:]
  blocks = re.split(r"remark: Function Name: ", res.stderr)[1:]
  names = [b.split()[0] for b in blocks]
  assert len([n for n in names if "stable_window_kernel" in n]) == 3      # 16, 4 and 1 pixels per store
  assert len([n for n in names if "stable_pose_kernel" in n]) == 1 and len(blocks) == 4
  for n in names:                                  # the names other tests count in lr_misc.hip stay theirs
    assert not any(s in n for s in ("lip_crop_collate_kernel", "lip_augment_collate_kernel", "collate_pad_aug_kernel"))
  for b in blocks:
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) + int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
    vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
    occupancy = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
    print(b.split()[0], "VGPRs", vgprs, "occupancy", occupancy, "scratch", scratch)
    assert scratch == 0 and spill == 0 and occupancy >= 8


# ---- the numpy restatement ------------------------------------------------------------------------------------------
SHAPES = [(96, 96, 32), (120, 160, 36), (120, 160, 30), (48, 64, 32)]


@pytest.mark.parametrize("H,W,S", SHAPES)
def test_restatement_agrees_with_the_box_oracle_where_both_rules_define_the_same_window(H, W, S):
  """Mouth points symmetric about their mean, level eyes, eye distance = the box's side / extent (level_case): the two
  rules cut the same window and differ in how the source coordinate is rounded only, which the bar covers."""
  from oracle import torch_oracle
  frames, lm, offsets, lens = SC.level_case(5, (H, W), S, margin=0.3, extent=2.0)
  want = torch_oracle.lip_crop(frames, lm, size=S, margin=0.3)
  real = want.size
  for fused in (False, True):
    got, _ = SC.stable_batch(frames, lm, offsets, lens, None, None, SC.T_MAX, S, extent=2.0, radius=0, fused=fused)
    flat = np.concatenate([got[b, :int(n)] for b, n in enumerate(lens)])
    worst, share = SC.within_bar(flat, want, real)
    print((H, W, S), "fused", fused, "max", worst, "share", share)
    assert worst <= 1 and share < 1e-3
    for b, n in enumerate(lens):
      assert not got[b, int(n):].any()
  assert want.any() and len(np.unique(want)) > 100


def test_pose_of_the_restatement():
  frames, lm, offsets, lens = SC.stable_case(5, (96, 96), 32, roll=20.0)
  raw = SC.smoothed_poses(lm, offsets, lens, 0)
  assert raw.dtype == np.float32 and raw.shape == (int(lens.sum()), 4)
  for n in range(len(lm)):                         # radius 0: the raw pose, and the raw pose is what it says
    assert raw[n].tobytes() == SC.raw_pose(lm[n]).tobytes()
    m = lm[n].astype(np.float64)
    want = [m[48:68, 0].mean(), m[48:68, 1].mean(), m[42:48, 0].mean() - m[36:42, 0].mean(),
            m[42:48, 1].mean() - m[36:42, 1].mean()]
    assert np.allclose(raw[n], want, rtol=1e-6, atol=1e-5)
  # the sums are exact inside the tests' range: no order of summation changes a bit
  rev = np.array([[np.float32(np.sum(lm[n, 48:68, c][::-1].astype(np.float64)) / 20.0) for c in (0, 1)]
                  for n in range(len(lm))])
  assert rev.tobytes() == raw[:, :2].tobytes()
  # a radius of at least the clip's length: every row gets its clip's mean
  for radius in (int(lens.max()), 32):
    sm = SC.smoothed_poses(lm, offsets, lens, radius)
    for b in range(5):
      lo, n = int(offsets[b]), int(lens[b])
      mean = np.array([SC._mean(raw[lo:lo + n, c]) for c in range(4)], np.float32)
      assert all(sm[lo + i].tobytes() == mean.tobytes() for i in range(n))
  # radius 2 smooths within the sample only: the first row of a sample never sees the previous sample's rows
  sm = SC.smoothed_poses(lm, offsets, lens, 2)
  for b in range(5):
    lo, n = int(offsets[b]), int(lens[b])
    assert sm[lo, 0] == SC._mean(raw[lo:lo + min(n, 3), 0])
  assert not np.array_equal(sm, raw)
  # the rolled eyes are rolled by about +-20 degrees, the coincident row has no eye vector
  ang = np.degrees(np.arctan2(raw[:, 3], raw[:, 2]))
  rows = len(lm)
  keep = np.arange(rows) != rows // 2
  assert (np.abs(np.abs(ang[keep]) - 20) < 3).all() and (ang[keep] > 0).any() and (ang[keep] < 0).any()
  assert raw[rows // 2, 2] == 0 and raw[rows // 2, 3] == 0


def test_restatement_flips_maps_masks_clamps_and_rotates():
  S = 32
  frames, lm, offsets, lens = SC.stable_case(5, (96, 96), S, roll=20.0)
  clip, tmap = SC.identity_records(lens)
  base, poses = SC.stable_batch(frames, lm, offsets, lens, clip, tmap, SC.T_MAX, S, radius=2)
  none, _ = SC.stable_batch(frames, lm, offsets, lens, None, None, SC.T_MAX, S, radius=2)
  assert np.array_equal(base, none)
  flipped = clip.copy()
  flipped[:, 3] = 1.0
  assert np.array_equal(SC.stable_batch(frames, lm, offsets, lens, flipped, tmap, SC.T_MAX, S, radius=2)[0],
                        base[..., ::-1])
  drawn = AugmentSpec(tjitter=0.3, tmask=(2, 3), seed=1).draw(0, range(5), lens)[1]
  drawn[int(offsets[4])] = int(lens[4])                                   # past the sample: clamped to its last frame
  got, _ = SC.stable_batch(frames, lm, offsets, lens, clip, drawn, SC.T_MAX, S, radius=2)
  for b in range(5):
    lo, n = int(offsets[b]), int(lens[b])
    for t in range(n):
      m = int(drawn[lo + t])
      assert np.array_equal(got[b, t], base[b, min(m, n - 1)] if m >= 0 else np.zeros_like(base[b, t]))
    assert not got[b, n:].any()
  # the roll reaches the pixels: the level case's windows are other windows
  level = SC.stable_batch(frames, SC.stable_case(5, (96, 96), S, roll=0.0)[1], offsets, lens, clip, tmap, SC.T_MAX, S,
                          radius=2)[0]
  assert not np.array_equal(level, base)
  # a quarter turn of the eye vector turns the crop: the window's x axis runs down the frame
  f = np.arange(3 * 40 * 40, dtype=np.int64).reshape(3, 40, 40) % 251
  up = SC.stable_crop(f.astype(np.uint8), [20, 20, 16, 0], (0, 0, 1, 0), size=16, extent=1.0)
  turned = SC.stable_crop(f.astype(np.uint8), [20, 20, 0, 16], (0, 0, 1, 0), size=16, extent=1.0)
  assert np.array_equal(up, f[:, 12:28, 12:28]) and np.array_equal(turned, np.rot90(up, k=1, axes=(1, 2)))
  # coincident eye points: the 2-pixel minimum side about the mouth mean
  cx, cy, ux, uy = SC.window([20, 20, 0, 0], (0, 0, 1, 0), 16, 1.25)
  assert (cx, cy, uy) == (20, 20, 0) and abs(ux * 16 - 2) < 1e-6


def test_fused_and_plain_arithmetic_of_the_restatement_stay_within_the_gpu_tests_bar():
  """The GPU test's bar (<= 1 LSB, < 1e-3 of the pixels) has to leave room for what the restatement itself does not pin
  down: whether an a + b * c is rounded once or twice.  Uniform noise is the hardest image for that."""
  spec = AugmentSpec(flip=0.5, shift=0.15, zoom=0.25, seed=8)
  for H, W, S in ((96, 96, 32), (120, 160, 36), (120, 160, 30), (96, 96, 96)):
    frames, lm, offsets, lens = SC.stable_case(5, (H, W), S, roll=20.0)
    clip, _ = spec.draw(0, range(5), lens)
    tmap = SC.identity_records(lens)[1]
    poses = SC.smoothed_poses(lm, offsets, lens, 2)
    a, _ = SC.stable_batch(frames, lm, offsets, lens, clip, tmap, SC.T_MAX, S, fused=False, poses=poses)
    b, _ = SC.stable_batch(frames, lm, offsets, lens, clip, tmap, SC.T_MAX, S, fused=True, poses=poses)
    worst, share = SC.within_bar(a, b, int(lens.sum()) * 3 * S * S)
    print((H, W, S), "max", worst, "share", share)
    assert worst <= 1 and share < 1e-3


def test_cpu_tensors_raise():
  from lipreading_amd import landmarks
  with pytest.raises(_C.LipReadingHipError):
    landmarks.lip_crop_stable(torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.zeros((2, 68, 3)))


# ---- driver and loader arguments ------------------------------------------------------------------------------------
def test_driver_crop_flags():
  from lipreading_amd import driver
  from lipreading_amd import data as D
  from lipreading_amd import dataset as DS
  assert (driver.DEFAULTS["crop"], driver.DEFAULTS["crop_extent"], driver.DEFAULTS["crop_smooth"]) == ("box", 1.25, 2)
  f = driver.parse_flags([])
  assert f["crop"] == "box"
  f = driver.parse_flags(["--frontend=conv3d", "--crop=stable"])
  assert (f["crop"], f["crop_extent"], f["crop_smooth"]) == ("stable", 1.25, 2)
  f = driver.parse_flags(["--frontend=conv3d", "--crop=stable", "--crop_extent=1.5", "--crop_smooth=0", "--prefetch=2"])
  assert (f["crop"], f["crop_extent"], f["crop_smooth"]) == ("stable", 1.5, 0)
  with pytest.raises(ValueError) as e:
    driver.parse_flags(["--crop=tight"])
  assert "box" in str(e.value) and "stable" in str(e.value)
  for bad in (["--crop=stable", "--crop_extent=0"], ["--crop=stable", "--crop_extent=-1"],
              ["--crop=stable", "--crop_extent=inf"], ["--crop=stable", "--crop_smooth=33"],
              ["--crop=stable", "--crop_smooth=-1"]):
    with pytest.raises(ValueError):
      driver.parse_flags(bad)
  with pytest.raises(ValueError) as e:             # run() checks before it touches data or the GPU
    driver.run(crop="round", data="no/such/dataset", root="/nonexistent")
  assert "box" in str(e.value) and "stable" in str(e.value)
  # the collate function and the loader name the same two choices
  with pytest.raises(ValueError):
    D.make_pixel_collate_fn("cuda", crop="round")
  with pytest.raises(ValueError):
    DS.make_loader([], 2, None, prefetch=2, device="cuda", pixels=True, crop="round")
  with pytest.raises(_C.LipReadingHipError):       # no CPU path, whatever the crop
    D.make_pixel_collate_fn("cpu", crop="stable")
