"""CPU: the numpy restatement of the landmark pose normalisation (tests/pose_cases.py) — what it recovers, what it is
invariant to, what it rejects — the generator's asserts, landmarks.PoseSpec, the driver's --lmk_pose flags,
fit_template's host canonicalisation, the argument checks of lr_lmk_pose_collate_f32 that need no device and the compiled
resources of lr_lmk_pose.hip.  The device stage is tests/test_gpu_pose.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from lipreading_amd import _build, _C
from tests import pose_cases as PC


def _motion(rng, scale=True, angle=None):
  R = PC.rot(rng.randn(3), rng.uniform(0.3, 2.5) if angle is None else angle)
  return R, (rng.uniform(0.5, 2.0) if scale else 1.0), rng.uniform(-50, 50, 3)


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts,rigid", PC.SHAPES)
def test_restatement_recovers_a_known_motion(npts, rigid):
  rng = np.random.RandomState(1)
  tmpl = PC.template(npts)
  for scale in (True, False):
    R, s, t = _motion(rng, scale)
    # the template moved away by (R, s, t): normalising must move it back, whatever the other points do
    x = (tmpl.astype(np.float64) - t) @ R / s              # x = R^T (q - t) / s   <=>   q = s R x + t
    lmk = x[None].astype(np.float32)
    Rg, sg, pb, status, qbar, _ = PC.poses(lmk, [0], [1], tmpl, rigid, 0, scale)
    xr = lmk[0].astype(np.float64)                         # (the fp32 rounding of the input is part of the input)
    want_t = qbar - sg[0] * (Rg[0] @ pb[0])
    got = sg[0] * (xr @ Rg[0].T) + want_t
    assert status[0] == PC.OK
    assert np.abs(Rg[0] - R).max() < 1e-6 and abs(sg[0] - s) < 1e-6 * s     # fp32 input: 1e-7 relative
    assert np.abs(got - tmpl).max() < 1e-4
    # and in float64 input, to 1e-9: the same solve on the unrounded points
    p = x[list(rigid)]
    q = tmpl.astype(np.float64)[list(rigid)]
    M = (q - q.mean(0)).T @ (p - p.mean(0))
    R64 = PC.rotation(M)
    s64 = np.trace(R64 @ M.T) / ((p - p.mean(0)) ** 2).sum()
    t64 = q.mean(0) - s64 * R64 @ p.mean(0)
    assert np.abs(R64 - R).max() < 1e-9 and abs(s64 - s) < 1e-9 and np.abs(t64 - t).max() < 1e-9
    assert abs(np.linalg.det(R64) - 1) < 1e-12


@pytest.mark.parametrize("npts,rigid", PC.SHAPES)
@pytest.mark.parametrize("radius", PC.RADII)
def test_restatement_is_invariant_under_one_motion_per_clip(npts, rigid, radius):
  rng = np.random.RandomState(2)
  lmk, offsets, lens = PC.make_clips(npts, seed=5)
  tmpl = PC.template(npts)
  x = lmk.astype(np.float64)
  for scale in (True, False):
    moved = x.copy()
    for b in range(len(lens)):
      R, s, t = _motion(rng, scale)
      lo, n = int(offsets[b]), int(lens[b])
      moved[lo:lo + n] = s * (x[lo:lo + n] @ R.T) + t
    # float64 in, float64 out: pose_batch widens fp32, so the arithmetic is restated on the float64 points here
    def run(points):
      idx = list(rigid)
      q = tmpl.astype(np.float64)[idx]
      out = np.zeros_like(points)
      for n_, win in PC.windows(offsets, lens, radius).items():
        Mw, vw = np.zeros((3, 3)), 0.0
        for m in win:
          p = points[m, idx]
          Mw += (q - q.mean(0)).T @ (p - p.mean(0))
          vw += ((p - p.mean(0)) ** 2).sum()
        Rn = PC.rotation(Mw)
        sn = np.trace(Rn @ Mw.T) / vw if scale else 1.0
        out[n_] = sn * ((points[n_] - points[n_, idx].mean(0)) @ Rn.T) + q.mean(0)
      return out
    a, b_ = run(x), run(moved)
    err = np.abs(a - b_).max() / np.abs(a).max()
    print(npts, radius, scale, "relative change under a motion per clip: %.3g" % err)
    assert err < 1e-11
    # and the shipped restatement (fp32 in) says the same as this one on the unmoved points
    want = PC.pose_batch(lmk, offsets, lens, None, int(lens.max()), tmpl, rigid, radius, scale)[3]
    for b in range(len(lens)):
      lo, n = int(offsets[b]), int(lens[b])
      assert np.abs(want[b, :n] - a[lo:lo + n]).max() < 1e-9


def test_generator_asserts_hold_for_every_case():
  """case() asserts the eigenvalue gap and the distance from rounding ties; here they are looked at once more."""
  gaps, ties, n = [], [], 0
  for c in PC.all_cases():
    gaps += [np.nanmin(c["gaps"]), np.nanmax(c["gaps"])]
    ties.append(PC.tie_distance(c["out64"]))
    assert (c["status"] == PC.OK).all() and np.isfinite(c["out"]).all()
    n += 1
  print("cases %d, Horn gap %.3f .. %.3f, nearest tie %.3g of an fp32 step" % (n, min(gaps), max(gaps), min(ties)))
  assert n == 48 and min(gaps) >= PC.MIN_GAP and min(ties) >= PC.TIE_MARGIN
  # the helpers themselves: a value on a tie, and a matrix with two equal top eigenvalues
  one = np.float32(1.0)
  assert PC.tie_distance([0.5 * (float(one) + float(np.nextafter(one, np.float32(2))))]) == 0.0
  assert PC.tie_distance([1.0]) == 0.5
  assert PC.horn_gap(np.diag([1.0, 0.0, 0.0])) < 1e-12       # collinear: a whole circle of maximisers
  assert PC.ulp(np.float32(0.0)) == 2.0 ** -33 and PC.ulp(np.float32(100.0)) == 2.0 ** -17


def test_mirrored_input_still_yields_a_proper_rotation():
  for npts, rigid in PC.SHAPES:
    c = PC.case(npts, rigid, 2, True, 9, mirrored=True)
    R = c["pose"][:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-5)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5
    wrong = PC.poses(c["lmk"], c["offsets"], c["lens"], c["tmpl"], rigid, 2, True, variant="no_det")[0]
    if npts == 68:                                             # (three rigid points lie in a plane: U V^T may be proper)
      assert np.allclose(np.linalg.det(wrong), -1.0)


def test_window_never_crosses_samples_and_translation_is_the_rows_own():
  lmk, offsets, lens = PC.make_clips(68)
  tmpl = PC.template(68)
  for radius in (2, 32):
    full = PC.pose_batch(lmk, offsets, lens, None, 9, tmpl, PC.RIGID_68, radius, True)
    for b in range(3):                                         # a batch is its samples, one by one
      lo, n = int(offsets[b]), int(lens[b])
      alone = PC.pose_batch(lmk[lo:lo + n], [0], [n], None, 9, tmpl, PC.RIGID_68, radius, True)
      assert alone[0][0].tobytes() == full[0][b].tobytes() and alone[1].tobytes() == full[1][lo:lo + n].tobytes()
    pbar = PC.row_stats(lmk, tmpl, PC.RIGID_68)[0]
    assert full[1][:, 10:].tobytes() == pbar.astype(np.float32).tobytes()
  # radius >= len: every row of a sample has the sample's rotation and scale
  pose = PC.pose_batch(lmk, offsets, lens, None, 9, tmpl, PC.RIGID_68, 32, True)[1]
  for b in range(3):
    lo, n = int(offsets[b]), int(lens[b])
    assert (pose[lo:lo + n, :10] == pose[lo, :10]).all()
  assert not (pose[int(offsets[1]), :10] == pose[int(offsets[2]), :10]).all()


def test_bad_and_degenerate_rows_follow_the_specification():
  lmk, offsets, lens = PC.make_clips(68)
  lmk = lmk.copy()
  tmpl = PC.template(68)
  lo = int(offsets[2])
  lmk[lo + 3, 50, 1] = np.nan                                  # not a rigid point: the row is BAD all the same
  lmk[lo + 6, 27, 0] = np.inf
  # the one-row sample: coincident rigid points (at a point whose nine-fold sum is exact, so the spread is exactly 0)
  lmk[int(offsets[0]), list(PC.RIGID_68)] = [64.0, 32.0, 8.0]
  tmap = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
  tmap[lo + 1] = 3                                             # a good frame that shows a BAD row
  for radius in (0, 2):
    out, pose, status, _, _ = PC.pose_batch(lmk, offsets, lens, tmap, 12, tmpl, PC.RIGID_68, radius, True)
    assert list(np.flatnonzero(status == PC.BAD_ROW)) == [lo + 3, lo + 6]
    assert list(np.flatnonzero(status == PC.DEGENERATE)) == [0]
    assert np.isfinite(out).all() and np.isfinite(pose).all()
    assert not out[2, 3].any() and not out[2, 6].any() and not out[2, 1].any() and out[2, 2].any()
    assert pose[lo + 3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0]
    assert pose[0, :10].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1]
    qbar = PC.row_stats(lmk, tmpl, PC.RIGID_68)[4]
    x0 = lmk[0].astype(np.float64)
    assert np.array_equal(out[0, 0], (x0 - x0[list(PC.RIGID_68)].mean(0) + qbar).astype(np.float32))
    assert not out[0, 1:].any() and not out[:, 9:].any()
    if radius:                                                 # the BAD rows are left out of their neighbours' windows
      clean = np.delete(lmk[lo:lo + 9], [3, 6], axis=0)
      alone = PC.pose_batch(clean, [0], [7], None, 7, tmpl, PC.RIGID_68, 32, True)[1]
      whole = PC.pose_batch(lmk, offsets, lens, None, 9, tmpl, PC.RIGID_68, 32, True)[1]
      assert np.array_equal(whole[lo, :10], alone[0, :10])


@pytest.mark.parametrize("npts,rigid", PC.SHAPES)
@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("t_max", PC.T_MAXES)
def test_restatement_rejects_three_wrong_variants(npts, rigid, scale, t_max):
  """With the parity tolerance of the GPU test (one ulp), at every case shape where the variant can differ: a window
  needs radius > 0, the determinant fix needs the mirrored input."""
  for radius in PC.RADII:
    c = PC.case(npts, rigid, radius, scale, t_max)
    args = (c["lmk"], c["offsets"], c["lens"], None, t_max, c["tmpl"], rigid, radius, scale)
    for variant in ("cross", "smooth_centroid"):
      wrong = PC.pose_batch(*args, variant=variant)[0]
      worst = PC.worst_ulps(wrong, c["out"])
      if radius == 0:
        assert worst == 0                                      # no window: nothing to get wrong
      else:
        assert worst > 100, (variant, radius, worst)
    m = PC.case(npts, rigid, radius, scale, t_max, mirrored=True)
    wrong = PC.pose_batch(m["lmk"], m["offsets"], m["lens"], None, t_max, m["tmpl"], rigid, radius, scale,
                          variant="no_det")
    if npts == 68:
      assert PC.worst_ulps(wrong[0], m["out"]) > 100
    else:     # three rigid points: the reflection through their plane fits as well, so SVD's U V^T is proper or not by
      pass    # the sign it happens to give the null vector; the variant is checked where it is defined


# ---- PoseSpec, flags, canonicalisation -------------------------------------------------------------------------------
def test_pose_spec_validates_on_the_host():
  from lipreading_amd.landmarks import RIGID_68, PoseSpec
  assert RIGID_68 == (27, 28, 29, 30, 33, 36, 39, 42, 45) == PC.RIGID_68
  t = PC.template(68)
  s = PoseSpec(t)
  assert (s.npts, s.rigid, s.radius, s.scale, s.flags) == (68, RIGID_68, 0, True, _C.LR_POSE_SCALE)
  assert s.template.dtype == np.float32 and np.array_equal(s.template, t) and not s.template.flags.writeable
  s = PoseSpec(torch.from_numpy(PC.template(4)).double(), rigid=[3, 0, 1], radius=32, scale=False)
  assert (s.npts, s.rigid, s.radius, s.flags) == (4, (3, 0, 1), 32, 0)
  assert list(s._rigid_c) == [3, 0, 1]
  for kwargs, word in ((dict(template=t[:, :2]), "(68, 2)"), (dict(template=np.zeros((257, 3))), "(257, 3)"),
                       (dict(template=t, rigid=(0, 1)), "got 2"), (dict(template=t, rigid=range(65)), "got 65"),
                       (dict(template=t, rigid=(0, 1, 68)), "68"), (dict(template=t, rigid=(0, 1, -1)), "-1"),
                       (dict(template=t, rigid=(5, 9, 5)), "5 is repeated"), (dict(template=t, radius=33), "33"),
                       (dict(template=t, radius=-1), "-1"), (dict(template=t, radius=1.5), "1.5"),
                       (dict(template=t, rigid=None), "None")):
    with pytest.raises(ValueError) as e:
      PoseSpec(**kwargs)
    assert word in str(e.value), (kwargs.keys(), str(e.value))
  nan = t.copy()
  nan[7, 1] = np.nan
  with pytest.raises(ValueError) as e:
    PoseSpec(nan)
  assert "point 7" in str(e.value)


def test_cpu_tensors_raise():
  from lipreading_amd import landmarks
  spec = landmarks.PoseSpec(PC.template(68))
  with pytest.raises(_C.LipReadingHipError):
    landmarks.normalise_pose(torch.zeros((2, 68, 3)), spec)
  with pytest.raises(_C.LipReadingHipError):
    landmarks.fit_template([np.zeros((2, 68, 3))], device="cpu")
  from lipreading_amd.loader import PrefetchLoader
  with pytest.raises(ValueError) as e:
    PrefetchLoader([], 2, "cuda", pixels=True, pose=spec)
  assert "pixels=True" in str(e.value)


def test_driver_pose_flags():
  from lipreading_amd import driver
  d = driver.DEFAULTS
  assert (d["lmk_pose"], d["lmk_pose_smooth"], d["lmk_pose_template"]) == ("none", 0, "")
  assert driver.parse_flags([])["lmk_pose"] == "none"
  f = driver.parse_flags(["--lmk_pose=similarity", "--lmk_pose_smooth=3", "--lmk_pose_template=face.npy", "--prefetch=2"])
  assert (f["lmk_pose"], f["lmk_pose_smooth"], f["lmk_pose_template"]) == ("similarity", 3, "face.npy")
  assert driver.parse_flags(["--lmk_pose=rigid", "--lmk_pose_smooth=32"])["lmk_pose_smooth"] == 32
  with pytest.raises(ValueError) as e:
    driver.parse_flags(["--lmk_pose=affine"])
  assert all(w in str(e.value) for w in ("none", "rigid", "similarity", "affine"))
  for bad in ("33", "-1"):
    with pytest.raises(ValueError) as e:
      driver.parse_flags(["--lmk_pose=rigid", "--lmk_pose_smooth=" + bad])
    assert bad in str(e.value)
  assert driver.parse_flags(["--lmk_pose_smooth=99"])["lmk_pose"] == "none"     # unused without --lmk_pose
  with pytest.raises(ValueError) as e:
    driver.parse_flags(["--lmk_pose=rigid", "--frontend=conv3d"])
  assert "--lmk_pose" in str(e.value) and "--frontend=conv3d" in str(e.value)
  with pytest.raises(ValueError) as e:                         # run() checks before it touches data or the GPU
    driver.run(lmk_pose="affine", data="no/such/dataset", root="/nonexistent")
  assert "similarity" in str(e.value)
  assert driver.lmk_pose_spec(dict(lmk_pose="none"), None, None) is None


def test_template_file_of_the_wrong_shape_is_rejected(tmp_path):
  from lipreading_amd import driver
  path = str(tmp_path / "face.npy")
  np.save(path, np.zeros((67, 3), np.float32))
  with pytest.raises(ValueError) as e:
    driver.lmk_pose_spec(dict(lmk_pose="rigid", lmk_pose_template=path), None, None)
  assert "(67, 3)" in str(e.value)
  np.save(path, PC.template(68))
  spec = driver.lmk_pose_spec(dict(lmk_pose="rigid", lmk_pose_smooth=4, lmk_pose_template=path), None, None)
  assert (spec.radius, spec.scale) == (4, False) and np.array_equal(spec.template, PC.template(68))


def test_canonical_orientation_on_hand_made_anchors():
  from lipreading_amd.landmarks import canonical_orientation
  p = np.zeros((68, 3))
  p[36:42] = [-3, 2, 0]
  p[42:48] = [3, 2, 0]
  p[48:68] = [0, -4, 0]
  p[30] = [0, 0, 5]
  same = canonical_orientation(p)                              # x = +x, y = -y (eyes to mouth), z = x × y = -z
  assert np.allclose(same[:, 0], p[:, 0]) and np.allclose(same[:, 1], -p[:, 1]) and np.allclose(same[:, 2], -p[:, 2])
  rng = np.random.RandomState(4)
  base = rng.randn(68, 3) * 10
  base[42:48] += [40, 0, 0]
  base[48:68] += [20, 50, 5]
  want = canonical_orientation(base)
  for _ in range(5):                                           # whatever way the head is turned, the same face comes out
    R, _, _ = _motion(rng, scale=False)
    got = canonical_orientation(base @ R.T)
    assert np.abs(got - want).max() < 1e-11
  eye = want[42:48].mean(0) - want[36:42].mean(0)
  mouth = want[48:68].mean(0) - 0.5 * (want[42:48].mean(0) + want[36:42].mean(0))
  assert eye[0] > 0 and abs(eye[1]) < 1e-12 and abs(eye[2]) < 1e-12 and mouth[1] > 0 and abs(mouth[2]) < 1e-12
  assert np.allclose(np.linalg.norm(want, axis=1), np.linalg.norm(base, axis=1))     # a rotation about the origin
  line = np.zeros((68, 3))
  line[36:42], line[42:48], line[48:68] = [-1, 0, 0], [1, 0, 0], [5, 0, 0]
  with pytest.raises(ValueError) as e:
    canonical_orientation(line)
  assert "collinear" in str(e.value)
  with pytest.raises(ValueError):
    canonical_orientation(np.zeros((68, 3)))
  with pytest.raises(ValueError):
    canonical_orientation(np.zeros((4, 3)))


# ---- header, bindings and the argument checks ------------------------------------------------------------------------
def test_entry_points_are_bound_from_the_header():
  restype, argtypes = _C.SIGNATURES["lr_lmk_pose_collate_f32"]
  assert restype is _C.c_int and len(argtypes) == 19
  assert argtypes[:6] == [_C.P] * 6 and argtypes[6] is _C.c_int and argtypes[7:11] == [_C.P] * 4
  assert argtypes[11] is ctypes.c_size_t and argtypes[13] is ctypes.c_int64 and argtypes[18] is _C.P
  assert _C.SIGNATURES["lr_lmk_pose_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, _C.c_int, _C.c_int])
  assert (_C.LR_POSE_MAX_RADIUS, _C.LR_POSE_MAX_RIGID, _C.LR_POSE_MAX_POINTS, _C.LR_POSE_SCALE) == (32, 64, 256, 1)
  assert (_C.LR_POSE_OK, _C.LR_POSE_DEGENERATE, _C.LR_POSE_BAD_ROW) == (0, 1, 2)


GOOD = dict(n_rigid=9, nbytes=1 << 20, B=1, rows=1, t_max=1, npts=68, radius=2, flags=1)


def _call(L, ptrs, rigid=PC.RIGID_68, **change):
  a = dict(GOOD)
  a.update(change)
  lmk, offsets, lens, tmap, tmpl, out, pose, status, work = ptrs
  host = (ctypes.c_int32 * max(len(rigid), 1))(*rigid)
  rigid_ptr = ctypes.addressof(host) if change.get("rigid_null") is None else None
  return L.lr_lmk_pose_collate_f32(lmk, offsets, lens, tmap, tmpl, rigid_ptr, a["n_rigid"], out, pose, status, work,
                                   a["nbytes"], a["B"], a["rows"], a["t_max"], a["npts"], a["radius"], a["flags"], None)


def test_bad_arguments_are_rejected_without_a_device():
  _build.build_library()
  L = _C.lib()
  one = 4096                       # any non-NULL, 16-byte aligned value: the checks return before a pointer is used
  #        lmk offsets lens tmap tmpl out pose status workspace
  good = [one] * 9
  for i in (0, 1, 2, 4, 5, 7, 8):  # each required pointer alone (tmap and pose are optional)
    args = list(good)
    args[i] = None
    assert _call(L, args) == _C.LR_ERR_INVALID_ARG, i
  assert _call(L, good, rigid_null=True) == _C.LR_ERR_INVALID_ARG
  for change in (dict(n_rigid=2), dict(n_rigid=65), dict(npts=0), dict(npts=257), dict(radius=-1), dict(radius=33),
                 dict(flags=2), dict(flags=3), dict(flags=-1)):
    assert _call(L, good, **change) == _C.LR_ERR_UNSUPPORTED, change
  for rigid in ((27, 28, 29, 30, 33, 36, 39, 42, 68), (27, 28, 29, 30, 33, 36, 39, 42, -1),
                (27, 28, 29, 30, 33, 36, 39, 42, 27)):
    assert _call(L, good, rigid=rigid) == _C.LR_ERR_INVALID_ARG, rigid
  assert _call(L, good, rigid=(0, 1, 2, 3), n_rigid=4, npts=3) == _C.LR_ERR_INVALID_ARG    # more rigid points than points
  for change in (dict(B=0), dict(rows=0), dict(t_max=0), dict(B=1 << 20, t_max=1 << 12), dict(rows=1 << 31)):
    assert _call(L, good, **change) == _C.LR_ERR_INVALID_ARG, change
  misaligned = list(good)
  misaligned[8] = one + 8
  assert _call(L, misaligned) == _C.LR_ERR_INVALID_ARG
  assert _call(L, good, nbytes=16) == _C.LR_ERR_WORKSPACE
  need = L.lr_lmk_pose_workspace_bytes(1, 9, 2)
  assert _call(L, good, nbytes=need - 1) == _C.LR_ERR_WORKSPACE
  # the workspace: 0 for what the entry rejects, otherwise 14 float64 words per row and the template's centroid
  for bad in ((0, 9, 2), (-5, 9, 2), (10, 2, 2), (10, 65, 2), (10, 9, -1), (10, 9, 33), (1 << 31, 9, 0)):
    assert L.lr_lmk_pose_workspace_bytes(*bad) == 0, bad
  for rows in (1, 7, 2400):
    for radius in (0, 2, 32):
      assert L.lr_lmk_pose_workspace_bytes(rows, 9, radius) >= (rows * 14 + 3) * 8


# ---- compiled resources ----------------------------------------------------------------------------------------------
def test_pose_kernels_compile_without_scratch_or_spills(tmp_path):
  src = os.path.join(_build.CSRC, "lr_lmk_pose.hip")
  res = subprocess.run([_build._hipcc()] + _build._flags(src) +
                       ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o",
                        str(tmp_path / "lr_lmk_pose.o")], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-2000:]
  blocks = re.split(r"remark: Function Name: ", res.stderr)[1:]
  names = [b.split()[0] for b in blocks]
  assert len(blocks) == 2 and any("pose_stats_kernel" in n for n in names) and any("pose_apply_kernel" in n for n in names)
  for b in blocks:
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) + int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
    vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
    occupancy = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    print(b.split()[0], "VGPRs", vgprs, "occupancy", occupancy, "scratch", scratch, "LDS", lds)
    # the apply kernel is one wave per (sample, frame): B = 32, T = 75 is 2400 waves on 256 CUs x 4 SIMDs, 2.4 a SIMD,
    # so three resident waves a SIMD hold the whole grid at once; the float64 Jacobi state (two 4x4 matrices) is
    # what fills the registers
    assert scratch == 0 and spill == 0 and lds == 0 and occupancy >= 3
