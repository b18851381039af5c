"""GPU: lr_lmk_pose_collate_f32, landmarks.pose_collate / normalise_pose / fit_template, make_collate_fn(pose=),
PrefetchLoader(pose=) and the driver's --lmk_pose.  The yardstick is the float64 numpy restatement (tests/pose_cases.py:
SVD, not the kernel's method) or existing code (lr_collate_pad_f32, today's loaders), never the new code.  Everything is
float64 with one rounding, so `out` must lie within ONE fp32 ulp of the restatement's value (the ulp taken at
max(|want|, 2^-10)), the rotation's entries within 2^-23, scale and centroid within one ulp; what the kernel promises
about itself (zeros, determinism, batch = samples) is exact.  The host side is tests/test_pose_cpu.py.

Measured on the MI355X (the 48 parity cases, mirrored ones included, the batch-semantics cases and the exact motions):
out, the rotation, the scale and the centroid all came out bit-equal to the restatement's fp32 values, 0 ulp."""
import numpy as np
import pytest
import torch

from tests import pose_cases as PC

pytestmark = pytest.mark.gpu

GUARD = 1024                                       # elements either side of out, pose and status; bytes of the workspace


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _guarded(dev, n, dtype, fill):
  raw = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
  return raw, raw[GUARD:GUARD + n]


def _intact(raw, n, fill):
  edge = torch.cat([raw[:GUARD], raw[GUARD + n:]])
  return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


def pose_call(dev, lmk, offsets, lens, t_max, tmpl, rigid, radius, scale, tmap=None, want_pose=True):
  """One call of the C entry on numpy inputs -> (out [B][t_max][npts][3], pose [rows][13], status [rows]) as numpy.
  out and pose are pre-filled with NaN and status with -7, so an unwritten element shows; all three and the workspace
  lie between guards, which every call checks.  The landmark buffer carries one spare row of NaN behind the last sample."""
  from lipreading_amd import _C
  import ctypes
  L = _C.lib()
  lmk = np.ascontiguousarray(lmk, dtype=np.float32)
  rows, npts = lmk.shape[0], lmk.shape[1]
  B = len(lens)
  lmk_d = torch.from_numpy(np.concatenate([lmk, np.full_like(lmk[:1], np.nan)])).to(dev)
  off_d = torch.from_numpy(np.array(offsets, dtype=np.int64)).to(dev)
  lens_d = torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(dev)
  tmap_d = None if tmap is None else torch.from_numpy(np.ascontiguousarray(tmap, dtype=np.int32)).to(dev)
  tmpl_d = torch.from_numpy(np.array(tmpl, dtype=np.float32)).to(dev)
  host = (ctypes.c_int32 * len(rigid))(*rigid)
  need = L.lr_lmk_pose_workspace_bytes(rows, len(rigid), radius)
  assert need >= (rows * 14 + 3) * 8
  n_out = B * t_max * npts * 3
  raw_o, out = _guarded(dev, n_out, torch.float32, float("nan"))
  raw_p, pose = _guarded(dev, rows * 13, torch.float32, float("nan"))
  raw_s, status = _guarded(dev, rows, torch.int32, -7)
  raw_w, work = _guarded(dev, need, torch.uint8, 0xFF)
  assert work.data_ptr() % 16 == 0
  _C.check(L.lr_lmk_pose_collate_f32(lmk_d.data_ptr(), off_d.data_ptr(), lens_d.data_ptr(), _C.ptr(tmap_d),
                                     tmpl_d.data_ptr(), ctypes.addressof(host), len(rigid), out.data_ptr(),
                                     pose.data_ptr() if want_pose else None, status.data_ptr(), work.data_ptr(), need, B,
                                     rows, t_max, npts, radius, _C.LR_POSE_SCALE if scale else 0, _C.stream_handle()),
           "lr_lmk_pose_collate_f32")
  torch.cuda.synchronize()
  assert _intact(raw_o, n_out, float("nan")), "wrote outside out"
  assert _intact(raw_p, rows * 13, float("nan")), "wrote outside pose"
  assert _intact(raw_s, rows, -7), "wrote outside status"
  assert _intact(raw_w, need, 0xFF), "wrote outside the workspace"
  out_h = out.view(B, t_max, npts, 3).cpu().numpy()
  assert not np.isnan(out_h).any(), "%d elements of out were not written" % int(np.isnan(out_h).sum())
  status_h = status.cpu().numpy()
  assert (status_h != -7).all(), "status of %d rows was not written" % int((status_h == -7).sum())
  pose_h = pose.view(rows, 13).cpu().numpy()
  assert np.isnan(pose_h).all() if not want_pose else not np.isnan(pose_h).any()
  return out_h, pose_h, status_h


def check_against(got, want, what):
  """(out, pose, status) of the device against the restatement's, at the tolerances of the module docstring."""
  out, pose, status = got
  w_out, w_pose, w_status = want[:3]
  assert np.array_equal(status, w_status), (what, status, w_status)
  e_out = PC.worst_ulps(out, w_out)
  e_rot = float(np.abs(pose[:, :9].astype(np.float64) - w_pose[:, :9]).max())
  e_rest = PC.worst_ulps(pose[:, 9:], w_pose[:, 9:])
  print("%s: out %.3g ulp, R %.3g, s and centroid %.3g ulp" % (what, e_out, e_rot, e_rest))
  assert e_out <= 1.0 and e_rot <= 2.0 ** -23 and e_rest <= 1.0, (what, e_out, e_rot, e_rest)
  return e_out, e_rot, e_rest


# ---- parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_max", PC.T_MAXES)
@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("radius", PC.RADII)
@pytest.mark.parametrize("npts,rigid", PC.SHAPES)
def test_parity_with_the_restatement(dev, npts, rigid, radius, scale, t_max):
  for mirrored in (False, True):
    c = PC.case(npts, rigid, radius, scale, t_max, mirrored=mirrored)
    got = pose_call(dev, c["lmk"], c["offsets"], c["lens"], t_max, c["tmpl"], rigid, radius, scale)
    check_against(got, (c["out"], c["pose"], c["status"]),
                  "npts %d radius %d scale %d t_max %d mirrored %d" % (npts, radius, scale, t_max, mirrored))
    for b, n in enumerate(c["lens"]):
      assert not got[0][b, int(n):].any()                      # padding frames are zeros
    R = got[1][:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-6)       # proper, the mirrored input included
    # without pose the same out
    again = pose_call(dev, c["lmk"], c["offsets"], c["lens"], t_max, c["tmpl"], rigid, radius, scale, want_pose=False)
    assert again[0].tobytes() == got[0].tobytes() and np.array_equal(again[2], got[2])


# ---- batch semantics ------------------------------------------------------------------------------------------------
def _semantics_case():
  lmk, offsets, lens = PC.make_clips(68, seed=2)
  lmk = PC.nudge_off_ties(lmk, PC.RIGID_68)
  lo1, lo2 = int(offsets[1]), int(offsets[2])
  lmk[lo2 + 3, 50, 1] = np.nan                                 # BAD by a point that is not rigid
  lmk[lo2 + 6, 27, 0] = np.inf                                 # BAD by a rigid point
  lmk[0, list(PC.RIGID_68)] = [64.0, 32.0, 8.0]                # the one-row sample: its rigid points coincide
  tmap = np.concatenate([np.arange(n) for n in lens]).astype(np.int32)
  tmap[lo1:lo1 + 4] = [2, 2, -1, 9]                            # repeats, a masked frame, a value past the sample
  tmap[lo2:lo2 + 9] = [0, 3, 0, 40, -5, 8, 8, 1 << 30, 6]      # a BAD source row twice; rows 2, 4, 5, 7 unreferenced
  return lmk, offsets, lens, tmap


@pytest.mark.parametrize("radius", PC.RADII)
@pytest.mark.parametrize("scale", [True, False])
def test_batch_semantics(dev, radius, scale):
  lmk, offsets, lens, tmap = _semantics_case()
  tmpl = PC.template(68)
  for t_max in PC.T_MAXES:
    plain_want = PC.pose_batch(lmk, offsets, lens, None, t_max, tmpl, PC.RIGID_68, radius, scale)
    plain = pose_call(dev, lmk, offsets, lens, t_max, tmpl, PC.RIGID_68, radius, scale)
    check_against(plain, plain_want, "plain radius %d scale %d t_max %d" % (radius, scale, t_max))
    want = PC.pose_batch(lmk, offsets, lens, tmap, t_max, tmpl, PC.RIGID_68, radius, scale)
    got = pose_call(dev, lmk, offsets, lens, t_max, tmpl, PC.RIGID_68, radius, scale, tmap=tmap)
    check_against(got, want, "mapped radius %d scale %d t_max %d" % (radius, scale, t_max))
    lo1, lo2 = int(offsets[1]), int(offsets[2])
    # status and pose belong to the rows, not to the map: the unreferenced rows have theirs
    assert got[1].tobytes() == plain[1].tobytes() and np.array_equal(got[2], plain[2])
    assert list(np.flatnonzero(got[2] == PC.BAD_ROW)) == [lo2 + 3, lo2 + 6]
    assert list(np.flatnonzero(got[2] == PC.DEGENERATE)) == [0] and got[1][0, :10].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1]
    assert got[1][lo2 + 3].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0]
    # a mapped frame is exactly the plain call's frame of its source row; masked frames and BAD rows are zeros
    o, p = got[0], plain[0]
    assert o[1, 0].tobytes() == p[1, 2].tobytes() == o[1, 1].tobytes() and not o[1, 2].any()
    assert o[1, 3].tobytes() == p[1, 3].tobytes()              # 9 is past the sample of four: its last row
    assert o[2, 0].tobytes() == p[2, 0].tobytes() == o[2, 2].tobytes() and not o[2, 1].any() and not o[2, 4].any()
    assert o[2, 3].tobytes() == p[2, 8].tobytes() == o[2, 7].tobytes() == o[2, 5].tobytes() and not o[2, 8].any()
    assert not p[2, 3].any() and not p[2, 6].any() and p[2, 2].any() and not o[:, 9:].any() and not o[0, 1:].any()
    assert np.isfinite(o).all() and np.isfinite(got[1]).all()


def test_collinear_rigid_points_give_finite_output(dev):
  lmk, offsets, lens = PC.make_clips(68, seed=3)
  line = np.linspace(0, 1, 9)[:, None] * np.array([30.0, 10.0, 5.0]) + [90, 100, 3]
  lmk[:, list(PC.RIGID_68)] = line.astype(np.float32)          # every maximiser is acceptable, none may be NaN
  for radius in (0, 2):
    out, pose, status = pose_call(dev, lmk, offsets, lens, 9, PC.template(68), PC.RIGID_68, radius, True)
    assert np.isfinite(out).all() and np.isfinite(pose).all() and (status == PC.OK).all()
    R = pose[:, :9].reshape(-1, 3, 3).astype(np.float64)
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-5) and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5


# ---- determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts,rigid", PC.SHAPES)
def test_two_launches_and_per_sample_calls_give_the_same_bits(dev, npts, rigid):
  if npts == 68:
    lmk, offsets, lens, tmap = _semantics_case()
  else:
    lmk, offsets, lens = PC.make_clips(4, seed=2)
    tmap = np.concatenate([np.arange(n)[::-1] for n in lens]).astype(np.int32)
  tmpl = PC.template(npts)
  for radius in (0, 2):
    for tm in (None, tmap):
      a = pose_call(dev, lmk, offsets, lens, 12, tmpl, rigid, radius, True, tmap=tm)
      b = pose_call(dev, lmk, offsets, lens, 12, tmpl, rigid, radius, True, tmap=tm)
      assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
      for s in range(len(lens)):
        lo, n = int(offsets[s]), int(lens[s])
        one = pose_call(dev, lmk[lo:lo + n], [0], [n], 12, tmpl, rigid, radius, True,
                        tmap=None if tm is None else tm[lo:lo + n])
        assert one[0][0].tobytes() == a[0][s].tobytes(), (radius, s)
        assert one[1].tobytes() == a[1][lo:lo + n].tobytes() and np.array_equal(one[2], a[2][lo:lo + n])


# ---- exact-in-fp32 motions --------------------------------------------------------------------------------------------
PERMS = [np.array(p, dtype=np.float64) for p in (
    [[0, 1, 0], [0, 0, 1], [1, 0, 0]],                         # x y z -> y z x
    [[0, -1, 0], [1, 0, 0], [0, 0, 1]],                        # a quarter turn about z
    [[1, 0, 0], [0, 0, -1], [0, 1, 0]],                        # a quarter turn about x
    [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],                       # a half turn about z
    [[0, 0, -1], [0, -1, 0], [-1, 0, 0]])]                     # a signed permutation with two swaps: det = +1


@pytest.mark.parametrize("npts,rigid", PC.SHAPES)
@pytest.mark.parametrize("scale", [True, False])
def test_exact_motions_leave_the_output_unchanged(dev, npts, rigid, scale):
  clip = PC.exact_clip(npts)
  n = len(clip)
  tmpl = PC.template(npts)
  assert np.abs(clip).max() < 128 and np.array_equal(clip * 64, np.round(clip * 64))
  for radius in (0, 2):
    base = pose_call(dev, clip, [0], [n], n, tmpl, rigid, radius, scale)
    assert (base[2] == PC.OK).all()
    want = PC.pose_batch(clip, [0], [n], None, n, tmpl, rigid, radius, scale)
    check_against(base, want, "exact clip npts %d radius %d scale %d" % (npts, radius, scale))
    for k, P in enumerate(PERMS):
      assert abs(np.linalg.det(P) - 1) < 1e-12
      for s in ((0.5, 2.0, 1.0) if scale else (1.0,)):
        t = np.array([[17, -40, 64], [-3, 5, -8], [0, 0, 0]][k % 3], dtype=np.float64)
        moved64 = s * (clip.astype(np.float64) @ P.T) + t
        moved = moved64.astype(np.float32)
        assert np.array_equal(moved.astype(np.float64), moved64)   # the motion is exact in fp32
        got = pose_call(dev, moved, [0], [n], n, tmpl, rigid, radius, scale)
        worst = PC.worst_ulps(got[0], base[0])
        rot = np.abs(got[1][:, :9].reshape(-1, 3, 3).astype(np.float64) @ P
                     - base[1][:, :9].reshape(-1, 3, 3)).max()
        print("npts %d radius %d scale %d perm %d s %g: out %.3g ulp, R P against R %.3g" % (npts, radius, scale, k, s,
                                                                                              worst, rot))
        # (R P and R: entries of magnitude <= 1, each rounded to fp32 once, 2^-24 apiece, and P only permutes them)
        assert worst <= 1.0 and rot <= 2.0 ** -22 and (got[2] == PC.OK).all()
        if scale:
          assert PC.worst_ulps(got[1][:, 9] * np.float32(s), base[1][:, 9]) <= 1.0


# ---- Python, up to the loaders ----------------------------------------------------------------------------------------
def _caption(rng, n):
  return np.array([1] + list(rng.randint(4, 64, n)) + [2])


def _landmark_dataset(n, seed):
  rng = np.random.RandomState(seed)
  out = []
  for t in np.sort(rng.randint(6, 20, n)):
    clip = PC.make_clips(68, lens=(int(t),), seed=int(rng.randint(1 << 20)))[0]
    out.append((clip.astype(np.float64), _caption(rng, rng.randint(2, 5))))
  return out


def _ragged(ds, lo, hi):
  seqs = [np.asarray(ds[i][0], dtype=np.float32) for i in range(lo, hi)]
  lens = np.array([len(s) for s in seqs], dtype=np.int64)
  return np.concatenate(seqs), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64), lens


def _same_batches(got, want, where):
  got, want = list(got), list(want)
  assert len(got) == len(want) > 0
  for k, (a, b) in enumerate(zip(got, want)):
    assert len(a) == len(b) == 4
    for i, (x, y) in enumerate(zip(a, b)):
      assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (where, k, i)
      assert torch.equal(x, y), (where, k, i)
  return got


def test_pose_collate_and_normalise_pose_are_the_c_entry(dev):
  from lipreading_amd import landmarks
  c = PC.case(68, PC.RIGID_68, 2, True, 9)
  spec = landmarks.PoseSpec(c["tmpl"], radius=2, scale=True)
  want = pose_call(dev, c["lmk"], c["offsets"], c["lens"], 9, c["tmpl"], PC.RIGID_68, 2, True)
  lmk_d = torch.from_numpy(np.array(c["lmk"])).to(dev)
  off_d = torch.from_numpy(np.array(c["offsets"])).to(dev)
  lens_d = torch.from_numpy(np.array(c["lens"], dtype=np.int32)).to(dev)
  out, pose, status = landmarks.pose_collate(lmk_d, off_d, lens_d, 9, spec, return_pose=True)
  assert out.shape == (3, 9, 68, 3) and out.dtype == torch.float32 and pose.shape == (14, 13) and status.shape == (14,)
  assert out.cpu().numpy().tobytes() == want[0].tobytes() and pose.cpu().numpy().tobytes() == want[1].tobytes()
  assert torch.equal(landmarks.pose_collate(lmk_d, off_d, lens_d, 9, spec), out)
  lo, n = int(c["offsets"][2]), int(c["lens"][2])
  one = landmarks.normalise_pose(lmk_d[lo:lo + n].double(), spec)
  assert one.shape == (n, 68, 3) and torch.equal(one, out[2, :n])
  one, p1, s1 = landmarks.normalise_pose(lmk_d[lo:lo + n], spec, return_pose=True)
  assert torch.equal(p1, pose[lo:lo + n]) and torch.equal(s1, status[lo:lo + n])
  with pytest.raises(ValueError):
    landmarks.pose_collate(lmk_d[:, :4].contiguous(), off_d, lens_d, 9, spec)


def test_fit_template_finds_the_face_behind_the_clips(dev):
  from lipreading_amd import landmarks
  clips = [PC.make_clips(68, lens=(n,), seed=s)[0] for s, n in enumerate((7, 12, 9, 15, 11))]
  fitted = landmarks.fit_template(clips, device=dev)
  assert fitted.shape == (68, 3) and fitted.dtype == np.float32 and np.isfinite(fitted).all()
  again = landmarks.fit_template(clips, device=dev)
  assert again.tobytes() == fitted.tobytes()
  # canonical: eyes along +x, mouth below them along +y, centred on the rigid points
  eye = fitted[42:48].mean(0) - fitted[36:42].mean(0)
  mouth = fitted[48:68].mean(0) - 0.5 * (fitted[42:48].mean(0) + fitted[36:42].mean(0))
  assert eye[0] > 0 and abs(eye[1]) < 1e-3 and abs(eye[2]) < 1e-3 and mouth[1] > 0 and abs(mouth[2]) < 1e-3
  assert np.abs(fitted[list(PC.RIGID_68)].mean(0)).max() < 1e-3
  # it is the generator's face up to a similarity: aligned to it (numpy), the rigid points agree to the noise level
  tm = PC.template(68).astype(np.float64)
  idx = list(PC.RIGID_68)
  q, p = tm[idx], fitted.astype(np.float64)[idx]
  M = (q - q.mean(0)).T @ (p - p.mean(0))
  R = PC.rotation(M)
  s = np.trace(R @ M.T) / ((p - p.mean(0)) ** 2).sum()
  back = s * ((fitted.astype(np.float64) - p.mean(0)) @ R.T) + q.mean(0)
  assert np.abs(back[idx] - tm[idx]).max() < 1.0              # pixels; the clips carry noise of 0.4 a point
  raw = np.concatenate(clips).astype(np.float64)
  want_r = landmarks._rigid_frame(raw, PC.RIGID_68)[1].mean()
  assert abs(landmarks._rigid_frame(fitted.astype(np.float64), PC.RIGID_68)[1] - want_r) < 1e-3 * want_r
  assert landmarks.fit_template(clips, max_frames=10, iters=1, device=dev).shape == (68, 3)


def test_loaders_yield_the_pose_collates_batches(dev):
  from lipreading_amd import landmarks
  from lipreading_amd.augment import AugmentSpec
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.dataset import make_loader
  ds = _landmark_dataset(11, seed=9)
  spec = landmarks.PoseSpec(PC.template(68), radius=3, scale=True)
  tmpl = PC.template(68)
  plain = list(make_loader(ds, 4, make_collate_fn(dev, pose=spec)))
  assert len(plain) == 3 and plain[0][0].dtype == torch.float32 and plain[0][0].shape[2:] == (68, 3)
  for k, (lo, hi) in enumerate(((0, 4), (4, 8), (8, 11))):     # ... which is the C entry on the ragged data
    lmk, offsets, lens = _ragged(ds, lo, hi)
    want = pose_call(dev, lmk, offsets, lens, int(lens.max()), tmpl, PC.RIGID_68, 3, True)[0]
    assert plain[k][0].cpu().numpy().tobytes() == want.tobytes(), k
  pre = make_loader(ds, 4, None, prefetch=2, workers=2, device=dev, pose=spec)
  for _ in range(2):                                           # re-iterable, the slots' workspace is reused
    _same_batches(pre, plain, "prefetch")
  aug_spec = AugmentSpec.parse("tjitter=0.2,tmask=2x3", seed=5)
  aug = make_loader(ds, 4, None, prefetch=2, workers=2, device=dev, pose=spec, augment=aug_spec)
  first = list(aug)
  assert sum(not torch.equal(a[0], b[0]) for a, b in zip(first, plain)) >= 2      # the map reached the batches
  _same_batches(aug.plain(), plain, "plain pass of the augmented loader")
  for k, (lo, hi) in enumerate(((0, 4), (4, 8), (8, 11))):
    lmk, offsets, lens = _ragged(ds, lo, hi)
    tmap = aug_spec.draw(0, range(lo, hi), lens)[1]
    want = pose_call(dev, lmk, offsets, lens, int(lens.max()), tmpl, PC.RIGID_68, 3, True, tmap=tmap)[0]
    assert first[k][0].cpu().numpy().tobytes() == want.tobytes(), k
  # a loader built without pose yields today's bytes: the plain pad collate
  today = list(make_loader(ds, 4, make_collate_fn(dev)))
  _same_batches(make_loader(ds, 4, None, prefetch=2, workers=2, device=dev), today, "default prefetch")
  _same_batches(make_loader(ds, 4, None, prefetch=2, workers=2, device=dev, pose=None), today, "pose=None prefetch")
  assert not torch.equal(today[0][0], plain[0][0])
  for b, n in enumerate(today[0][1]):
    assert torch.equal(today[0][0][b, :int(n)].cpu(), torch.from_numpy(np.asarray(ds[b][0], dtype=np.float32)))
  for x in (pre, aug):
    x.close()


# ---- driver -----------------------------------------------------------------------------------------------------------
def test_driver_fits_writes_and_reloads_the_template(dev, tmp_path, capsys):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/nano", n_videos=6, captions_per_video=3, seed=11)
  path = str(tmp_path / "face" / "template.npy")
  flags = ["--root=" + root, "--data=synth/nano", "--batch_size=4", "--enable_ctc=True", "--ctc_only=True",
           "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=1", "--lmk_pose=similarity", "--lmk_pose_smooth=1",
           "--prefetch=2", "--lmk_pose_template=" + path]
  out = driver.run(**driver.parse_flags(flags))
  text = capsys.readouterr().out
  assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["ctc_loss"])
  assert "template fitted from" in text and "written to " + path in text and "template loaded" not in text
  with open(path, "rb") as f:
    written = f.read()
  tmpl = np.load(path)
  assert tmpl.shape == (68, 3) and tmpl.dtype == np.float32 and np.isfinite(tmpl).all()
  for loader in out["loaders"]:
    assert loader.pose is not None and loader.pose.radius == 1 and loader.pose.scale
    assert np.array_equal(loader.pose.template, tmpl)
    loader.close()
  assert not any(k for k in out["encoder"].state_dict() if "pose" in k or "template" in k)
  out = driver.run(**driver.parse_flags(flags))
  text = capsys.readouterr().out
  assert "template loaded from " + path in text and "fitted" not in text
  with open(path, "rb") as f:
    assert f.read() == written
  for loader in out["loaders"]:
    loader.close()
