"""No GPU: landmarks.MIRROR_68, augment.LandmarkAugmentSpec (the policy, its draws, parse / str), the slot layout with
the landmark records, the drawing ahead of the host stage, the driver's flag, and the numpy restatement the GPU file
grades against (tests/lmk_aug_cases.py).  The device stage is tests/test_gpu_lmk_aug.py."""
import numpy as np
import pytest

from lipreading_amd import loader as LD
from lipreading_amd.augment import AugmentSpec, LandmarkAugmentSpec
from tests import lmk_aug_cases as AC

FULL = "mirror=0.5,rot=10/10/15,scale=0.1,stretch=0.05,shift=0.05,jitter=0.01"


def _fields(rec):
  """uint64 (B,16) -> A (B,3,3), shift (B,3), jitter (B,), mirror (B,), key (B,) uint64, word 15."""
  f = np.ascontiguousarray(rec).view(np.float64)
  return f[:, :9].reshape(-1, 3, 3), f[:, 9:12], f[:, 12], f[:, 13], rec[:, 14], rec[:, 15]


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [0, 1, 0xDEADBEEF12345678])
def test_the_unit_noise_has_zero_mean_unit_variance_and_its_bound(key):
  g = AC.unit_noise(key, 1000, 68)[:, :, :].ravel()[:200000]
  assert g.size == 200000
  print("key %#x: mean %.4f var %.4f max %.4f" % (key, g.mean(), g.var(), np.abs(g).max()))
  assert abs(g.mean()) <= 0.01 and abs(g.var() - 1.0) <= 0.02
  assert np.abs(g).max() <= 3.4641


def test_the_restatement_agrees_with_itself_under_another_summation_order():
  worst = 0.0
  for c in AC.parity_cases():
    other = AC.augment(c["x"], c["lens"], c["rec"], c["perm"], pairwise=True)[0]
    worst = max(worst, AC.worst_ulps(other, c["y"]))
    assert np.isfinite(c["y"]).all()
  print("ascending against pairwise sums: %.3g ulp" % worst)
  assert worst <= 1.0


def test_the_restatement_zeroes_what_is_empty_and_ignores_it_in_the_statistics():
  x, lens = AC.semantics_case()
  live = AC.live_rows(x, lens)
  assert live.sum(axis=1).tolist() == [4, 7, 0, 8]
  assert not live[1, 3] and not live[1, 6] and not live[3, 2] and live[1, 5] and not live[0, 4:].any()
  rec = AC.records("full_jitter", 4)
  y, stats, _ = AC.augment(x, lens, rec, AC.perm_for(68))
  assert not y[~live].any() and np.isfinite(y).all() and (y[live] != 0).any(axis=(1, 2)).all()
  assert stats[2].tolist() == [0, 0, 0, 0]
  rows = x[1][live[1]].astype(np.float64).reshape(-1, 3)
  assert np.allclose(stats[1, :3], rows.mean(axis=0), rtol=1e-13)
  assert np.isclose(stats[1, 3], np.sqrt(((rows - rows.mean(axis=0)) ** 2).sum(axis=1).mean()), rtol=1e-10)


def test_a_mirror_about_the_clip_centre_applied_twice_returns_the_input():
  """The second pass sees x + e, e the first pass's fp32 rounding error: at most half an ulp OF THE MIRRORED VALUE, plus
  twice the shift of the centre, which is a mean of such errors.  That is inside one ulp of x where a value and its
  mirror image lie in the same binade, so the faces here are narrowed until every x and 2 c_x - x lies in [64, 128);
  y and z pass through (v - c) + c, which rounds back to v.  (On the generator's own faces, x from 30 to 170, the
  same round trip measures 5 ulp of the smaller value: that is fp32, not the restatement.)"""
  for npts in (68, 4):
    c = AC.case(npts, 9, "mirror")
    live = AC.live_rows(c["x"], c["lens"])
    x = np.array(c["x"])
    x[..., 0] = np.where(live[:, :, None], np.float32(96.0) + (x[..., 0] - np.float32(100.0)) * np.float32(0.15), 0)
    once = AC.augment(x, c["lens"], c["rec"], c["perm"])[0]
    for v in (x[live][..., 0], once[live][..., 0]):
      assert v.min() >= 64.0 and v.max() < 128.0
    twice = AC.augment(once, c["lens"], c["rec"], c["perm"])[0]
    assert not np.array_equal(once, x) and np.array_equal(once[:, :, c["perm"], 1:], x[..., 1:])
    print("npts %d: %.3g ulp" % (npts, AC.worst_ulps(twice, x)))
    assert AC.worst_ulps(twice, x) <= 1.0


def test_the_exact_case_is_exact_in_the_restatement():
  x, rec, want = AC.exact_case()
  y, stats, y64 = AC.augment(x, [4], rec, AC.perm_for(4))
  assert stats[0].tolist() == [10.0, 20.0, 5.0, 5.0]
  assert y.tobytes() == want.tobytes() and np.array_equal(want, np.round(want))


# ---- MIRROR_68 ----------------------------------------------------------------------------------------------------------
def test_mirror_68_is_an_involution_with_the_midline_fixed():
  from lipreading_amd import landmarks
  p = landmarks.MIRROR_68
  assert len(p) == 68 and sorted(p) == list(range(68))
  assert all(p[p[j]] == j for j in range(68))
  assert tuple(j for j in range(68) if p[j] == j) == AC.MIRROR_68_FIXED
  assert list(p) == AC.mirror_68()
  assert p[0] == 16 and p[17] == 26 and p[21] == 22 and p[31] == 35 and p[36] == 45 and p[40] == 47 and p[41] == 46
  assert p[48] == 54 and p[55] == 59 and p[60] == 64 and p[65] == 67
  assert landmarks.check_mirror_perm(list(p), 68) == p
  for bad in ([0] * 68, list(range(67)), list(range(67)) + [68], [1, 2, 0] + list(range(3, 68)), "x"):
    with pytest.raises(ValueError):
      landmarks.check_mirror_perm(bad, 68)


# ---- the policy -----------------------------------------------------------------------------------------------------------
def test_parse_reads_the_drivers_string_and_round_trips():
  s = LandmarkAugmentSpec.parse(FULL)
  assert (s.mirror, s.rot, s.scale, s.stretch, s.shift, s.jitter, s.seed) == (0.5, (10.0, 10.0, 15.0), 0.1, 0.05, 0.05,
                                                                               0.01, 0)
  assert str(s) == "mirror=0.5,rot=10.0/10.0/15.0,scale=0.1,stretch=0.05,shift=0.05,jitter=0.01"
  assert LandmarkAugmentSpec.parse(str(s)) == s and hash(LandmarkAugmentSpec.parse(str(s))) == hash(s)
  assert LandmarkAugmentSpec.parse(FULL, seed=3) != s and LandmarkAugmentSpec.parse(FULL, seed=3).seed == 3
  assert LandmarkAugmentSpec.parse("") is None and LandmarkAugmentSpec.parse(None) is None
  assert LandmarkAugmentSpec.parse(" rot = 5/0/0 ").rot == (5.0, 0.0, 0.0)
  assert s != AugmentSpec() and LandmarkAugmentSpec() == LandmarkAugmentSpec(rot=(0, 0, 0))
  for bad in ("blur=1", "mirror", "mirror=0.5,mirror=0.5", "rot=10", "rot=1/2/3/4", "rot=a/b/c", "scale=x",
              "mirror=1.5", "rot=50/0/0", "rot=-1/0/0", "scale=0.6", "stretch=0.3", "shift=0.7", "jitter=0.2",
              "flip=0.5"):
    with pytest.raises(ValueError):
      LandmarkAugmentSpec.parse(bad)
  # AugmentSpec is what it was
  assert AugmentSpec.FIELDS == ("flip", "shift", "zoom", "tjitter", "tmask")
  assert str(AugmentSpec(flip=0.5, tmask=(2, 10))) == "flip=0.5,shift=0.0,zoom=0.0,tjitter=0.0,tmask=2x10"


def test_the_identity_spec_draws_identity_records():
  rec = LandmarkAugmentSpec(seed=9).draw(3, range(5), [7, 8, 9, 10, 11])
  assert rec.dtype == np.uint64 and rec.shape == (5, 16)
  assert all(r.tobytes() == AC.record().tobytes() for r in rec)


def test_a_record_depends_on_seed_pass_index_and_length_alone():
  spec = LandmarkAugmentSpec.parse(FULL, seed=4)
  lens = np.arange(40) % 13 + 5
  whole = spec.draw(2, range(100, 140), lens)
  assert whole.dtype == np.uint64 and whole.shape == (40, 16) and whole.flags.c_contiguous
  for lo, hi in ((0, 4), (4, 8), (8, 40), (17, 18)):           # chunking: a DRAW_AHEAD draw equals per-batch draws
    assert spec.draw(2, range(100 + lo, 100 + hi), lens[lo:hi]).tobytes() == whole[lo:hi].tobytes()
  order = np.random.RandomState(0).permutation(40)              # batch composition
  assert spec.draw(2, 100 + order, lens[order]).tobytes() == whole[order].tobytes()
  assert spec.draw(2, range(100, 140), lens).tobytes() == whole.tobytes()
  for other in (LandmarkAugmentSpec.parse(FULL, seed=5).draw(2, range(100, 140), lens),
                spec.draw(3, range(100, 140), lens), spec.draw(2, range(101, 141), lens),
                spec.draw(2, range(100, 140), lens + 1)):
    assert not (other[:, :15] == whole[:, :15]).all(axis=1).any()


def test_the_draws_lie_inside_their_limits_and_compose_as_stated():
  n = 4096
  lens = np.full(n, 30)
  spec = LandmarkAugmentSpec.parse("mirror=0.5,rot=10/20/15,scale=0.1,shift=0.05,jitter=0.01", seed=1)
  A, shift, jitter, mirror, key, last = _fields(spec.draw(0, range(n), lens))
  assert set(np.unique(mirror)) == {0.0, 1.0} and abs(mirror.mean() - 0.5) <= 0.04
  assert (jitter == 0.01).all() and (last == 0).all() and len(np.unique(key)) == n
  assert np.abs(shift).max() <= 0.05 and np.abs(shift).max() > 0.04 and (np.abs(shift.mean(axis=0)) < 0.005).all()
  det = np.linalg.det(A)
  assert ((det < 0) == (mirror == 1.0)).all()
  s = np.cbrt(np.abs(det))                                     # stretch is off: A = s R diag(+-1, 1, 1)
  assert s.min() >= 0.9 - 1e-12 and s.max() <= 1.1 + 1e-12 and s.max() - s.min() > 0.15
  R = A * np.where(mirror == 1.0, -1.0, 1.0)[:, None, None] * np.array([1.0, 0.0, 0.0]) + A * np.array([0.0, 1.0, 1.0])
  R = R / s[:, None, None]
  assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12 and np.allclose(np.linalg.det(R), 1.0)
  # R = Rz(roll) Ry(yaw) Rx(pitch): yaw = -asin(R[2][0]), roll = atan2(R[1][0], R[0][0]), pitch = atan2(R[2][1], R[2][2])
  yaw = np.degrees(-np.arcsin(R[:, 2, 0]))
  roll = np.degrees(np.arctan2(R[:, 1, 0], R[:, 0, 0]))
  pitch = np.degrees(np.arctan2(R[:, 2, 1], R[:, 2, 2]))
  for got, limit in ((yaw, 10.0), (pitch, 20.0), (roll, 15.0)):
    assert np.abs(got).max() <= limit + 1e-9 and np.abs(got).max() > 0.9 * limit and abs(got.mean()) < 0.06 * limit
  # stretch alone: A = diag(1 + e_x, 1 + e_y, 1)
  A = _fields(LandmarkAugmentSpec(stretch=0.25, seed=2).draw(0, range(n), lens))[0]
  off = A * (1 - np.eye(3))
  assert not off.any() and (A[:, 2, 2] == 1.0).all()
  for k in (0, 1):
    assert 0.75 <= A[:, k, k].min() < 0.8 and 1.2 < A[:, k, k].max() <= 1.25
  assert abs(np.corrcoef(A[:, 0, 0], A[:, 1, 1])[0, 1]) < 0.06
  # a limit of zero draws exactly nothing
  A, shift, jitter, mirror, _, _ = _fields(LandmarkAugmentSpec(mirror=1.0, seed=2).draw(0, range(8), lens[:8]))
  assert (mirror == 1.0).all() and not shift.any() and not jitter.any()
  assert all(np.array_equal(a, np.diag([-1.0, 1.0, 1.0])) for a in A)


def test_the_stream_is_not_augment_specs():
  n = 512
  lens = np.full(n, 20)
  clip = AugmentSpec(shift=0.5, zoom=0.5, seed=6).draw(0, range(n), lens)[0].astype(np.float64)
  A, shift = _fields(LandmarkAugmentSpec(shift=0.5, scale=0.5, seed=6).draw(0, range(n), lens))[:2]
  theirs = np.stack([clip[:, 0] / 0.5, clip[:, 1] / 0.5, (clip[:, 2] - 1.0) / 0.5], axis=1)      # each in [-1, 1]
  mine = np.concatenate([shift / 0.5, (A[:, 0, 0, None] - 1.0) / 0.5], axis=1)
  for a in theirs.T:                                            # same seed, pass, indices and lengths: other numbers
    for b in mine.T:
      assert np.abs(a - b).mean() > 0.3 and abs(np.corrcoef(a, b)[0, 1]) < 0.2


# ---- the slot ---------------------------------------------------------------------------------------------------------------
def _dataset(n, seed=0, npts=68):
  rng = np.random.RandomState(seed)
  return [(rng.randn(int(t), npts, 3), np.array([1] + list(rng.randint(4, 60, 3)) + [2]))
          for t in rng.randint(5, 14, n)]


def test_pack_batch_without_the_policy_is_todays_and_with_it_holds_the_draw():
  ds = _dataset(5)
  aug = AugmentSpec(tjitter=0.2, tmask=(1, 3), seed=3)
  spec = LandmarkAugmentSpec.parse(FULL, seed=3)
  for augment in (None, aug):
    kw = dict(augment=augment, pass_no=2, indices=range(10, 15)) if augment is not None else {}
    a, b, c = (np.full(1 << 20, 0xAB, np.uint8) for _ in range(3))
    pa = LD.pack_batch(ds, False, a, **kw)
    pb = LD.pack_batch(ds, False, b, lmk_augment=None, lmk_records=None, **kw)
    assert a.tobytes() == b.tobytes() and vars(pa).keys() == vars(pb).keys()
    assert not pa.lmk_augmented and pa.lmk_aug_off == 0
    kw2 = dict(kw, pass_no=2, indices=range(10, 15))
    pc = LD.pack_batch(ds, False, c, lmk_augment=spec, **kw2)
    assert pc.lmk_augmented and pc.lmk_aug_off == pa.nbytes and pc.nbytes == pa.nbytes + LD._align(5 * 128)
    assert pc.lmk_aug_off % 256 == 0
    assert c[:pa.nbytes].tobytes() == a[:pa.nbytes].tobytes()       # every other region is where and what it was
    for name in ("frames_off", "offsets_off", "lens_off", "aug_off", "tmap_off", "augmented", "B", "rows", "t_max"):
      assert getattr(pc, name) == getattr(pa, name), name
    rec = pc.region(c, "lmk_aug")
    assert rec.dtype == np.uint64 and rec.shape == (5, 16)
    assert rec.tobytes() == spec.draw(2, range(10, 15), pa.frame_lens).tobytes()
    assert (c[pc.nbytes:] == 0xAB).all()
    # records the caller drew already are taken as they are
    given = spec.draw(7, range(5), pa.frame_lens)
    pd = LD.pack_batch(ds, False, c, lmk_augment=spec, lmk_records=given, **kw2)
    assert pd.region(c, "lmk_aug").tobytes() == given.tobytes()
  with pytest.raises(AssertionError):
    LD.pack_batch(ds, False, a, lmk_augment=spec)                    # no indices
  assert LD._slot_bytes(ds, [(0, 5)], False, False, True) == LD._slot_bytes(ds, [(0, 5)], False) + LD._align(5 * 128)
  assert LD._slot_bytes(ds, [(0, 5)], False, True, True) == LD._slot_bytes(ds, [(0, 5)], False, True) + LD._align(640)
  assert LD._slot_bytes(ds, [(0, 5)], False, True, False) == LD._slot_bytes(ds, [(0, 5)], False, True)


@pytest.mark.parametrize("with_aug", [False, True])
def test_the_host_stage_draws_ahead_what_a_batch_would_draw_for_itself(with_aug):
  ds = _dataset(3 * LD.DRAW_AHEAD + 5, seed=1, npts=4)           # more than one chunk of DRAW_AHEAD batches of 2
  spec = LandmarkAugmentSpec.parse(FULL, seed=8)
  aug = AugmentSpec(tjitter=0.3, seed=8) if with_aug else None
  stage = LD.HostStage(ds, 2, workers=3, augment=aug, lmk_augment=spec)
  plain = LD.HostStage(ds, 2, workers=1, augment=aug)
  assert stage.slot_bytes == plain.slot_bytes + 256 and len(stage) > LD.DRAW_AHEAD
  for pass_no in (0, 1):
    assert stage.pass_no == pass_no
    for k, (pb, pp) in enumerate(zip(stage, plain)):
      lo, hi = stage.plan[k]
      buf, ref = stage._np[pb.slot], plain._np[pp.slot]
      assert pb.lmk_augmented and not pp.lmk_augmented and pb.augmented == with_aug
      assert pb.region(buf, "lmk_aug").tobytes() == spec.draw(pass_no, range(lo, hi), pb.frame_lens).tobytes()
      assert pb.lmk_aug_off == pp.nbytes                             # behind every other region, which are today's
      for name in ("frames", "offsets", "lens") + (("tmap",) if with_aug else ()):
        assert pb.region(buf, name).tobytes() == pp.region(ref, name).tobytes(), name
  # a pass with augmentation off carries no records and leaves the pass number alone
  ep = stage.open(augmented=False)
  ep.submit(0)
  pb = ep.get(0)
  assert not pb.lmk_augmented and not pb.augmented and stage.pass_no == 2
  stage.close()
  plain.close()


def test_a_chunk_that_cannot_be_drawn_falls_back_to_a_draw_per_batch():
  ds = _dataset(12, seed=2, npts=4)
  ds[9] = (None, ds[9][1])                                      # batch 4 of 6 is malformed
  spec = LandmarkAugmentSpec.parse(FULL, seed=8)
  stage = LD.HostStage(ds, 2, workers=2, lmk_augment=spec)
  it = iter(stage)
  for k in range(4):
    pb = next(it)
    lo, hi = stage.plan[k]
    assert pb.region(stage._np[pb.slot], "lmk_aug").tobytes() == spec.draw(0, range(lo, hi), pb.frame_lens).tobytes()
  with pytest.raises(Exception):
    next(it)
  stage.close()


def test_the_loader_refuses_the_pixel_regime_and_make_loader_the_plain_loader():
  from lipreading_amd import dataset as DS
  spec = LandmarkAugmentSpec.parse(FULL)
  with pytest.raises(ValueError) as e:
    LD.PrefetchLoader(_dataset(3), 2, "cuda", pixels=True, lmk_augment=spec)
  assert "lmk_augment" in str(e.value)
  with pytest.raises(ValueError) as e:
    DS.make_loader(_dataset(3), 2, None, lmk_augment=spec)
  assert "lmk_augment" in str(e.value) and "prefetch" in str(e.value)


# ---- the driver -----------------------------------------------------------------------------------------------------------
def test_driver_flags():
  from lipreading_amd import driver
  assert driver.DEFAULTS["lmk_augment"] == ""
  f = driver.parse_flags([])
  assert f["lmk_augment"] == "" and driver.lmk_augment_spec(f) is None
  f = driver.parse_flags(["--prefetch=2", "--lmk_augment=" + FULL])
  assert f["lmk_augment"] == FULL and f["augment"] == ""
  assert driver.lmk_augment_spec(f) == LandmarkAugmentSpec.parse(FULL, seed=driver.DEFAULTS["seed"])   # None means --seed
  assert driver.lmk_augment_spec(driver.parse_flags(["--prefetch=2", "--lmk_augment=" + FULL, "--seed=5"])).seed == 5
  f = driver.parse_flags(["--prefetch=2", "--lmk_augment=" + FULL, "--seed=5", "--augment_seed=77",
                          "--augment=tjitter=0.1"])
  assert driver.lmk_augment_spec(f).seed == 77 and driver.augment_spec(f).seed == 77
  with pytest.raises(ValueError) as e:
    driver.parse_flags(["--lmk_augment=" + FULL])
  assert "--lmk_augment" in str(e.value) and "--prefetch" in str(e.value)
  with pytest.raises(ValueError) as e:
    driver.parse_flags(["--prefetch=2", "--frontend=conv3d", "--lmk_augment=" + FULL])
  assert "--lmk_augment" in str(e.value) and "conv3d" in str(e.value)
  with pytest.raises(ValueError):
    driver.parse_flags(["--prefetch=2", "--lmk_augment=blur=1"])
  with pytest.raises(ValueError) as e:                                    # run() checks before it touches data or the GPU
    driver.run(lmk_augment="mirror=0.5", data="no/such/dataset", root="/nonexistent")
  assert "--lmk_augment" in str(e.value) and "--prefetch" in str(e.value)
  with pytest.raises(ValueError):
    driver.run(lmk_augment="mirror=0.5", prefetch=2, frontend="conv3d", data="no/such/dataset", root="/nonexistent")
  with pytest.raises(ValueError):
    driver.run(lmk_augment="mirror=2", prefetch=2, data="no/such/dataset", root="/nonexistent")


# ---- the entry's declaration and its kernels' resources ---------------------------------------------------------------------
def test_the_entry_is_declared_and_bound():
  from lipreading_amd import _C
  assert _C.LR_LMK_AUG_MAX_POINTS == 256 and _C.LR_LMK_AUG_REC_WORDS == 16 == AC.WORDS
  assert LD.LMK_REC_BYTES == 8 * _C.LR_LMK_AUG_REC_WORDS
  restype, args = _C.SIGNATURES["lr_lmk_augment_f32"]
  assert restype is _C.c_int and len(args) == 12 and args[:8] == [_C.P] * 7 + [__import__("ctypes").c_size_t]
  assert _C.SIGNATURES["lr_lmk_augment_workspace_bytes"] == (__import__("ctypes").c_size_t, [_C.c_int])
