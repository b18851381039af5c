"""CPU: lipreading_amd.augment (policy, stateless draws), the augmentation regions of the loader's host stage, the
driver's and make_loader's argument handling, the declarations of the two augmenting entry points and the compiled
resources of their kernels, and the numpy restatement the GPU file grades against (tests/augment_cases.py).  The
device stage is tests/test_gpu_augment.py."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from lipreading_amd import _build, _C
from lipreading_amd import dataset as DS
from lipreading_amd import loader as LD
from lipreading_amd.augment import AugmentSpec
from tests import augment_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL = "flip=0.5,shift=0.08,zoom=0.1,tjitter=0.05,tmask=2x10"


# ---- parse ----------------------------------------------------------------------------------------------------------
def test_parse_reads_the_drivers_string_and_round_trips():
  s = AugmentSpec.parse(FULL)
  assert (s.flip, s.shift, s.zoom, s.tjitter, s.tmask, s.seed) == (0.5, 0.08, 0.1, 0.05, (2, 10), 0)
  assert AugmentSpec.parse(str(s)) == s
  assert AugmentSpec.parse(str(s), seed=9) != s and AugmentSpec.parse(str(s), seed=9).seed == 9
  assert AugmentSpec.parse("") is None and AugmentSpec.parse("  ") is None and AugmentSpec.parse(None) is None
  part = AugmentSpec.parse(" shift=0.25 , tmask=8x0 ")
  assert part == AugmentSpec(shift=0.25, tmask=(8, 0)) and AugmentSpec.parse(str(part)) == part
  assert AugmentSpec() == AugmentSpec.parse("flip=0")
  for s in (AugmentSpec(flip=1.0, shift=0.5, zoom=0.5, tjitter=0.5, tmask=(8, 1000)), AugmentSpec(tjitter=1 / 3.0)):
    assert AugmentSpec.parse(str(s)) == s


@pytest.mark.parametrize("text", [
    "blur=0.5", "flip", "flip=0.5,flip=0.5", "seed=3", "flip=x", "flip=1.01", "flip=-0.1", "shift=0.51", "shift=-0.01",
    "zoom=0.6", "zoom=-1", "tjitter=0.500001", "tjitter=-0.2", "tmask=9x3", "tmask=-1x3", "tmask=2x-1", "tmask=2",
    "tmask=2.5x3", "tmask=ax3", "flip=0.5;shift=0.1", "flip=nan"])
def test_parse_rejects(text):
  with pytest.raises(ValueError):
    AugmentSpec.parse(text)


def test_constructor_rejects_what_parse_rejects():
  for bad in (dict(flip=1.5), dict(shift=0.6), dict(zoom=-0.1), dict(tjitter=0.7), dict(tmask=(9, 1)), dict(tmask=(1, -1)),
              dict(tmask=3), dict(tmask=(1.5, 2))):
    with pytest.raises(ValueError):
      AugmentSpec(**bad)


# ---- draw: properties -----------------------------------------------------------------------------------------------
def _clips(n, seed=0):
  rng = np.random.RandomState(seed)
  lens = np.concatenate([np.arange(1, 121), rng.randint(1, 121, n - 120)])
  return np.arange(n), lens


def _split(tmap, lens):
  return np.split(tmap, np.cumsum(lens)[:-1])


@pytest.mark.parametrize("text", [FULL, "flip=0.3,shift=0.5,zoom=0.5,tjitter=0.5,tmask=8x1000", "tjitter=0.3,tmask=2x3",
                                  "flip=1,shift=0.15,zoom=0.25", "tmask=1x1"])
def test_draw_properties(text):
  spec = AugmentSpec.parse(text, seed=11)
  n = 2400
  idx, lens = _clips(n)
  clip, tmap = spec.draw(0, idx, lens)
  assert clip.dtype == np.float32 and clip.shape == (n, 4)
  assert tmap.dtype == np.int32 and tmap.shape == (int(lens.sum()),)      # one entry per frame
  n_masked = 0
  for ln, m in zip(lens, _split(tmap, lens)):
    live = m[m >= 0]
    assert len(m) == ln and (m >= -1).all()
    assert (np.diff(live) >= 0).all() and (live < ln).all()              # monotone, inside the clip
    assert (m < 0).sum() <= ln // 2                                       # at most half a clip is masked
    n_masked += int((m < 0).sum())
    if ln == 1:
      assert list(m) == [0]
  dx, dy, zoom, flip = (clip[:, i].astype(np.float64) for i in range(4))
  assert (np.abs(dx) <= spec.shift).all() and (np.abs(dy) <= spec.shift).all()
  assert (zoom >= 1 - spec.zoom).all() and (zoom <= 1 + spec.zoom).all()
  assert set(np.unique(flip)) <= {0.0, 1.0}
  p = spec.flip
  assert abs(flip.mean() - p) <= 4 * math.sqrt(p * (1 - p) / n)
  assert abs(dx.mean()) <= 4 * spec.shift / math.sqrt(3 * n) and abs(dy.mean()) <= 4 * spec.shift / math.sqrt(3 * n)
  # the policy is not a no-op where it is switched on
  if spec.shift:
    assert dx.std() > 0.4 * spec.shift and not np.array_equal(dx, dy)     # (uniform: shift / sqrt(3))
  if spec.zoom:
    assert zoom.std() > 0.4 * spec.zoom
  if spec.tmask[0] and spec.tmask[1]:
    assert n_masked > 0
  if spec.tjitter:
    ident = np.concatenate([np.arange(ln) for ln in lens])
    moved = (tmap >= 0) & (tmap != ident)
    assert moved.any()
    long = [m for ln, m in zip(lens, _split(tmap, lens)) if ln >= 60]
    assert any((np.diff(m[m >= 0]) == 0).any() for m in long) and any((np.diff(m[m >= 0]) >= 2).any() for m in long)


def test_the_all_zero_spec_draws_the_identity():
  idx, lens = _clips(300)
  for spec in (AugmentSpec(), AugmentSpec(seed=5, tmask=(4, 0)), AugmentSpec(tmask=(0, 10))):
    clip, tmap = spec.draw(3, idx, lens)
    want_clip, want_map = AC.identity_records(lens)
    assert np.array_equal(clip, want_clip) and np.array_equal(tmap, want_map)
    assert clip.dtype == np.float32 and tmap.dtype == np.int32


# ---- draw: reproducibility ------------------------------------------------------------------------------------------
def test_a_record_depends_on_seed_pass_index_and_length_only():
  spec = AugmentSpec.parse(FULL, seed=21)
  rng = np.random.RandomState(2)
  lens = rng.randint(1, 90, 64)
  idx = np.arange(64)
  for p in (0, 1, 7):
    for i in (0, 13, 31, 63):
      alone = spec.draw(p, [i], [lens[i]])
      for group in (np.arange(i, i + 4) % 64, np.arange(i - 3, i + 1) % 64, np.arange(i, i + 32) % 64,
                    np.arange(i - 31, i + 1) % 64):                       # batches of 4 and 32, first and last
        clip, tmap = spec.draw(p, group, lens[group])
        at = list(group).index(i)
        assert np.array_equal(clip[at], alone[0][0])
        assert np.array_equal(_split(tmap, lens[group])[at], alone[1])
  a, b = spec.draw(0, idx, lens), spec.draw(1, idx, lens)
  assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])          # passes differ
  c = AugmentSpec.parse(FULL, seed=22).draw(0, idx, lens)
  assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])          # seeds differ
  again = AugmentSpec.parse(FULL, seed=21).draw(0, idx, lens)
  assert np.array_equal(a[0], again[0]) and np.array_equal(a[1], again[1])
  # and two clips of one pass do not share a record
  assert len({tuple(r) for r in a[0]}) == 64


# ---- packing --------------------------------------------------------------------------------------------------------
def _landmark_samples(n, seed=0, lo=3, hi=17):
  rng = np.random.RandomState(seed)
  lens = np.sort(rng.randint(lo, hi, n))
  return [(rng.randn(int(t), 68, 3) * 50, np.array([1] + list(rng.randint(4, 64, rng.randint(1, 6))) + [2]))
          for t in lens]


def _pixel_samples(n, seed=0, hw=(12, 16), lo=1, hi=9):
  rng = np.random.RandomState(seed)
  lens = np.sort(rng.randint(lo, hi, n))
  H, W = hw
  return [((rng.randint(0, 256, (int(t), 3, H, W)).astype(np.uint8), rng.uniform(0, W, (int(t), 68, 3))),
           np.array([1] + list(rng.randint(4, 64, rng.randint(1, 6))) + [2])) for t in lens]


def _slots(stage):
  """Every batch's (layout, bytes) of one pass."""
  out = []
  for pb in stage:
    buf = stage.slots[pb.slot].numpy()
    out.append(((pb.B, pb.rows, pb.t_max, pb.nbytes, pb.frames_off, pb.lmk_off, pb.offsets_off, pb.lens_off, pb.aug_off,
                 pb.tmap_off, pb.augmented),
                {name: pb.region(buf, name).tobytes() for name in
                 ("frames", "offsets", "lens") + (("lmk",) if pb.pixels else ()) +
                 ((("aug",) if pb.pixels else ()) + ("tmap",) if pb.augmented else ())},
                (pb.frame_lens.copy(), pb.chars.copy(), pb.char_lens.copy())))
  return out


def _same(a, b):
  return len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and all(np.array_equal(p, q) for p, q in zip(x[2], y[2]))
                                  for x, y in zip(a, b))


@pytest.mark.parametrize("pixels", [False, True])
def test_host_stage_packs_the_drawn_records_whatever_the_depth_and_the_workers(pixels):
  ds = _pixel_samples(23, seed=5) if pixels else _landmark_samples(23, seed=5)
  spec = AugmentSpec.parse(FULL, seed=4)
  small = LD.HostStage(ds, 4, pixels=pixels, depth=1, workers=1, augment=spec)
  big = LD.HostStage(ds, 4, pixels=pixels, depth=3, workers=4, augment=spec)
  clean = LD.HostStage(ds, 4, pixels=pixels, depth=2, workers=2)
  first, first_big, plain = _slots(small), _slots(big), _slots(clean)
  assert _same(first, first_big)
  assert small.pass_no == big.pass_no == 1 and clean.pass_no == 0
  # the regions hold spec.draw's records of that pass, behind today's layout
  for k, ((layout, regions, host), (p_layout, p_regions, p_host)) in enumerate(zip(first, plain)):
    lo, hi = small.plan[k]
    lens = [len(ds[i][0][0]) if pixels else len(ds[i][0]) for i in range(lo, hi)]
    clip, tmap = spec.draw(0, range(lo, hi), lens)
    B, rows, t_max, nbytes, f_off, l_off, o_off, n_off, a_off, m_off, augmented = layout
    assert augmented and not p_layout[-1]
    assert layout[:3] == p_layout[:3] and layout[4:8] == p_layout[4:8]
    assert a_off == p_layout[3] and a_off % 256 == 0 and m_off % 256 == 0  # behind today's last region, 256-aligned
    assert m_off == a_off + (LD._align(16 * B) if pixels else 0)
    assert nbytes == m_off + LD._align(4 * rows) <= small.slot_bytes
    assert regions["tmap"] == tmap.tobytes()
    if pixels:
      assert regions["aug"] == clip.tobytes()
    for name in p_regions:                                                # frames, landmarks, offsets, lens: unchanged
      assert regions[name] == p_regions[name], name
    assert all(np.array_equal(a, b) for a, b in zip(host, p_host))       # frame_lens, chars, char_lens: unchanged
  # today's nbytes without a spec
  for k, (layout, _, _) in enumerate(plain):
    lo, hi = clean.plan[k]
    rows = layout[1]
    per_row = 3 * 12 * 16 if pixels else 204 * 4
    want = LD._align(rows * per_row) + (LD._align(rows * 204 * 4) if pixels else 0) + LD._align(8 * (hi - lo)) + \
        LD._align(4 * (hi - lo))
    assert layout[3] == want
  # a second pass differs, set_pass(0) reproduces the first
  second = _slots(small)
  assert small.pass_no == 2 and not _same(first, second)
  assert [x[1]["frames"] for x in second] == [x[1]["frames"] for x in first]
  small.set_pass(0)
  assert _same(_slots(small), first) and small.pass_no == 1
  # an abandoned pass counts, an un-augmented one does not
  for _ in big:
    break
  assert big.pass_no == 2
  ep = big.open(augmented=False)
  ep.close()
  assert big.pass_no == 2
  assert _same(_slots(big), _slots_at(small, 2))


def _slots_at(stage, n):
  stage.set_pass(n)
  return _slots(stage)


def test_pack_batch_without_a_spec_takes_no_new_argument_and_needs_indices_with_one():
  ds = _landmark_samples(4, seed=1)
  buf = np.zeros(1 << 20, np.uint8)
  a = LD.pack_batch(ds, False, buf)
  b = LD.pack_batch(ds, False, buf.copy(), augment=None, pass_no=5, indices=None)
  assert a.nbytes == b.nbytes and not a.augmented and not b.augmented
  with pytest.raises(AssertionError):
    LD.pack_batch(ds, False, buf, augment=AugmentSpec(flip=0.5))
  c = LD.pack_batch(ds, False, buf, augment=AugmentSpec(tjitter=0.4, seed=1), pass_no=2, indices=[10, 11, 12, 13])
  want = AugmentSpec(tjitter=0.4, seed=1).draw(2, [10, 11, 12, 13], [len(s[0]) for s in ds])[1]
  assert c.augmented and np.array_equal(c.region(buf, "tmap"), want)
  with pytest.raises(AssertionError):
    c.region(buf, "aug")                                                 # the landmark regime carries the map alone


# ---- errors and bindings --------------------------------------------------------------------------------------------
def test_augmentation_needs_the_prefetch_loader():
  ds = _landmark_samples(5)
  spec = AugmentSpec(flip=0.5)
  with pytest.raises(ValueError) as e:
    DS.make_loader(ds, 2, lambda b: b, augment=spec, prefetch=0)
  assert "augment" in str(e.value) and "prefetch" in str(e.value)
  with pytest.raises(ValueError):
    DS.make_loader(ds, 2, lambda b: b, augment=spec)
  assert isinstance(DS.make_loader(ds, 2, lambda b: b, augment=None), DS.BatchLoader)
  with pytest.raises(_C.LipReadingHipError):                              # forwarded to PrefetchLoader, which needs the GPU
    DS.make_loader(ds, 2, None, prefetch=2, augment=spec, device=torch.device("cpu"))


def test_driver_flags():
  from lipreading_amd import driver
  assert driver.DEFAULTS["augment"] == "" and driver.DEFAULTS["augment_seed"] is None
  f = driver.parse_flags([])
  assert f["augment"] == "" and f["augment_seed"] is None and driver.augment_spec(f) is None
  f = driver.parse_flags(["--prefetch=2", "--augment=" + FULL])
  assert f["augment"] == FULL and f["augment_seed"] is None
  assert driver.augment_spec(f) == AugmentSpec.parse(FULL, seed=driver.DEFAULTS["seed"])      # None means --seed
  f = driver.parse_flags(["--prefetch=2", "--augment=" + FULL, "--seed=5"])
  assert driver.augment_spec(f).seed == 5
  f = driver.parse_flags(["--prefetch=2", "--augment=" + FULL, "--seed=5", "--augment_seed=77"])
  assert f["augment_seed"] == 77 and driver.augment_spec(f).seed == 77
  with pytest.raises(ValueError) as e:
    driver.parse_flags(["--augment=" + FULL])
  assert "--augment" in str(e.value) and "--prefetch" in str(e.value)
  with pytest.raises(ValueError):
    driver.parse_flags(["--prefetch=0", "--augment=flip=0.5"])
  with pytest.raises(ValueError):
    driver.parse_flags(["--prefetch=2", "--augment=blur=1"])
  with pytest.raises(ValueError) as e:                                    # run() checks before it touches data or the GPU
    driver.run(augment="flip=0.5", data="no/such/dataset", root="/nonexistent")
  assert "--augment" in str(e.value) and "--prefetch" in str(e.value)
  with pytest.raises(ValueError):
    driver.run(augment="flip=2", prefetch=2, data="no/such/dataset", root="/nonexistent")


def _declaration(name):
  text = open(os.path.join(ROOT, "include", "lipreading_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
  assert m, "include/lipreading_hip.h does not declare %s" % name
  return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("lr_lip_crop_collate_aug_u8", 17), ("lr_collate_pad_aug_f32", 9)])
def test_entry_points_are_declared_and_bound(name, n_args):
  params = _declaration(name)
  restype, argtypes = _C.SIGNATURES[name]
  assert restype is _C.c_int and len(params) == len(argtypes) == n_args
  for decl, ctype in zip(params, argtypes):
    if "*" in decl or decl.startswith("lr_stream_t"):
      assert ctype is _C.P, decl
    elif decl.startswith("float"):
      assert ctype is _C.c_float, decl
    else:
      assert decl.startswith("int ") and ctype is _C.c_int, decl
  names = [p.split()[-1].lstrip("*") for p in params]
  if name == "lr_lip_crop_collate_aug_u8":
    assert names == ["frames", "lmk", "offsets", "lens", "clip_aug", "tmap", "out", "B", "t_max", "H", "W", "S", "npts",
                     "lo", "hi", "margin", "stream"]
  else:
    assert names == ["packed", "offsets", "lens", "tmap", "out", "B", "t_max", "feat", "stream"]


def test_null_arguments_are_rejected_without_a_device():
  _build.build_library()
  L = _C.lib()
  one = 4096                                        # any non-NULL value: the checks return before a pointer is used
  good = [one] * 7
  tail = (1, 1, 8, 8, 4, 68, 48, 68, 0.3, None)
  assert L.lr_lip_crop_collate_aug_u8(*([None] * 7), *tail) == -1
  for i in range(7):                                # each pointer alone, clip_aug and tmap among them
    args = list(good)
    args[i] = None
    assert L.lr_lip_crop_collate_aug_u8(*args, *tail) == -1, i
  assert L.lr_lip_crop_collate_aug_u8(*good, 0, 1, 8, 8, 4, 68, 48, 68, 0.3, None) == -1      # an empty batch
  assert L.lr_lip_crop_collate_aug_u8(*good, 1, 1, 8, 8, 4, 68, 48, 69, 0.3, None) == -1      # hi > npts
  assert L.lr_lip_crop_collate_aug_u8(*good, 1, 1, 8, 8, 4, 68, 48, 68, -0.1, None) == -1     # a negative margin
  for i in range(5):
    args = [one] * 5
    args[i] = None
    assert L.lr_collate_pad_aug_f32(*args, 1, 1, 4, None) == -1, i
  assert L.lr_collate_pad_aug_f32(*([one] * 5), 1, 0, 4, None) == -1
  assert L.lr_collate_pad_aug_f32(*([one] * 5), 1, 1, 0, None) == -1


# ---- compiled resources ---------------------------------------------------------------------------------------------
def test_augment_kernels_compile_without_scratch_and_leave_the_plain_kernels_alone(tmp_path):
  src = os.path.join(_build.CSRC, "lr_misc.hip")
  res = subprocess.run([_build._hipcc()] + _build._flags(src) +
                       ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o",
                        str(tmp_path / "lr_misc.o")], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-2000:]
  blocks = re.split(r"remark: Function Name: ", res.stderr)[1:]
  mine = [b for b in blocks if "lip_augment_collate_kernel" in b.split()[0]]
  assert len(mine) == 3, [b.split()[0] for b in blocks]                   # 16, 4 and 1 pixels per store
  mine += [b for b in blocks if "collate_pad_aug_kernel" in b.split()[0]]
  assert len(mine) == 4
  for b in mine:
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) + int(re.search(r"SGPRs Spill: (\d+)", b).group(1))
    vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
    occupancy = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
    print(b.split()[0], "VGPRs", vgprs, "occupancy", occupancy, "scratch", scratch)
    assert scratch == 0 and spill == 0 and occupancy >= 8
  # the new template's name does not contain the existing one's: that one still has exactly its three instantiations
  assert len([b for b in blocks if "lip_crop_collate_kernel" in b.split()[0]]) == 3


# ---- the numpy restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,S", [(96, 96, 96), (96, 96, 32), (120, 160, 36), (120, 160, 30), (48, 64, 32)])
def test_numpy_restatement_with_identity_records_is_the_oracles_lip_crop(H, W, S):
  from oracle import torch_oracle
  frames, lm, offsets, lens = AC.ragged_case(5, (H, W), S)
  want = torch_oracle.lip_crop(frames, lm, size=S, margin=0.3)
  clip, tmap = AC.identity_records(lens)
  got = AC.augmented_batch(frames, lm, offsets, lens, clip, tmap, AC.T_MAX, S)
  for b in range(5):
    lo, n = int(offsets[b]), int(lens[b])
    assert got[b, :n].tobytes() == want[lo:lo + n].tobytes()
    assert not got[b, n:].any()
  assert want.any()


def test_numpy_restatement_flips_maps_masks_and_clamps():
  S = 32
  frames, lm, offsets, lens = AC.ragged_case(5, (96, 96), S)
  clip, tmap = AC.identity_records(lens)
  base = AC.augmented_batch(frames, lm, offsets, lens, clip, tmap, AC.T_MAX, S)
  flipped = clip.copy()
  flipped[:, 3] = 1.0
  assert np.array_equal(AC.augmented_batch(frames, lm, offsets, lens, flipped, tmap, AC.T_MAX, S), base[..., ::-1])
  drawn = AugmentSpec(tjitter=0.3, tmask=(2, 3), seed=1).draw(0, range(5), lens)[1]
  drawn[int(offsets[4])] = int(lens[4])                                   # past the sample: clamped to its last frame
  got = AC.augmented_batch(frames, lm, offsets, lens, clip, drawn, AC.T_MAX, S)
  for b in range(5):
    lo, n = int(offsets[b]), int(lens[b])
    for t in range(n):
      m = int(drawn[lo + t])
      assert np.array_equal(got[b, t], base[b, min(m, n - 1)] if m >= 0 else np.zeros_like(base[b, t]))
    assert not got[b, n:].any()


def test_fused_and_plain_arithmetic_of_the_restatement_stay_within_the_gpu_tests_bar():
  """The GPU test's bar (<= 1 LSB, < 1e-3 of the pixels) has to leave room for what the restatement itself does not pin
  down: whether an a + b * c is rounded once or twice.  Uniform noise is the hardest image for that."""
  spec = AugmentSpec(flip=0.5, shift=0.15, zoom=0.25, seed=8)
  for H, W, S in ((96, 96, 96), (96, 96, 32), (120, 160, 36), (120, 160, 30)):
    frames, lm, offsets, lens = AC.ragged_case(5, (H, W), S)
    clip, _ = spec.draw(0, range(5), lens)
    tmap = AC.identity_records(lens)[1]
    a = AC.augmented_batch(frames, lm, offsets, lens, clip, tmap, AC.T_MAX, S, fused=False)
    b = AC.augmented_batch(frames, lm, offsets, lens, clip, tmap, AC.T_MAX, S, fused=True)
    diff = np.abs(a.astype(np.int16) - b.astype(np.int16))
    real = np.concatenate([a[i, :int(n)].reshape(-1) for i, n in enumerate(lens)]).size
    share = float((diff > 0).sum()) / real
    print((H, W, S), "max", int(diff.max()), "share", share)
    assert diff.max() <= 1 and share < 1e-3


@pytest.mark.parametrize("pixels", [False, True])
def test_records_drawn_for_many_batches_at_once_are_the_per_batch_draws(pixels):
  """The workers draw for LD.DRAW_AHEAD batches in one call; a record depends on (seed, pass, index, length) only, so
  every slot holds what a draw for its batch alone gives — across the chunk boundary and in a ragged last chunk."""
  n = 2 * LD.DRAW_AHEAD + 5
  ds = _pixel_samples(n, seed=8) if pixels else _landmark_samples(n, seed=8)
  spec = AugmentSpec.parse(FULL, seed=6)
  stage = LD.HostStage(ds, 1, pixels=pixels, depth=3, workers=4, augment=spec)
  assert len(stage) == n > 2 * LD.DRAW_AHEAD
  for p in range(2):
    seen = 0
    for k, pb in enumerate(stage):
      buf = stage.slots[pb.slot].numpy()
      ln = len(ds[k][0][0]) if pixels else len(ds[k][0])
      clip, tmap = spec.draw(p, [k], [ln])
      assert pb.augmented and np.array_equal(pb.region(buf, "tmap"), tmap), (p, k)
      if pixels:
        assert np.array_equal(pb.region(buf, "aug"), clip), (p, k)
      seen += 1
    assert seen == n


def test_a_malformed_sample_in_an_augmented_pass_raises_at_its_batch_and_not_before():
  ds = _landmark_samples(14, seed=7)
  f, c = ds[9]
  ds[9] = (f[:, :67].copy(), c)                      # (len, 67, 3): batch 2 of batch size 4
  spec = AugmentSpec.parse(FULL, seed=6)
  stage = LD.HostStage(ds, 4, depth=3, workers=2, augment=spec)
  got = []
  with pytest.raises(AssertionError):
    for pb in stage:
      lo, hi = stage.plan[pb.index]
      want = spec.draw(0, range(lo, hi), [len(ds[i][0]) for i in range(lo, hi)])[1]
      assert np.array_equal(pb.region(stage.slots[pb.slot].numpy(), "tmap"), want)
      got.append(pb.index)
  assert got == [0, 1] and stage.threads_alive() == 0
