"""CPU: the host stage of lipreading_amd.loader (batch plan, ragged packing into a slot, chars padding, error
hand-over, shutdown) and the declaration of lr_lip_crop_collate_u8.  The device stage is tests/test_gpu_loader.py."""
import gc
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import torch

from lipreading_amd import _build, _C
from lipreading_amd import dataset as DS
from lipreading_amd import loader as LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _loader_threads():
  return [t for t in threading.enumerate() if t.name.startswith("lipreading-prefetch") and t.is_alive()]


def _expected_chars(captions):
  """data.make_collate_fn's host half, line for line (data.py: caps / tgt_lens / tgt)."""
  caps = [np.asarray(c, dtype=np.int64) for c in captions]
  tgt_lens = torch.tensor([len(c) for c in caps], dtype=torch.long)
  tgt = torch.zeros((len(caps), int(tgt_lens.max())), dtype=torch.long)
  for i, c in enumerate(caps):
    tgt[i, :len(c)] = torch.from_numpy(c)
  return tgt, tgt_lens


@pytest.mark.parametrize("batch_size", [1, 4, 32])
def test_batch_plan_equals_batch_loaders(batch_size):
  for n in range(1, 71):
    items = list(range(n))
    seen = []
    plain = DS.BatchLoader(items, batch_size, lambda batch: seen.append(list(batch)))
    for _ in plain:
      pass
    plan = LD.batch_plan(n, batch_size)
    assert [list(range(lo, hi)) for lo, hi in plan] == seen
    assert len(plan) == len(plain)
  ds = _landmark_samples(70, seed=3)
  stage = LD.HostStage(ds, batch_size, depth=2, workers=2)
  assert len(stage) == len(DS.BatchLoader(ds, batch_size, None)) and stage.plan == LD.batch_plan(70, batch_size)


@pytest.mark.parametrize("pixels", [False, True])
def test_host_packing_equals_concatenate(pixels):
  ds = _pixel_samples(23, seed=5) if pixels else _landmark_samples(23, seed=5)
  B = 4
  stage = LD.HostStage(ds, B, pixels=pixels, depth=2, workers=2)
  assert len(stage.slots) == 3 and all(not s.is_cuda for s in stage.slots)
  n_seen = 0
  for k, pb in enumerate(stage):
    lo, hi = stage.plan[k]
    batch = [ds[i] for i in range(lo, hi)]
    buf = stage.slots[pb.slot].numpy()
    assert (pb.index, pb.B) == (k, hi - lo) and pb.nbytes <= stage.slot_bytes
    if pixels:
      want_f = np.concatenate([s[0][0] for s in batch], axis=0)
      want_l = np.concatenate([np.asarray(s[0][1], dtype=np.float32) for s in batch], axis=0)
      got_l = pb.region(buf, "lmk")
      assert got_l.dtype == np.float32 and got_l.tobytes() == want_l.tobytes()
      lens = [len(s[0][0]) for s in batch]
      assert (pb.H, pb.W) == (12, 16)
    else:
      want_f = np.concatenate([np.asarray(s[0], dtype=np.float32).reshape(len(s[0]), 204) for s in batch], axis=0)
      lens = [len(s[0]) for s in batch]
      assert pb.tail == (68, 3) and pb.feat == 204
    got_f = pb.region(buf, "frames")
    assert got_f.dtype == want_f.dtype and got_f.shape == want_f.shape and got_f.tobytes() == want_f.tobytes()
    assert pb.region(buf, "lens").dtype == np.int32 and list(pb.region(buf, "lens")) == lens
    assert pb.region(buf, "offsets").dtype == np.int64
    assert list(pb.region(buf, "offsets")) == [int(sum(lens[:b])) for b in range(len(lens))]
    assert pb.t_max == max(lens) and pb.rows == sum(lens)
    for name in ("frames_off", "lmk_off", "offsets_off", "lens_off"):
      assert getattr(pb, name) % 16 == 0          # the kernels read int64 offsets and the upload is one range
    tgt, tgt_lens = _expected_chars([s[1] for s in batch])
    assert pb.chars.dtype == np.int64 and torch.equal(torch.from_numpy(pb.chars), tgt)
    assert pb.char_lens.dtype == np.int64 and torch.equal(torch.from_numpy(pb.char_lens), tgt_lens)
    assert pb.frame_lens.dtype == np.int64 and list(pb.frame_lens) == lens
    n_seen += 1
  assert n_seen == len(stage) == 6
  assert not _loader_threads()


@pytest.mark.parametrize("pixels", [False, True])
def test_a_malformed_sample_raises_at_its_batch_and_not_before(pixels):
  ds = _pixel_samples(14, seed=7) if pixels else _landmark_samples(14, seed=7)
  bad = 9                                           # batch 2 of batch size 4
  if pixels:
    (f, l), c = ds[bad]
    ds[bad] = ((f[:, :, :, :-1].copy(), l), c)      # (len, 3, H, W-1)
  else:
    f, c = ds[bad]
    ds[bad] = (f[:, :67].copy(), c)                 # (len, 67, 3)
  stage = LD.HostStage(ds, 4, pixels=pixels, depth=3, workers=2)   # deep enough to pack the bad batch early
  got = []
  with pytest.raises(AssertionError):
    for pb in stage:
      got.append(pb.index)
  assert got == [0, 1]
  assert not _loader_threads() and stage.threads_alive() == 0


def test_abandoned_pass_then_a_full_one_and_no_thread_outlives_the_loader():
  ds = _landmark_samples(19, seed=9)
  stage = LD.HostStage(ds, 4, depth=2, workers=3)
  for pb in stage:
    assert pb.index == 0
    break
  gc.collect()
  assert not _loader_threads()
  it = iter(stage)                                  # abandoned without a break: the next iter() shuts it down
  assert next(it).index == 0 and len(_loader_threads()) == 3
  assert [pb.index for pb in stage] == list(range(5))
  seen = []
  for k, pb in enumerate(stage):                    # and the pass is a full, correct one
    lo, hi = stage.plan[k]
    want = np.concatenate([np.asarray(ds[i][0], dtype=np.float32).reshape(-1, 204) for i in range(lo, hi)])
    assert pb.region(stage.slots[pb.slot].numpy(), "frames").tobytes() == want.tobytes()
    seen.append(pb.index)
  assert seen == list(range(5))
  it2 = iter(stage)
  next(it2)
  assert len(_loader_threads()) == 3
  del it, it2, stage, pb
  gc.collect()
  assert not _loader_threads()


def test_workers_are_capped_and_never_sized_by_the_machine():
  stage = LD.HostStage(_landmark_samples(5), 2, workers=64)
  assert stage.workers == LD.MAX_WORKERS == 8
  assert LD.HostStage(_landmark_samples(5), 2).workers == 2


def test_a_non_cuda_device_raises():
  ds = _landmark_samples(5)
  with pytest.raises(_C.LipReadingHipError):
    LD.PrefetchLoader(ds, 2, "cpu")
  with pytest.raises(_C.LipReadingHipError):
    DS.make_loader(ds, 2, None, prefetch=2, device=torch.device("cpu"))
  plain = DS.make_loader(ds, 2, lambda b: b)        # prefetch=0 is today's loader
  assert isinstance(plain, DS.BatchLoader) and len(plain) == 3
  assert not _loader_threads()


def test_driver_flag_defaults_to_the_plain_loader():
  from lipreading_amd import driver
  assert driver.DEFAULTS["prefetch"] == 0
  assert driver.parse_flags(["--prefetch=2"])["prefetch"] == 2


def test_collate_kernel_is_declared_bound_and_compiles_without_scratch(tmp_path):
  text = open(os.path.join(ROOT, "include", "lipreading_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  m = re.search(r"\bint\s+lr_lip_crop_collate_u8\s*\(([^)]*)\)\s*;", text)
  assert m, "include/lipreading_hip.h does not declare lr_lip_crop_collate_u8"
  params = [p.strip() for p in m.group(1).split(",")]
  restype, argtypes = _C.SIGNATURES["lr_lip_crop_collate_u8"]
  assert len(params) == len(argtypes) == 15
  # pointers, ints and the float sit where the header puts them
  for decl, ctype in zip(params, argtypes):
    if "*" in decl or decl.startswith("lr_stream_t"):
      assert ctype is _C.P, decl
    elif decl.startswith("float"):
      assert ctype is _C.c_float, decl
    else:
      assert decl.startswith("int ") and ctype is _C.c_int, decl
  _build.build_library()
  assert hasattr(_C.lib(), "lr_lip_crop_collate_u8")
  # NULL arguments and an empty batch are rejected before any launch (no device needed)
  assert _C.lib().lr_lip_crop_collate_u8(None, None, None, None, None, 1, 1, 8, 8, 4, 68, 48, 68, 0.3, None) == -1
  # the new kernel keeps its registers: no scratch in any of its instantiations
  src = os.path.join(_build.CSRC, "lr_misc.hip")
  res = subprocess.run([_build._hipcc()] + _build._flags(src) +
                       ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o",
                        str(tmp_path / "lr_misc.o")], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-2000:]
  blocks = re.split(r"remark: Function Name: ", res.stderr)[1:]
  mine = [b for b in blocks if "lip_crop_collate_kernel" in b.split()[0]]
  assert len(mine) == 3, [b.split()[0] for b in blocks]
  for b in mine:
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    spill = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
    vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
    occupancy = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
    print(b.split()[0], "VGPRs", vgprs, "occupancy", occupancy, "scratch", scratch)
    assert scratch == 0 and spill == 0 and occupancy >= 8
