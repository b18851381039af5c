#!/usr/bin/env python
"""Measure the stabilised crop beside the box crop: the collate launch, and the loop it runs under.

  python tools/bench_crop.py                   # both tables, one JSON document on stdout and profiles/crop_stable.json
  python tools/bench_crop.py --batches 16 --repeats 5

  kernel  lr_lip_crop_collate_aug_u8 beside lr_lip_stable_collate_u8 at radius 0 and 2, on ONE set of records
          (tools/bench_loader.py's same-bytes policy: flip, shift, time jitter), device events, one process, the arms
          alternated after a warm-up; B = 32, T = 75, 96 x 96 frames -> 96 x 96 crops (bench_loader's shape).
  trace   with --trace: each loop arm once more in a fresh child process under `rocprofv3 --kernel-trace` (no counters):
          the collate kernels' durations INSIDE the loop, beside the step's own kernels.
  loop    tools/bench_loader.py's regime X (u8 frames -> mouth crop -> PixelLipReader + CTC, eager, B = 32) fed by
          PrefetchLoader(crop="box") and PrefetchLoader(crop="stable"), the arms alternated epoch by epoch in one
          process: ms per step of train()'s loop, median and min-max.

The synthetic faces give both rules windows of the same size: the eye contours lie 0.38 frame widths apart, rolled by
up to 15 degrees, so that 1.25 eye distances is about the side the box rule takes from the mouth points.

No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import contextlib
import glob
import io
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import bench_loader as BL  # noqa: E402

EXTENT = 1.25


def place_eyes(lmk, hw, rng):
  """Eye contours (36..41, 42..47) 0.38 * hw apart about (0.5, 0.4) * hw, rolled by up to +-15 degrees per clip with
  a little jitter per frame.  lmk [rows][68][3], in place."""
  rows = lmk.shape[0]
  ang = np.deg2rad(rng.uniform(-15, 15)) + rng.uniform(-0.02, 0.02, rows)
  half = 0.19 * hw + rng.uniform(-0.5, 0.5, rows)
  ring = np.stack([np.cos(np.arange(6) * np.pi / 3), 0.5 * np.sin(np.arange(6) * np.pi / 3)], 1) * 0.04 * hw
  for first, sign in ((36, -1.0), (42, 1.0)):
    lmk[:, first:first + 6, 0] = (0.5 * hw + sign * half * np.cos(ang))[:, None] + ring[None, :, 0]
    lmk[:, first:first + 6, 1] = (0.4 * hw + sign * half * np.sin(ang))[:, None] + ring[None, :, 1]
  return lmk


def dataset_with_eyes(n_samples, hw=96):
  rng = np.random.RandomState(99)
  seen = {}
  out = []
  for (frames, lmk), cap in BL.synthetic_dataset("X", n_samples, hw=hw):
    if id(lmk) not in seen:                          # (the pool holds a few distinct samples)
      seen[id(lmk)] = place_eyes(lmk.copy(), hw, rng)
    out.append(((frames, seen[id(lmk)]), cap))
  return out


def time_kernels(dev, batch=32, size=96, hw=96, t_frames=BL.T_FRAMES, reps=10, policy=BL.SAME_BYTES_POLICY):
  """ms of one collate call per arm (device events around the call: the stable arms are two launches)."""
  import torch
  from lipreading_amd import _C
  from lipreading_amd.augment import AugmentSpec
  from lipreading_amd.landmarks import _eyes, _mouth
  L = _C.lib()
  rng = np.random.RandomState(7)
  rows = batch * t_frames
  frames = torch.from_numpy(rng.randint(0, 256, (rows, 3, hw, hw)).astype(np.uint8)).to(dev)
  lm = np.zeros((rows, BL.N_LMK, 3), np.float32)
  lm[:, :, 0] = rng.uniform(0.35, 0.65, (rows, BL.N_LMK)) * hw
  lm[:, :, 1] = rng.uniform(0.6, 0.8, (rows, BL.N_LMK)) * hw
  for b in range(batch):
    place_eyes(lm[b * t_frames:(b + 1) * t_frames], hw, rng)
  lmk = torch.from_numpy(lm).to(dev)
  offsets = torch.arange(batch, dtype=torch.int64, device=dev) * t_frames
  lens = torch.full((batch,), t_frames, dtype=torch.int32, device=dev)
  out = torch.empty((batch, t_frames, 3, size, size), dtype=torch.uint8, device=dev)
  spec = AugmentSpec.parse(policy, seed=123456)
  clip, tmap = spec.draw(0, np.arange(batch), np.full(batch, t_frames))
  clip_d, tmap_d = torch.from_numpy(clip).to(dev), torch.from_numpy(tmap).to(dev)
  need = L.lr_lip_stable_workspace_bytes(rows, 2)
  work = torch.empty(need, dtype=torch.uint8, device=dev)
  stream = torch.cuda.current_stream(dev)
  ea, eb = _eyes

  def box():
    _C.check(L.lr_lip_crop_collate_aug_u8(frames.data_ptr(), lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(),
                                          clip_d.data_ptr(), tmap_d.data_ptr(), out.data_ptr(), batch, t_frames, hw, hw,
                                          size, BL.N_LMK, _mouth.start, _mouth.stop, 0.3, stream.cuda_stream),
             "lr_lip_crop_collate_aug_u8")

  def stable(radius):
    def call():
      _C.check(L.lr_lip_stable_collate_u8(frames.data_ptr(), lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(),
                                          clip_d.data_ptr(), tmap_d.data_ptr(), out.data_ptr(), None, work.data_ptr(),
                                          need, batch, rows, t_frames, hw, hw, size, BL.N_LMK, _mouth.start, _mouth.stop,
                                          ea.start, ea.stop, eb.start, eb.stop, EXTENT, radius, stream.cuda_stream),
               "lr_lip_stable_collate_u8")
    return call

  arms = (("box_aug_ms", box), ("stable_radius0_ms", stable(0)), ("stable_radius2_ms", stable(2)))
  for _, fn in arms:
    BL._event_ms(fn, stream, 3)
  ms = {name: [] for name, _ in arms}
  for _ in range(reps):                              # alternated
    for name, fn in arms:
      ms[name] += BL._event_ms(fn, stream, 1)
  res = {name: BL._summary(v) for name, v in ms.items()}
  res.update(shape=[batch, t_frames, 3, size, size], source_hw=[hw, hw], policy=str(spec), extent=EXTENT,
             bytes_written_plus_read=int(out.numel() + frames.numel()), masked_frames=int((tmap < 0).sum()))
  return res


def time_loop(dev, batch=32, n_batches=32, repeats=5, size=96, hw=96, depth=2, workers=2, radius=2, log=None,
              own_streams=False, stable_first=False):
  """ms per step of train()'s loop over PrefetchLoader(crop="box") and PrefetchLoader(crop="stable"), alternated.
  Both loaders enqueue on ONE copy stream (they never run at the same time): a process has a few hardware queues, and
  which of them the second loader's own stream lands on — alone, or behind the step's stream — would otherwise be
  part of what is compared.  own_streams=True keeps a stream per loader (to see just that); stable_first constructs
  the stabilised loader first."""
  import torch
  from lipreading_amd import train as T
  from lipreading_amd.loader import PrefetchLoader
  ds = dataset_with_eyes(batch * n_batches, hw=hw)
  model, opt, c2i = BL.build_model("X", dev, size=size)
  graphs = T.StepGraphs(enabled=False)               # regime X runs eager, as in bench_loader
  common = dict(pixels=True, size=size, depth=depth, workers=workers)
  make = {"prefetch_box": lambda: PrefetchLoader(ds, batch, dev, **common),
          "prefetch_stable": lambda: PrefetchLoader(ds, batch, dev, crop="stable", extent=EXTENT, radius=radius, **common)}
  built = {name: make[name]() for name in (sorted(make, reverse=stable_first))}
  arms = tuple((name, built[name]) for name in ("prefetch_box", "prefetch_stable"))
  if not own_streams:
    first = built[sorted(make, reverse=stable_first)[0]]
    for loader in built.values():
      loader._copy = first._copy

  host_s = {}

  class Timed(object):
    """The loader as train() sees it, with the host time spent inside its __next__ added up (bench_loader's)."""
    def __init__(self, name, loader):
      self.name, self.loader = name, loader
    def __len__(self):
      return len(self.loader)
    def close(self):
      self.loader.close()
    def __iter__(self):
      it = iter(self.loader)
      while True:
        t0 = time.perf_counter()
        try:
          item = next(it)
        except StopIteration:
          return
        finally:
          host_s[self.name] = host_s.get(self.name, 0.0) + time.perf_counter() - t0
        yield item

  def epoch(loader):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
      T.train(model, None, loader, opt, dev, c2i, grad_norm=50, graphs=graphs)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / n_batches

  arms = tuple((name, Timed(name, loader)) for name, loader in arms)
  for _, loader in arms:                             # warm-up: allocator, pinned ring
    epoch(loader)
    epoch(loader)
  host_s.clear()
  ms = {name: [] for name, _ in arms}
  for r in range(repeats):
    for name, loader in arms:
      ms[name].append(epoch(loader))
    if log:
      log("  repeat %d: " % r + ", ".join("%s %.3f" % (n, ms[n][-1]) for n, _ in arms))
  for _, loader in arms:
    loader.close()
  out = {name: BL._summary(v) for name, v in ms.items()}
  box, new = out["prefetch_box"], out["prefetch_stable"]
  out["stable_minus_box_median_ms"] = new["median"] - box["median"]
  out["box_spread_ms"] = box["max"] - box["min"]
  out["within_box_spread"] = bool(abs(new["median"] - box["median"]) <= box["max"] - box["min"])
  out["host_ms_in_loader_per_step"] = {n: host_s.get(n, 0.0) * 1e3 / (repeats * n_batches) for n in ms}
  out.update(steps_per_epoch=n_batches, batch=batch, radius=radius, extent=EXTENT, one_copy_stream=not own_streams,
             constructed_first="stable" if stable_first else "box")
  return out


# ---- what the kernels cost inside the loop: one run per arm under rocprofv3 ------------------------------------------
TRACE_STEPS, TRACE_EPOCHS = 16, 3
COLLATE_NAMES = ("lip_crop_collate_kernel", "lip_augment_collate_kernel", "stable_pose_kernel", "stable_window_kernel")


def trace_child(args):
  """The traced program: a short prefetched loop of regime X over one crop (nothing is timed here)."""
  import torch
  dev = torch.device("cuda:0")
  from lipreading_amd import train as T
  from lipreading_amd.loader import PrefetchLoader
  ds = dataset_with_eyes(args.batch * TRACE_STEPS)
  model, opt, c2i = BL.build_model("X", dev, size=args.size)
  stable = dict(crop="stable", extent=EXTENT, radius=2) if args.trace_child == "stable" else {}
  loader = PrefetchLoader(ds, args.batch, dev, pixels=True, size=args.size, depth=args.depth, workers=args.workers,
                          **stable)
  with contextlib.redirect_stdout(io.StringIO()):
    for _ in range(TRACE_EPOCHS):
      T.train(model, None, loader, opt, dev, c2i, grad_norm=50, graphs=T.StepGraphs(enabled=False))
  torch.cuda.synchronize(dev)
  loader.close()


def summarise_trace(directory):
  """Per collate kernel: calls and median / max microseconds inside the loop; the step's other kernels: their summed
  microseconds per step over the last epoch (the first holds the one-off initialisation)."""
  files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
  if not files:
    return {"error": "trace files missing", "found": sorted(os.listdir(directory))}
  rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Kernel_Name", "")) for r in BL._rows(files[0])]
  rows.sort()
  out = {"kernels": len(rows), "collate": {}}
  marks = [s for s, _, n in rows if any(c in n for c in COLLATE_NAMES[:2] + COLLATE_NAMES[3:])]   # one per batch
  for c in COLLATE_NAMES:
    us = [(e - s) / 1e3 for s, e, n in rows if c in n]
    if us:
      out["collate"][c] = {"calls": len(us), "median_us": statistics.median(us), "max_us": max(us)}
  if len(marks) >= TRACE_STEPS:
    t0 = marks[-TRACE_STEPS]                         # from the last epoch's first collate to the end of the trace
    rest = [(s, e) for s, e, n in rows if s >= t0 and not any(c in n for c in COLLATE_NAMES)]
    out["other_kernels_us_per_step_last_epoch"] = sum(e - s for s, e in rest) / 1e3 / TRACE_STEPS
    out["other_kernels_per_step_last_epoch"] = len(rest) / TRACE_STEPS
    out["span_us_per_step_last_epoch"] = (max(e for _, e in rest) - t0) / 1e3 / TRACE_STEPS if rest else None
  return out


def run_trace(args, arm):
  prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
  if not os.path.exists(prof):
    return {"error": "rocprofv3 not found"}
  tmp = tempfile.mkdtemp(prefix="crop_trace_")
  try:
    cmd = [prof, "--kernel-trace", "-f", "csv", "-d", tmp, "-o", "crop", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child", arm, "--batch", str(args.batch), "--size", str(args.size),
           "--depth", str(args.depth), "--workers", str(args.workers)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.trace_timeout)
    if res.returncode != 0:
      return {"error": "traced run exited %d" % res.returncode, "stderr": res.stderr[-1500:]}
    return summarise_trace(tmp)
  except subprocess.TimeoutExpired:
    return {"error": "traced run exceeded %d s" % args.trace_timeout}
  finally:
    shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--batches", type=int, default=32, help="steps per epoch of the loop arms")
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--reps", type=int, default=10, help="timed calls per kernel arm")
  ap.add_argument("--size", type=int, default=96)
  ap.add_argument("--depth", type=int, default=2)
  ap.add_argument("--workers", type=int, default=2)
  ap.add_argument("--no-loop", action="store_true", help="the kernel table only")
  ap.add_argument("--own-streams", action="store_true", help="a copy stream per loader, as each makes for itself")
  ap.add_argument("--stable-first", action="store_true", help="construct the stabilised loader before the box one")
  ap.add_argument("--trace", action="store_true", help="one more run per loop arm under rocprofv3 --kernel-trace")
  ap.add_argument("--trace-timeout", type=int, default=240)
  ap.add_argument("--trace-child", default="", help=argparse.SUPPRESS)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_stable.json"))
  args = ap.parse_args(argv)
  assert args.repeats >= 5 and args.reps >= 5, "at least five repeats per arm"
  import torch
  if not torch.cuda.is_available():
    print("bench_crop: no GPU — this tool measures the MI355X and has no fallback", file=sys.stderr)
    return 2
  from lipreading_amd import _build
  _build.build_library()
  if args.trace_child:
    trace_child(args)
    return 0
  dev = torch.device("cuda:0")
  log = lambda s: print(s, file=sys.stderr, flush=True)
  doc = {"tool": "tools/bench_crop.py", "device": torch.cuda.get_device_name(0),
         "kernel": time_kernels(dev, batch=args.batch, size=args.size, reps=args.reps)}
  log("kernel: " + json.dumps(doc["kernel"], sort_keys=True))
  if not args.no_loop:
    doc["loop"] = time_loop(dev, batch=args.batch, n_batches=args.batches, repeats=args.repeats, size=args.size,
                            depth=args.depth, workers=args.workers, log=log, own_streams=args.own_streams,
                            stable_first=args.stable_first)
  if args.trace:
    doc["trace"] = {}
    for arm in ("box", "stable"):
      log("tracing the %s arm under rocprofv3" % arm)
      doc["trace"][arm] = run_trace(args, arm)
      log("  " + json.dumps(doc["trace"][arm], sort_keys=True))
  text = json.dumps(doc, indent=1, sort_keys=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(text + "\n")
  print(text)
  return 0


if __name__ == "__main__":
  sys.exit(main())
