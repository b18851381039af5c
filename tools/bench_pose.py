#!/usr/bin/env python
"""Measure the landmark pose normalisation against what it replaces, in the same run on the same box.

  python tools/bench_pose.py                   # one JSON document on stdout and profiles/pose_collate.json
  python tools/bench_pose.py --batches 256 --repeats 5

  kernel  lr_collate_pad_f32 beside lr_lmk_pose_collate_f32 with radius 0 and radius 2 (similarity), B = 32, T = 75,
          68 points, the three arms alternated, device events around each call
  loop    regime R of tools/bench_loader.py (landmarks -> BiGRU-256 + CTC, B = 32, hipGraphs on): train()'s loop fed by
          PrefetchLoader without and with pose=PoseSpec(radius 2), the arms alternated; ms per step, medians and
          min-max, and the spread of the plain arm, which is the yardstick for the other

No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import bench_loader as BL  # noqa: E402


def face_template():
  """A face-like (68, 3) template in the pixels range (bench data, not a fitted face)."""
  rng = np.random.RandomState(68)
  t = np.stack([rng.uniform(30, 170, 68), rng.uniform(40, 190, 68), rng.uniform(-20, 20, 68)], axis=1)
  t[27:31] = [[100, 70, 10], [100, 80, 16], [100, 90, 22], [100, 100, 30]]
  t[33] = [100, 110, 18]
  t[36], t[39], t[42], t[45] = [55, 70, -5], [82, 72, 2], [118, 72, 2], [145, 70, -5]
  return t.astype(np.float32)


def moving_faces(n_clips, t_frames, seed=1):
  """(t_frames, 68, 3) float64 clips: the template under a slowly turning, drifting head plus landmark noise."""
  rng = np.random.RandomState(seed)
  tm = face_template().astype(np.float64)
  c = tm.mean(axis=0)
  out = []
  for _ in range(n_clips):
    yaw = np.cumsum(rng.randn(t_frames) * 0.01) + rng.uniform(-0.3, 0.3)
    shift = np.cumsum(rng.randn(t_frames, 3), axis=0)
    clip = np.empty((t_frames, 68, 3))
    for i in range(t_frames):
      cy, sy = np.cos(yaw[i]), np.sin(yaw[i])
      R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
      clip[i] = (tm - c + rng.randn(68, 3) * 0.5) @ R.T + c + shift[i]
    out.append(clip)
  return out


def time_kernels(dev, batch=32, t_frames=BL.T_FRAMES, reps=20):
  import torch
  from lipreading_amd import _C
  from lipreading_amd.landmarks import PoseSpec
  L = _C.lib()
  rows = batch * t_frames
  clips = moving_faces(batch, t_frames)
  lmk = torch.from_numpy(np.concatenate(clips).astype(np.float32)).to(dev)
  offsets = torch.arange(batch, dtype=torch.int64, device=dev) * t_frames
  lens = torch.full((batch,), t_frames, dtype=torch.int32, device=dev)
  out = torch.empty((batch, t_frames, 68 * 3), dtype=torch.float32, device=dev)
  stream = torch.cuda.current_stream(dev)
  specs = {r: PoseSpec(face_template(), radius=r, scale=True) for r in (0, 2)}
  work = torch.empty(specs[2].workspace_bytes(rows), dtype=torch.uint8, device=dev)

  def pad():
    _C.check(L.lr_collate_pad_f32(lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(), out.data_ptr(), batch, t_frames,
                                  68 * 3, stream.cuda_stream), "lr_collate_pad_f32")

  status = torch.empty((rows,), dtype=torch.int32, device=dev)

  def pose(r):
    s = specs[r]
    tmpl = s.template_on(dev)
    return lambda: _C.check(L.lr_lmk_pose_collate_f32(
        lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(), None, tmpl.data_ptr(), s.rigid_ptr, len(s.rigid),
        out.data_ptr(), None, status.data_ptr(), work.data_ptr(), work.numel(), batch, rows, t_frames, 68, s.radius,
        s.flags, stream.cuda_stream), "lr_lmk_pose_collate_f32")

  arms = (("pad", pad), ("pose_radius0", pose(0)), ("pose_radius2", pose(2)))
  for _, fn in arms:
    BL._event_ms(fn, stream, 3)
  ms = {name: [] for name, _ in arms}
  for _ in range(reps):                       # alternated
    for name, fn in arms:
      ms[name] += BL._event_ms(fn, stream, 1)
  res = {name + "_ms": BL._summary(v) for name, v in ms.items()}
  res["shape"] = [batch, t_frames, 68, 3]
  res["bytes_written_plus_read"] = int(2 * rows * 68 * 3 * 4)
  return res


def time_loop(dev, batch=32, n_batches=256, repeats=5, depth=2, workers=2, log=None):
  import torch
  from lipreading_amd import train as T
  from lipreading_amd.landmarks import PoseSpec
  from lipreading_amd.loader import PrefetchLoader
  pool = moving_faces(8, BL.T_FRAMES)
  caps = BL.synthetic_dataset("R", 8)
  ds = [(pool[i % 8], caps[i % 8][1]) for i in range(batch * n_batches)]
  model, opt, c2i = BL.build_model("R", dev)
  graphs = T.StepGraphs(enabled=True)
  spec = PoseSpec(face_template(), radius=2, scale=True)
  arms = (("plain", PrefetchLoader(ds, batch, dev, depth=depth, workers=workers)),
          ("pose", PrefetchLoader(ds, batch, dev, depth=depth, workers=workers, pose=spec)))

  def epoch(loader):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
      T.train(model, None, loader, opt, dev, c2i, grad_norm=50, graphs=graphs)
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / n_batches

  for _, loader in arms:
    epoch(loader)
    epoch(loader)
  ms = {name: [] for name, _ in arms}
  for r in range(repeats):
    for name, loader in arms:
      ms[name].append(epoch(loader))
    if log:
      log("  repeat %d: " % r + ", ".join("%s %.4f" % (n, ms[n][-1]) for n, _ in arms))
  for _, loader in arms:
    loader.close()
  out = {name + "_ms_per_step": BL._summary(v) for name, v in ms.items()}
  out["steps_per_epoch"], out["batch"] = n_batches, batch
  out["plain_spread_ms"] = max(ms["plain"]) - min(ms["plain"])
  out["pose_minus_plain_median_ms"] = out["pose_ms_per_step"]["median"] - out["plain_ms_per_step"]["median"]
  return out


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--batches", type=int, default=512, help="steps per epoch of the loop")
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_collate.json"))
  args = ap.parse_args(argv)
  assert args.repeats >= 5, "at least five repeats per arm"
  import torch
  if not torch.cuda.is_available():
    print("bench_pose: no GPU — this tool measures the MI355X and has no fallback", file=sys.stderr)
    return 2
  from lipreading_amd import _build
  _build.build_library()
  dev = torch.device("cuda:0")
  log = lambda s: print(s, file=sys.stderr, flush=True)
  doc = {"tool": "tools/bench_pose.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
         "kernel": time_kernels(dev, batch=args.batch),
         "loop": time_loop(dev, batch=args.batch, n_batches=args.batches, repeats=args.repeats, log=log)}
  text = json.dumps(doc, indent=1, sort_keys=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(text + "\n")
  print(text)
  return 0


if __name__ == "__main__":
  sys.exit(main())
