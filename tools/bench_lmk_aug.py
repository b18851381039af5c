#!/usr/bin/env python
"""Measure the landmark-space augmentation against the collate it follows, in the same run on the same box.

  python tools/bench_lmk_aug.py                   # one JSON document on stdout and profiles/lmk_augment.json
  python tools/bench_lmk_aug.py --batches 256 --repeats 5

  kernel  B = 32, T = 75, 68 points, device events around each arm, the arms alternated, medians with min-max:
          lr_collate_pad_f32 (the yardstick); lr_collate_pad_f32 + lr_lmk_augment_f32; lr_lmk_pose_collate_f32;
          lr_lmk_pose_collate_f32 + lr_lmk_augment_f32; and lr_lmk_augment_f32 alone (in place) with the identity
          record and with a full record, without and with jitter
  loop    regime R of tools/bench_loader.py (landmarks -> BiGRU-256 + CTC, B = 32, hipGraphs on): train()'s loop fed by
          PrefetchLoader without and with lmk_augment=, the arms alternated; ms per step, medians and min-max, and the
          spread of the plain arm, which is the yardstick for the other

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
import bench_pose as BP  # noqa: E402

FULL = "mirror=0.5,rot=10/10/15,scale=0.1,stretch=0.05,shift=0.05"


def time_kernels(dev, batch=32, t_frames=BL.T_FRAMES, reps=20):
  import torch
  from lipreading_amd import _C
  from lipreading_amd.augment import LandmarkAugmentSpec
  from lipreading_amd.landmarks import MIRROR_68, PoseSpec, mirror_perm_on
  L = _C.lib()
  rows = batch * t_frames
  lmk = torch.from_numpy(np.concatenate(BP.moving_faces(batch, t_frames)).astype(np.float32)).to(dev)
  offsets = torch.arange(batch, dtype=torch.int64, device=dev) * t_frames
  lens = torch.full((batch,), t_frames, dtype=torch.int32, device=dev)
  out = torch.empty((batch, t_frames, 68 * 3), dtype=torch.float32, device=dev)
  stream = torch.cuda.current_stream(dev)
  spec = PoseSpec(BP.face_template(), radius=2, scale=True)
  tmpl = spec.template_on(dev)
  pose_work = torch.empty(spec.workspace_bytes(rows), dtype=torch.uint8, device=dev)
  status = torch.empty((rows,), dtype=torch.int32, device=dev)
  perm = mirror_perm_on(MIRROR_68, dev)
  work = torch.empty(L.lr_lmk_augment_workspace_bytes(batch), dtype=torch.uint8, device=dev)
  host_lens = np.full(batch, t_frames)
  policies = (("identity", LandmarkAugmentSpec()), ("full", LandmarkAugmentSpec.parse(FULL, seed=1)),
              ("full_jitter", LandmarkAugmentSpec.parse(FULL + ",jitter=0.01", seed=1)))
  recs = {name: torch.from_numpy(p.draw(0, range(batch), host_lens).view(np.int64)).to(dev) for name, p in policies}

  def pad():
    _C.check(L.lr_collate_pad_f32(lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(), out.data_ptr(), batch, t_frames,
                                  68 * 3, stream.cuda_stream), "lr_collate_pad_f32")

  def pose():
    _C.check(L.lr_lmk_pose_collate_f32(
        lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(), None, tmpl.data_ptr(), spec.rigid_ptr, len(spec.rigid),
        out.data_ptr(), None, status.data_ptr(), pose_work.data_ptr(), pose_work.numel(), batch, rows, t_frames, 68,
        spec.radius, spec.flags, stream.cuda_stream), "lr_lmk_pose_collate_f32")

  def augment(name):
    rec = recs[name]
    return lambda: _C.check(L.lr_lmk_augment_f32(out.data_ptr(), lens.data_ptr(), rec.data_ptr(), perm.data_ptr(),
                                                 out.data_ptr(), None, work.data_ptr(), work.numel(), batch, t_frames,
                                                 68, stream.cuda_stream), "lr_lmk_augment_f32")

  def both(first, second):
    def run():
      first()
      second()
    return run

  # (an augment-alone arm works in place on the batch the arm before it left in `out`; "pad_again" resets that batch)
  arms = (("pad", pad), ("pad_augment", both(pad, augment("full_jitter"))), ("pose", pose),
          ("pose_augment", both(pose, augment("full_jitter"))), ("pad_again", pad),
          ("augment_identity", augment("identity")), ("augment_full", augment("full")),
          ("augment_full_jitter", augment("full_jitter")))
  for _, fn in arms:
    BL._event_ms(fn, stream, 3)
  ms = {name: [] for name, _ in arms}
  for _ in range(reps):                       # alternated
    for name, fn in arms:
      ms[name] += BL._event_ms(fn, stream, 1)
  res = {name + "_ms": BL._summary(v) for name, v in ms.items() if name != "pad_again"}
  res["shape"] = [batch, t_frames, 68, 3]
  res["batch_bytes"] = int(rows * 68 * 3 * 4)
  res["pad_augment_over_pad"] = res["pad_augment_ms"]["median"] / res["pad_ms"]["median"]
  res["pose_augment_over_pose"] = res["pose_augment_ms"]["median"] / res["pose_ms"]["median"]
  return res


def time_loop(dev, batch=32, n_batches=256, repeats=5, depth=2, workers=2, log=None):
  import torch
  from lipreading_amd import train as T
  from lipreading_amd.augment import LandmarkAugmentSpec
  from lipreading_amd.loader import PrefetchLoader
  pool = BP.moving_faces(8, BL.T_FRAMES)
  caps = BL.synthetic_dataset("R", 8)
  ds = [(pool[i % 8], caps[i % 8][1]) for i in range(batch * n_batches)]
  model, opt, c2i = BL.build_model("R", dev)
  graphs = T.StepGraphs(enabled=True)
  spec = LandmarkAugmentSpec.parse(FULL + ",jitter=0.01", seed=1)
  arms = (("plain", PrefetchLoader(ds, batch, dev, depth=depth, workers=workers)),
          ("lmk_augment", PrefetchLoader(ds, batch, dev, depth=depth, workers=workers, lmk_augment=spec)))

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
  out["lmk_augment_minus_plain_median_ms"] = (out["lmk_augment_ms_per_step"]["median"]
                                              - out["plain_ms_per_step"]["median"])
  return out


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--batches", type=int, default=512, help="steps per epoch of the loop")
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmk_augment.json"))
  args = ap.parse_args(argv)
  assert args.repeats >= 5, "at least five repeats per arm"
  import torch
  if not torch.cuda.is_available():
    print("bench_lmk_aug: no GPU — this tool measures the MI355X and has no fallback", file=sys.stderr)
    return 2
  from lipreading_amd import _build
  _build.build_library()
  dev = torch.device("cuda:0")
  log = lambda s: print(s, file=sys.stderr, flush=True)
  doc = {"tool": "tools/bench_lmk_aug.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
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
