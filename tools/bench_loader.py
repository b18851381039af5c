#!/usr/bin/env python
"""Measure the LOOP, not just the step: train()'s ctc_step loop fed by (a) the plain BatchLoader, (b) PrefetchLoader,
(c) one resident batch repeated (what bench.py times).  bench.py stays as it is; this tool is the loader's yardstick.

  python tools/bench_loader.py                 # regimes R and X, one JSON document on stdout and profiles/loader_loop.json
  python tools/bench_loader.py --regimes X --batches 6 --repeats 5 --no-trace
  python tools/bench_loader.py --augment flip=0.5,shift=0.08,zoom=0.1,tjitter=0.05,tmask=2x10
                                               # the augmented loader beside the prefetched one: profiles/augment_loop.json

  R  landmarks -> BiGRU-256 + CTC, B = 32, hipGraphs on (as the driver has them)
  X  u8 frames 96x96 + landmarks -> mouth crop -> PixelLipReader (conv3d frontend, 2 x BiGRU-256) + CTC, B = 32, eager

Protocol: an in-memory synthetic dataset of fixed-length T = 75 clips; one warm-up epoch per arm, then `repeats` timed
epochs per arm with the arms alternated; the host clock around train() plus a device synchronise; medians and min-max.
Beside the loop: host-to-device GB/s of a slot upload (pinned and pageable), the time of lr_lip_crop_collate_u8 next to
the summed B per-sample lr_lip_crop_u8 launches it replaces (device events), and — unless --no-trace — one extra run of
regime X's prefetched loop under `rocprofv3 --kernel-trace --memory-copy-trace` (a fresh child process; no counters in
that run), summarised as copy time inside / outside kernel intervals.

No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import contextlib
import csv
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
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T_FRAMES, N_LMK, VOCAB, LABEL_LEN = 75, 68, 64, 30
SAME_BYTES_POLICY = "flip=0.5,shift=0.08,tjitter=0.05"     # augments, yet gathers and stores what the plain launch does


def synthetic_dataset(regime, n_samples, hw=96, t_frames=T_FRAMES, seed=123456, distinct=8):
  """`n_samples` samples of `t_frames` frames each, in FrameCaptionDataset's item format.  Only `distinct` different
  arrays exist (the loaders copy every sample of every batch regardless), so a long epoch fits in memory."""
  rng = np.random.RandomState(seed)
  pool = []
  for _ in range(min(distinct, n_samples)):
    cap = np.array([1] + list(rng.randint(4, VOCAB, LABEL_LEN)) + [2])
    if regime == "X":
      frames = rng.randint(0, 256, (t_frames, 3, hw, hw)).astype(np.uint8)
      lmk = np.zeros((t_frames, N_LMK, 3), np.float64)
      lmk[:, :, 0] = rng.uniform(0.2, 0.8, (t_frames, N_LMK)) * hw
      lmk[:, :, 1] = rng.uniform(0.2, 0.8, (t_frames, N_LMK)) * hw
      lmk[:, 48:68, 0] = rng.uniform(0.35, 0.65, (t_frames, 20)) * hw
      lmk[:, 48:68, 1] = rng.uniform(0.6, 0.8, (t_frames, 20)) * hw
      pool.append(((frames, lmk), cap))
    else:
      pool.append((rng.randn(t_frames, N_LMK, 3), cap))
  return [pool[i % len(pool)] for i in range(n_samples)]


def build_model(regime, dev, size=96, hidden=256):
  import torch
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  torch.manual_seed(123456)
  c2i = default_char2idx()
  if regime == "X":
    from lipreading_amd.frontend import ConvFrontend3D, PixelLipReader, feature_dim
    enc = VideoEncoder(feature_dim(size, size), hidden, rnn_type="GRU", num_layers=2, bidirectional=True,
                       enable_ctc=True, vocab_size=VOCAB, char2idx=c2i)
    model = PixelLipReader(enc, ConvFrontend3D())
  else:
    model = VideoEncoder(N_LMK * 3, hidden, rnn_type="GRU", num_layers=1, bidirectional=True, enable_ctc=True,
                         vocab_size=VOCAB, char2idx=c2i)
  model = model.to(dev).train()
  return model, FusedAdam(FlatParameters(model), lr=1e-4), c2i


def _summary(ms):
  return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def time_arms(regime, dev, batch=32, n_batches=8, repeats=5, size=96, hw=96, depth=2, workers=2, hidden=256,
              t_frames=T_FRAMES, log=None, augment=None):
  """ms per step of train()'s loop over the three arms.  Returns {"plain": {...}, "prefetch": {...}, "resident": {...}}
  with median / min / max of ms_per_step over `repeats` epochs of `n_batches` steps.  augment: an AugmentSpec adds an
  "augmented" arm beside "prefetch" — the same loader with the spec, every epoch a new pass of draws."""
  import torch
  from lipreading_amd import train as T
  from lipreading_amd.data import make_collate_fn, make_pixel_collate_fn
  from lipreading_amd.dataset import BatchLoader
  from lipreading_amd.loader import PrefetchLoader
  pixels = regime == "X"
  ds = synthetic_dataset(regime, batch * n_batches, hw=hw, t_frames=t_frames)
  model, opt, c2i = build_model(regime, dev, size=size, hidden=hidden)
  graphs = T.StepGraphs(enabled=not pixels)      # R: hipGraphs on, as the driver has them; X: eager
  collate = make_pixel_collate_fn(dev, size=size) if pixels else make_collate_fn(dev)
  plain = BatchLoader(ds, batch, collate)
  prefetch = PrefetchLoader(ds, batch, dev, pixels=pixels, size=size, depth=depth, workers=workers)
  resident = [collate(ds[:batch])] * n_batches
  arms = (("plain", plain), ("prefetch", prefetch), ("resident", resident))
  augmented = None
  if augment is not None:
    augmented = PrefetchLoader(ds, batch, dev, pixels=pixels, size=size, depth=depth, workers=workers, augment=augment)
    arms = arms[:2] + (("augmented", augmented),) + arms[2:]

  host_s = {}

  class Timed(object):
    """The loader as train() sees it, with the host time spent inside its __next__ added up."""
    def __init__(self, name, loader):
      self.name, self.loader = name, loader
    def __len__(self):
      return len(self.loader)
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

  for _, loader in arms:                          # warm-up: allocator, graph capture, pinned ring
    epoch(loader)
    epoch(loader)
  ms = {name: [] for name, _ in arms}
  host_s.clear()
  for r in range(repeats):
    for name, loader in arms:
      ms[name].append(epoch(loader))
    if log:
      log("  %s repeat %d: " % (regime, r) + ", ".join("%s %.3f" % (n, ms[n][-1]) for n, _ in arms))
  prefetch.close()
  if augmented is not None:
    augmented.close()
  out = {name: _summary(v) for name, v in ms.items()}
  out["steps_per_epoch"], out["batch"], out["graphs"] = n_batches, batch, bool(graphs.enabled)
  out["timed_seconds_per_epoch"] = {n: statistics.median(v) * n_batches / 1e3 for n, v in ms.items()}
  # host time inside the loader's __next__ per step (the step's launches are issued by the same thread: in a loop
  # that is bound by the host's launch rate this time adds to the step, overlapped or not on the device)
  out["host_ms_in_loader_per_step"] = {n: host_s.get(n, 0.0) * 1e3 / (repeats * n_batches) for n in ms}
  return out


def _event_ms(fn, stream, reps):
  import torch
  out = []
  for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    out.append(e0.elapsed_time(e1))
  return out


def time_draw(spec, batch=32, t_frames=T_FRAMES, reps=50):
  """Host milliseconds per batch inside AugmentSpec.draw (what a worker thread spends under the GIL)."""
  lens = np.full(batch, t_frames)
  spec.draw(0, np.arange(batch), lens)
  ms = []
  for r in range(reps):
    t0 = time.perf_counter()
    spec.draw(r, np.arange(batch) + r * batch, lens)
    ms.append((time.perf_counter() - t0) * 1e3)
  return dict(_summary(ms), batch=batch, frames=t_frames, policy=str(spec))


def time_kernel(dev, batch=32, size=96, hw=96, t_frames=T_FRAMES, reps=10, augment=None):
  """lr_lip_crop_collate_u8 beside the summed B per-sample lr_lip_crop_u8 launches it replaces (device events).
  augment: an AugmentSpec adds lr_lip_crop_collate_aug_u8 on that spec's draw as a third alternated arm."""
  import torch
  from lipreading_amd import _C
  from lipreading_amd.landmarks import _mouth
  L = _C.lib()
  rng = np.random.RandomState(7)
  rows = batch * t_frames
  frames = torch.from_numpy(rng.randint(0, 256, (rows, 3, hw, hw)).astype(np.uint8)).to(dev)
  lm = np.zeros((rows, N_LMK, 3), np.float32)
  lm[:, :, 0] = rng.uniform(0.35, 0.65, (rows, N_LMK)) * hw
  lm[:, :, 1] = rng.uniform(0.6, 0.8, (rows, N_LMK)) * hw
  lmk = torch.from_numpy(lm).to(dev)
  offsets = torch.arange(batch, dtype=torch.int64, device=dev) * t_frames
  lens = torch.full((batch,), t_frames, dtype=torch.int32, device=dev)
  out = torch.empty((batch, t_frames, 3, size, size), dtype=torch.uint8, device=dev)
  stream = torch.cuda.current_stream(dev)

  def one_launch():
    _C.check(L.lr_lip_crop_collate_u8(frames.data_ptr(), lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(),
                                      out.data_ptr(), batch, t_frames, hw, hw, size, N_LMK, _mouth.start, _mouth.stop, 0.3,
                                      stream.cuda_stream), "lr_lip_crop_collate_u8")

  def per_sample():     # (the torch.zeros of the plain collate is not counted: every frame here is a real one)
    for b in range(batch):
      lo = b * t_frames
      _C.check(L.lr_lip_crop_u8(frames[lo:lo + t_frames].data_ptr(), lmk[lo:lo + t_frames].data_ptr(), out[b].data_ptr(),
                                t_frames, hw, hw, size, N_LMK, _mouth.start, _mouth.stop, 0.3, stream.cuda_stream),
               "lr_lip_crop_u8")

  if augment is not None:
    clip, tmap = augment.draw(0, np.arange(batch), np.full(batch, t_frames))
    clip_d, tmap_d = torch.from_numpy(clip).to(dev), torch.from_numpy(tmap).to(dev)

  def one_launch_augmented():
    _C.check(L.lr_lip_crop_collate_aug_u8(frames.data_ptr(), lmk.data_ptr(), offsets.data_ptr(), lens.data_ptr(),
                                          clip_d.data_ptr(), tmap_d.data_ptr(), out.data_ptr(), batch, t_frames, hw, hw,
                                          size, N_LMK, _mouth.start, _mouth.stop, 0.3, stream.cuda_stream),
             "lr_lip_crop_collate_aug_u8")

  _event_ms(one_launch, stream, 3), _event_ms(per_sample, stream, 3)
  if augment is not None:
    _event_ms(one_launch_augmented, stream, 3)
  a, b, c = [], [], []
  for _ in range(reps):                       # alternated
    a += _event_ms(one_launch, stream, 1)
    b += _event_ms(per_sample, stream, 1)
    if augment is not None:
      c += _event_ms(one_launch_augmented, stream, 1)
  nbytes = out.numel() + frames.numel()
  res = {"collate_one_launch_ms": _summary(a), "per_sample_launches_ms": _summary(b),
         "bytes_written_plus_read": int(nbytes), "shape": [batch, t_frames, 3, size, size], "source_hw": [hw, hw]}
  if augment is not None:
    res["augmented_one_launch_ms"] = _summary(c)
    res["policy"] = str(augment)
    res["masked_frames"] = int((tmap < 0).sum())
  res["collate_GBps"] = nbytes / (res["collate_one_launch_ms"]["median"] * 1e-3) / 1e9
  return res


def time_upload(dev, nbytes, reps=10):
  """Host-to-device GB/s of one slot-sized copy: from pinned memory on a side stream (the loader's upload) and from
  pageable memory (the plain collate's)."""
  import torch
  side = torch.cuda.Stream(dev)
  dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
  pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
  pageable = torch.empty(nbytes, dtype=torch.uint8)
  pinned.fill_(1), pageable.fill_(1)
  with torch.cuda.stream(side):
    _event_ms(lambda: dst.copy_(pinned, non_blocking=True), side, 2)
    ms_pin = _event_ms(lambda: dst.copy_(pinned, non_blocking=True), side, reps)
  torch.cuda.synchronize(dev)
  ms_page = []
  for _ in range(reps):
    t0 = time.perf_counter()
    dst.copy_(pageable, non_blocking=True)
    torch.cuda.synchronize(dev)
    ms_page.append((time.perf_counter() - t0) * 1e3)
  g = lambda ms: nbytes / (statistics.median(ms) * 1e-3) / 1e9
  return {"bytes": int(nbytes), "pinned_ms": _summary(ms_pin), "pinned_GBps": g(ms_pin),
          "pageable_ms": _summary(ms_page), "pageable_GBps": g(ms_page)}


def time_host_gather(batch=32, hw=96, workers=2, reps=5):
  """GB/s of the host stage alone: samples -> slot (plain memory; no GPU involved)."""
  from lipreading_amd.loader import HostStage
  ds = synthetic_dataset("X", batch * 6, hw=hw)
  stage = HostStage(ds, batch, pixels=True, depth=2, workers=workers)
  ms = []
  for _ in range(reps):
    t0 = time.perf_counter()
    n = sum(pb.nbytes for pb in stage)
    ms.append((time.perf_counter() - t0) * 1e3)
  return {"bytes_per_epoch": int(n), "workers": workers, "epoch_ms": _summary(ms),
          "GBps": n / (statistics.median(ms) * 1e-3) / 1e9}


# ---- overlap evidence: one run under rocprofv3 --------------------------------------------------------------------
def trace_child(args):
  """The traced program: a short prefetched loop of regime X (nothing is timed here)."""
  import torch
  dev = torch.device("cuda:0")
  from lipreading_amd import train as T
  from lipreading_amd.loader import PrefetchLoader
  ds = synthetic_dataset("X", args.batch * 16)
  model, opt, c2i = build_model("X", dev, size=args.size)
  loader = PrefetchLoader(ds, args.batch, dev, pixels=True, size=args.size, depth=args.depth, workers=args.workers)
  with contextlib.redirect_stdout(io.StringIO()):
    for _ in range(3):                        # 48 steps; the first uploads of each pass prime the pipe
      T.train(model, None, loader, opt, dev, c2i, grad_norm=50)
  torch.cuda.synchronize(dev)
  loader.close()


def _rows(path):
  with open(path, newline="") as f:
    return list(csv.DictReader(f))


def _merge(spans, gap=0):
  merged = []
  for s, e in spans:
    if merged and s <= merged[-1][1] + gap:
      merged[-1][1] = max(merged[-1][1], e)
    else:
      merged.append([s, e])
  return merged


def _covered(uploads, merged):
  inside = 0
  for s, e in uploads:
    for ks, ke in merged:
      if ke <= s:
        continue
      if ks >= e:
        break
      inside += min(e, ke) - max(s, ks)
  return inside


def summarise_trace(directory, min_copy_ns=200000, busy_gap_ns=50000):
  """Host-to-device copies of at least `min_copy_ns` (the slot uploads) against the union of the other kernels'
  intervals, and against the device's busy periods (kernel intervals merged across gaps below `busy_gap_ns`: an eager
  step leaves the device idle between launches, and an upload inside such a gap still runs beside the step)."""
  kfiles = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
  cfiles = glob.glob(os.path.join(directory, "**", "*memory_copy_trace.csv"), recursive=True)
  if not kfiles or not cfiles:
    return {"error": "trace files missing", "found": sorted(os.listdir(directory))}
  kernels = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Kernel_Name", ""), r.get("Queue_Id", ""),
              r.get("Stream_Id", "")) for r in _rows(kfiles[0])]
  copies = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Direction", "")) for r in _rows(cfiles[0])]
  uploads = [(s, e) for s, e, d in copies if "HOST_TO_DEVICE" in d.upper() and e - s >= min_copy_ns]
  spans = sorted((s, e) for s, e, n, _, _ in kernels if "lip_crop_collate" not in n)
  total = sum(e - s for s, e in uploads)
  inside = _covered(uploads, _merge(spans))
  inside_busy = _covered(uploads, _merge(spans, busy_gap_ns))
  # how busy the device is over the whole traced span, from the first upload to the last kernel (this includes the
  # one-off initialisation inside the first step: context only, not a figure about a steady step)
  t0, t1 = (min(s for s, _ in uploads), max(e for _, e in spans)) if uploads and spans else (0, 0)
  busy = sum(min(e, t1) - max(s, t0) for s, e in _merge(spans) if e > t0 and s < t1)
  collate_q = sorted({(q, st) for _, _, n, q, st in kernels if "lip_crop_collate" in n})
  other_q = sorted({(q, st) for _, _, n, q, st in kernels if "lip_crop_collate" not in n})
  return {"uploads": len(uploads), "upload_ns_total": total, "upload_ns_inside_kernel_intervals": inside,
          "upload_ns_outside_kernel_intervals": total - inside,
          "fraction_inside": (inside / total) if total else None,
          "upload_ns_inside_busy_periods": inside_busy, "busy_gap_ns": busy_gap_ns,
          "device_kernel_busy_fraction": (busy / (t1 - t0)) if t1 > t0 else None,
          "fraction_inside_busy_periods": (inside_busy / total) if total else None,
          "collate_kernel_queue_stream_ids": collate_q, "other_kernels_queue_stream_ids": other_q,
          "copy_stream_shares_a_queue_with_compute": bool({q for q, _ in collate_q} & {q for q, _ in other_q}),
          "kernels": len(kernels), "copies": len(copies)}


def run_trace(args):
  prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
  if not os.path.exists(prof):
    return {"error": "rocprofv3 not found"}
  tmp = tempfile.mkdtemp(prefix="loader_trace_")
  try:
    cmd = [prof, "--kernel-trace", "--memory-copy-trace", "-f", "csv", "-d", tmp, "-o", "loader", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", "--batch", str(args.batch), "--size",
           str(args.size), "--depth", str(args.depth), "--workers", str(args.workers)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.trace_timeout)
    if res.returncode != 0:
      return {"error": "traced run exited %d" % res.returncode, "stderr": res.stderr[-1500:]}
    return summarise_trace(tmp)
  except subprocess.TimeoutExpired:
    return {"error": "traced run exceeded %d s" % args.trace_timeout}
  finally:
    shutil.rmtree(tmp, ignore_errors=True)


def parse_args(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
  ap.add_argument("--regimes", default="R,X", help="comma-separated: R (landmarks, hipGraphs), X (pixels, eager)")
  ap.add_argument("--batch", type=int, default=32)
  ap.add_argument("--batches", type=int, default=None, help="steps per epoch (default: R 2560, X 256: a timed window "
                  "of a second or more per arm and epoch)")
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--size", type=int, default=96, help="crop size of regime X")
  ap.add_argument("--depth", type=int, default=2)
  ap.add_argument("--workers", type=int, default=2)
  ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
  ap.add_argument("--trace-timeout", type=int, default=240)
  ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
  ap.add_argument("--augment", default="", help="an augmentation policy (augment.AugmentSpec.parse): time the augmented "
                  "loader and kernel beside the prefetched ones and write profiles/augment_loop.json")
  ap.add_argument("--out", default=None, help="default: profiles/loader_loop.json (profiles/augment_loop.json with "
                  "--augment)")
  args = ap.parse_args(argv)
  if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "augment_loop.json" if args.augment else "loader_loop.json")
  args.regimes = [r for r in args.regimes.upper().split(",") if r]
  assert set(args.regimes) <= {"R", "X"} and args.regimes, "--regimes takes R and/or X"
  assert args.repeats >= 5, "at least five repeats per arm"
  assert 1 <= args.workers <= 8 and args.depth >= 1
  return args


def main(argv=None):
  args = parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    print("bench_loader: no GPU — this tool measures the MI355X loop and has no fallback", file=sys.stderr)
    return 2
  from lipreading_amd import _build
  _build.build_library()
  if args.trace_child:
    trace_child(args)
    return 0
  dev = torch.device("cuda:0")
  log = lambda s: print(s, file=sys.stderr, flush=True)
  doc = {"tool": "tools/bench_loader.py", "device": torch.cuda.get_device_name(0), "depth": args.depth,
         "workers": args.workers, "repeats": args.repeats, "regimes": {}}
  from lipreading_amd.augment import AugmentSpec
  spec = AugmentSpec.parse(args.augment, seed=123456)
  for regime in args.regimes:
    n_batches = args.batches or (2560 if regime == "R" else 256)
    log("regime %s: %d steps per epoch" % (regime, n_batches))
    doc["regimes"][regime] = time_arms(regime, dev, batch=args.batch, n_batches=n_batches, repeats=args.repeats,
                                       size=args.size, depth=args.depth, workers=args.workers, log=log, augment=spec)
  if spec is not None:
    # the kernel under the policy and under one that touches the same bytes per frame as the plain launch (no zoom,
    # no masks), each beside its own alternated plain arm; and the host's share, the draws
    doc["policy"] = str(spec)
    doc["draw_host_ms_per_batch"] = time_draw(spec, batch=args.batch)
    if "X" in args.regimes:
      doc["kernel"] = {"policy": time_kernel(dev, batch=args.batch, size=args.size, augment=spec),
                       "same_bytes": time_kernel(dev, batch=args.batch, size=args.size,
                                                 augment=AugmentSpec.parse(SAME_BYTES_POLICY, seed=123456))}
  elif "X" in args.regimes:
    doc["kernel"] = time_kernel(dev, batch=args.batch, size=args.size)
    slot = args.batch * T_FRAMES * (3 * 96 * 96 + N_LMK * 3 * 4)
    doc["upload"] = time_upload(dev, slot)
    doc["host_gather"] = time_host_gather(batch=args.batch, workers=args.workers)
    if not args.no_trace:
      log("tracing one prefetched run of regime X under rocprofv3")
      doc["overlap_trace"] = run_trace(args)
  text = json.dumps(doc, indent=1, sort_keys=True)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    f.write(text + "\n")
  print(text)
  return 0


if __name__ == "__main__":
  sys.exit(main())
