#!/usr/bin/env python
"""Measure CTC segmentation: milliseconds of one lr_ctc_segment call by phase — the forward launches,
the walk back, the span launches — from device events recorded between them on the stream (lr_ctc_segment_phases), and
beside them what the host needs for the same answer at the first shape: the NumPy restatement of
tests/segment_cases.py.  The parent of this feature cannot segment at all, so there is no earlier time to compare
with.  bench.py stays as it is.

  python tools/bench_segment.py                 # one JSON document on stdout and profiles/segment.json
  python tools/bench_segment.py --no-save --repeats 2

Shapes (T, L), B = 1: (4096, 1024), (16384, 4096) and (65536, 16384) — a 2-minute, a 9-minute and the longest video
the kernels take, four frames per caption character.  C = 65.  Frames are peaked as a trained model's are: a planted
path spells the target in runs of 1 to 3 frames per token, blank elsewhere, and the planted class of a frame gets +8 on
logits of 3 * randn before the log-softmax; junk frames at both ends.  Eight utterances, both ends free.
Protocol: two warm-up calls per shape, then `repeats` timed calls; medians and min-max.  The outputs at the first shape
are checked equal to the restatement's in the run.

No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHAPES = ((4096, 1024), (16384, 4096), (65536, 16384))
C = 65
UTTS = 8


def _summary(v):
  return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def peaked_stream(rng, T, L):
  """(lp (1, T, C) float32, target [L]): see the module's docstring."""
  target = rng.randint(1, C, size=L)
  head = T // 32
  frames = np.zeros(T, np.int64)
  frames[:head] = rng.randint(1, C, size=head)
  frames[T - head:] = rng.randint(1, C, size=head)
  at, room = head, T - 2 * head
  per = room // L                       # frames a token may take with its blank
  for i in range(L):
    run = int(rng.randint(1, min(3, per - 1) + 1))
    frames[at + 1:at + 1 + run] = target[i]      # (the frame before it stays blank: repeats need one)
    at += per
  logits = (rng.randn(T, C) * 3).astype(np.float32)
  logits[np.arange(T), frames] += np.float32(8)
  logits -= logits.max(axis=1, keepdims=True)
  lp = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True, dtype=np.float32))
  return lp.astype(np.float32)[None], target


def utterances(L):
  per = L // UTTS
  first = np.arange(UTTS, dtype=np.int32) * per
  count = np.full(UTTS, per, np.int32)
  count[-1] = L - first[-1]
  return first[None], count[None], np.array([UTTS], np.int32)


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    print("bench_segment: no GPU (this tool never falls back)", file=sys.stderr)
    return 2
  from lipreading_amd import _C, _build
  _build.build_library()
  from lipreading_amd.segment import CTCSegmenter
  from tests import segment_cases as S
  dev = torch.device("cuda:0")
  lib = _C.lib()
  sg = CTCSegmenter(["c%d" % i for i in range(C)])
  doc = {"unit": "ms per call", "B": 1, "C": C, "utterances": UTTS, "device": torch.cuda.get_device_name(0), "shapes": {}}
  for k, (T, L) in enumerate(SHAPES):
    rng = np.random.RandomState(T + L)
    lp_h, target = peaked_stream(rng, T, L)
    uf, uc, nu = utterances(L)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    args = (d(lp_h), None, d(target[None].astype(np.int32)), d(np.array([L], np.int32)), d(uf), d(uc), d(nu))
    plan = (ctypes.c_int32 * _C.LR_SEG_PLAN_WORDS)()
    assert lib.lr_ctc_segment_plan(1, T, C, L, ctypes.addressof(plan)) == 0
    own, frames, launches, wgs, threads, lds = list(plan)
    ms = (ctypes.c_float * 3)()
    for _ in range(2):
      out = sg._segment_ids(*args, True, True, phase_ms=ms)
    fwd, walk, spans, whole = [], [], [], []
    for r in range(a.repeats):
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      out = sg._segment_ids(*args, True, True, phase_ms=ms)      # (waits for the device)
      whole.append((time.perf_counter() - t0) * 1e3)
      fwd.append(ms[0])
      walk.append(ms[1])
      spans.append(ms[2])
      print("T=%d L=%d repeat %d: forward %.3f ms, walk %.3f ms, spans %.3f ms, call %.3f ms"
            % (T, L, r, ms[0], ms[1], ms[2], whole[-1]), file=sys.stderr, flush=True)
    assert int(out["status"][0]) == 0
    span = out["span"][0].tolist()
    cells = T * (2 * L + 1)
    row = {"states_per_workgroup": own, "frames_per_launch": frames, "forward_launches": launches,
           "workgroups_per_launch": wgs, "threads": threads, "dynamic_lds_bytes": lds,
           "workspace_bytes": lib.lr_ctc_segment_workspace_bytes(1, T, C, L), "lattice_cells": cells,
           "forward": _summary(fwd), "walk": _summary(walk), "spans": _summary(spans), "call_host_clock": _summary(whole),
           "forward_cells_per_us": cells / (statistics.median(fwd) * 1e3), "span": span, "total": float(out["total"][0])}
    if k == 0:
      t0 = time.perf_counter()
      want = S.expected(lp_h, None, target[None].astype(np.int32), np.array([L], np.int32), 0, 3, uf, uc, nu)
      row["host_numpy_ms"] = (time.perf_counter() - t0) * 1e3
      for key, v in out.items():   # the two answer the same
        assert np.array_equal(v.cpu().numpy(), want[key]), key
      row["host_over_device"] = row["host_numpy_ms"] / (row["forward"]["median"] + row["walk"]["median"]
                                                        + row["spans"]["median"])
    doc["shapes"]["T%d_L%d" % (T, L)] = row
    del args, out
    sg._ws = type(sg._ws)()      # (the next shape's workspace is larger: let this one go first)
    torch.cuda.empty_cache()
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(os.path.join(ROOT, "profiles", "segment.json"), "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
