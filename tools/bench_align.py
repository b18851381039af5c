#!/usr/bin/env python
"""Measure the forced aligner: µs per CTCAligner.align_ids call (one lr_ctc_align launch), and beside it what the
host would need for the same answer — the device->host copy of the log-probs plus the NumPy restatement of
tests/align_cases.py (states vectorised, frames and samples in Python loops).  bench.py stays as it is.

  python tools/bench_align.py                 # one JSON document on stdout and profiles/align.json
  python tools/bench_align.py --no-save --repeats 1 --calls 20

Shapes: B = 32 and 256 at T = 75 with 30-token targets (the caption configurations: the one-wave kernel), and one
long shape, B = 8 at T = 2048 with 256-token targets (the multi-wave kernel at its limits).  C = 65, random
log-softmax rows, every sample feasible.  Protocol: five warm-up calls, then `repeats` rounds with the two arms
alternated; the device arm is `calls` launches back to back between two device events (the cost a loop sees per call,
not one launch's latency), the host arm one pass under the host clock.  Medians and min-max.

No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SHAPES = ((32, 75, 30), (256, 75, 30), (8, 2048, 256))
C = 65


def _summary(v):
  return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def placement(lib, B, T, L):
  """Which kernel a shape takes and where its tables lie: the library's own answer (lr_ctc_align_plan)."""
  import ctypes
  plan = (ctypes.c_int32 * 5)()
  assert lib.lr_ctc_align_plan(B, T, C, L, ctypes.addressof(plan)) == 0
  one_wave, threads, rows_in_lds, table_in_lds, lds_bytes = list(plan)
  return {"kernel": "one-wave" if one_wave else "multi-wave", "threads": threads,
          "rows": "LDS" if rows_in_lds else "global, 16 steps ahead in registers",
          "table": "LDS" if table_in_lds else "workspace", "dynamic_lds_bytes": lds_bytes}


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--calls", type=int, default=100)
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    print("bench_align: no GPU (this tool never falls back)", file=sys.stderr)
    return 2
  from lipreading_amd import _C, _build, lm
  _build.build_library()
  from lipreading_amd.align import CTCAligner
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.decoder import ctc_labels
  from tests import align_cases as A
  dev = torch.device("cuda:0")
  labels = ctc_labels(default_char2idx())
  roles = lm.class_roles(labels, 0)
  al = CTCAligner(labels)
  lib = _C.lib()
  doc = {"unit": "us per call", "C": C, "calls": a.calls, "shapes": {}}
  for B, T, L in SHAPES:
    rng = np.random.RandomState(B + T)
    lp_h = A.log_softmax(rng, (B, T, C))
    tg_h = np.stack([A.random_target(rng, L, C, 0) for _ in range(B)]).astype(np.int32)
    tl_h, sz_h = np.full(B, L, np.int32), np.full(B, T, np.int32)
    lp, tg, tl, sz = (torch.from_numpy(x).to(dev) for x in (lp_h, tg_h, tl_h, sz_h))
    calls = a.calls if T <= 256 else max(a.calls // 10, 3)

    def device_arm():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize(dev)
      e0.record()
      for _ in range(calls):
        out = al.align_ids(lp, sz, tg, tl)
      e1.record()
      torch.cuda.synchronize(dev)
      return e0.elapsed_time(e1) * 1e3 / calls, out

    def host_arm():
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      host = lp.cpu().numpy()
      t1 = time.perf_counter()
      want = A.expected(host, sz_h, tg_h, tl_h, 0, roles)
      return (t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6, want

    for _ in range(5):
      al.align_ids(lp, sz, tg, tl)
    dev_us, copy_us, numpy_us = [], [], []
    for r in range(a.repeats):
      t, out = device_arm()
      dev_us.append(t)
      c, n, want = host_arm()
      copy_us.append(c)
      numpy_us.append(n)
      print("B=%d T=%d L=%d repeat %d: device %.1f us, copy %.1f us, numpy %.1f us" % (B, T, L, r, t, c, n),
            file=sys.stderr, flush=True)
    for k, v in out.items():   # the two arms answer the same
      assert np.array_equal(v.cpu().numpy(), want[k]), k
    assert (want["status"] == 0).all()
    row = dict(placement(lib, B, T, L), device=_summary(dev_us), host_copy=_summary(copy_us),
               host_numpy=_summary(numpy_us))
    row["host_over_device"] = (row["host_copy"]["median"] + row["host_numpy"]["median"]) / row["device"]["median"]
    doc["shapes"]["B%d_T%d_L%d" % (B, T, L)] = row
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(os.path.join(ROOT, "profiles", "align.json"), "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
