#!/usr/bin/env python
"""Measure the keyword spotter: µs per KeywordSpotter.spot_ids call (one lr_ctc_spot launch plus the gathers that put
the keywords back into the caller's order), and beside it what the host would need for the same answer — the
device->host copy of the log-probs plus the NumPy restatement of tests/spot_cases.py (states and keywords vectorised;
frames and samples in Python loops, the hit selection per pair).  The parent of this feature cannot spot at all, so
there is no earlier time to compare with.  bench.py stays as it is.

  python tools/bench_spot.py                 # one JSON document on stdout and profiles/spot.json
  python tools/bench_spot.py --no-save --repeats 1 --calls 20

Shapes (B, T, K): (32, 75, 100) and (32, 75, 1000) — the caption configuration with a short and a long keyword list —
and (8, 2048, 100), the longest clip the kernel takes.  C = 65, random log-softmax rows, keywords of 3 to 10 tokens
drawn with a fixed seed, max_hits = 4, no threshold.  Protocol: five warm-up calls, then `repeats` rounds with the two
arms alternated; the device arm is `calls` calls back to back between two device events (the cost a loop sees per
call, not one launch's latency), the host arm one pass under the host clock.  Medians and min-max.  Both arms are
checked equal in the run.

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

SHAPES = ((32, 75, 100), (32, 75, 1000), (8, 2048, 100))
C = 65
FIRST_CHAR = 5      # classes 5.. of the default labels are single characters
MAX_HITS = 4


def _summary(v):
  return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def placement(lib, B, T, K, W):
  """What a shape launches and where its rows and traces lie: the library's own answer (lr_ctc_spot_plan)."""
  import ctypes
  plan = (ctypes.c_int32 * 11)()
  assert lib.lr_ctc_spot_plan(B, T, C, K, W, MAX_HITS, ctypes.addressof(plan)) == 0
  seg, threads, side, groups, rows_in_lds, trace_at, lds_bytes, per_wg, len16, len32, wgs = list(plan)
  return {"threads": threads, "keyword_groups_per_workgroup": groups, "keywords_per_workgroup": per_wg,
          "workgroups": wgs, "segment_of_longest_keyword": seg, "longest_keyword_16_lanes": len16,
          "longest_keyword_32_lanes": len32,
          "rows": "LDS, as ratios" if rows_in_lds else "global, 16 steps ahead in registers; m[t] in LDS",
          "trace": "LDS" if trace_at == 0 else "workspace", "dynamic_lds_bytes": lds_bytes}


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--calls", type=int, default=100)
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    print("bench_spot: no GPU (this tool never falls back)", file=sys.stderr)
    return 2
  from lipreading_amd import _C, _build
  _build.build_library()
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.decoder import ctc_labels
  from lipreading_amd.spot import KeywordSpotter
  from tests import spot_cases as S
  dev = torch.device("cuda:0")
  labels = ctc_labels(default_char2idx())
  lib = _C.lib()
  doc = {"unit": "us per call", "C": C, "calls": a.calls, "max_hits": MAX_HITS, "keyword_tokens": [3, 10], "shapes": {}}
  for B, T, K in SHAPES:
    rng = np.random.RandomState(B + T + K)
    lp_h = S.log_softmax(rng, (B, T, C))
    words = [''.join(labels[FIRST_CHAR + int(c)] for c in rng.randint(0, C - FIRST_CHAR, size=rng.randint(3, 11)))
             for _ in range(K)]
    sp = KeywordSpotter(labels, words, max_hits=MAX_HITS)
    lp = torch.from_numpy(lp_h).to(dev)
    calls = a.calls if T <= 256 else max(a.calls // 10, 3)

    def device_arm():
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize(dev)
      e0.record()
      for _ in range(calls):
        out = sp.spot_ids(lp)
      e1.record()
      torch.cuda.synchronize(dev)
      return e0.elapsed_time(e1) * 1e3 / calls, out

    def host_arm():
      torch.cuda.synchronize(dev)
      t0 = time.perf_counter()
      host = lp.cpu().numpy()
      t1 = time.perf_counter()
      want = S.expected(host, None, sp.ids, sp.lengths, 0, None, MAX_HITS)
      return (t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6, want

    for _ in range(5):
      sp.spot_ids(lp)
    dev_us, copy_us, numpy_us = [], [], []
    for r in range(a.repeats):
      t, out = device_arm()
      dev_us.append(t)
      c, n, want = host_arm()
      copy_us.append(c)
      numpy_us.append(n)
      print("B=%d T=%d K=%d repeat %d: device %.1f us, copy %.1f us, numpy %.1f us"
            % (B, T, K, r, t, copy_us[-1], numpy_us[-1]), file=sys.stderr, flush=True)
    for k, v in out.items():   # the two arms answer the same
      assert np.array_equal(v.cpu().numpy(), want[k]), k
    full = sp.spot_ids(lp, trace=True)
    for k, v in full.items():
      assert np.array_equal(v.cpu().numpy(), want[k]), k
    assert (want["status"] == 0).all()
    row = dict(placement(lib, B, T, K, sp.ids.shape[1]), device=_summary(dev_us), host_copy=_summary(copy_us),
               host_numpy=_summary(numpy_us), hits=int(want["n_hits"].sum()))
    row["host_over_device"] = (row["host_copy"]["median"] + row["host_numpy"]["median"]) / row["device"]["median"]
    doc["shapes"]["B%d_T%d_K%d" % (B, T, K)] = row
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(os.path.join(ROOT, "profiles", "spot.json"), "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
