#!/usr/bin/env python
"""Measure the transducer beam search (lipreading_amd/transducer.py rnnt_beam) at T = 75, V1 = 65,
J = 256, context 2, max_symbols = 3 for B = 1, 8, 32 and beam_width = 4, 8, 16.  bench.py stays as it is.

  python tools/bench_transducer_beam.py                  # one JSON line on stdout and profiles/transducer_beam.json
  python tools/bench_transducer_beam.py --no-save --repeats 1 --calls 2

Per (B, beam_width), us per call:
  beam          one rnnt_beam call over the batch (the weight-operand launch and the search launch)
  greedy        one rnnt_greedy launch on the same inputs (max_symbols = 3 as well)
  torch_floor   a floor for any host-driven search: T * (max_symbols + 1) rounds of the joint stage alone from torch
                device ops over [B * beam_width, J] rows (gather of the table rows, add, tanh, matmul, masked
                log_softmax, top-k) with no merging, no bookkeeping and no host read
and, from the float64 restatement of tests/transducer_beam_cases.py on the first clips of the same inputs (CPU, not
timed): the label rounds run per frame and the merges per clip.
Protocol: warm-up calls, then `repeats` rounds with the arms alternated; an arm is `calls` calls back to back between
two device events.  Medians and min-max.  No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

T, V1, J, CONTEXT, MAX_SYMBOLS = 75, 65, 256, 2, 3
BATCHES = (1, 8, 32)
WIDTHS = (4, 8, 16)
STAT_CLIPS = 2


def _summary(v):
  return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def _timed(torch, calls, fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  e0.record()
  for _ in range(calls):
    fn()
  e1.record()
  torch.cuda.synchronize()
  return e0.elapsed_time(e1) * 1e3 / calls


def _rounds(torch, arms, repeats, calls):
  for fn in arms.values():
    for _ in range(2):
      fn()
  out = {k: [] for k in arms}
  for _ in range(repeats):
    for k, fn in arms.items():
      out[k].append(_timed(torch, calls, fn))
  return {k: _summary(v) for k, v in out.items()}


def leg(torch, B, width, repeats, calls):
  from lipreading_amd import transducer as TR
  from tests import transducer_beam_cases as K
  dev = torch.device("cuda")
  g = torch.Generator().manual_seed(B)
  r = lambda *s: torch.randn(*s, generator=g)
  host = dict(e=r(B, T, J), W=r(V1, J) * (3.0 / J ** 0.5), b=r(V1) * 0.1, tables=r(CONTEXT, V1, J) * 0.7)
  host["b"][0] += 2.0
  host["mask"] = torch.ones(V1)
  host["mask"][2] = host["mask"][5] = 0
  e, W, b, tables, mask = (host[k].to(dev) for k in ("e", "W", "b", "tables", "mask"))
  sizes = torch.full((B,), T, dtype=torch.int32, device=dev)
  rows = B * width
  c0 = torch.randint(0, V1, (rows,), generator=g).to(dev)
  c1 = torch.randint(0, V1, (rows,), generator=g).to(dev)
  e_rows = e.repeat_interleave(width, dim=0)   # (rows, T, J)

  def floor():
    for t in range(T):
      for _ in range(MAX_SYMBOLS + 1):
        z = torch.tanh(e_rows[:, t] + tables[0][c0] + tables[1][c1])
        lp = torch.log_softmax((z @ W.t() + b).masked_fill(mask == 0, float("-inf")), dim=-1)
        lp.reshape(B, width * V1).topk(width, dim=1)

  arms = {"beam": lambda: TR.rnnt_beam(e, sizes, tables, W, b, mask, beam_width=width, max_symbols=MAX_SYMBOLS),
          "greedy": lambda: TR.rnnt_greedy(e, sizes, tables, W, b, mask, max_symbols=MAX_SYMBOLS),
          "torch_floor": floor}
  out = _rounds(torch, arms, repeats, calls)
  n = min(B, STAT_CLIPS)
  stats = K.new_stats()
  d = lambda k: host[k].double()
  K.beam_search(d("e")[:n], [T] * n, d("tables"), d("W"), d("b"), d("mask"), beam_width=width,
                max_symbols=MAX_SYMBOLS, stats=stats)
  out.update(B=B, beam_width=width, label_rounds_per_frame=stats["label_rounds"] / stats["frames"],
             merges_per_clip=stats["merges"] / n, stat_clips=n,
             beam_over_greedy=out["beam"]["median"] / out["greedy"]["median"],
             beam_over_torch_floor=out["beam"]["median"] / out["torch_floor"]["median"])
  print("B %d width %d: beam %.0f, greedy %.0f, torch floor %.0f us" % (B, width, out["beam"]["median"],
        out["greedy"]["median"], out["torch_floor"]["median"]), file=sys.stderr, flush=True)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--calls", type=int, default=3)
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    print("bench_transducer_beam: no GPU (this tool never falls back)", file=sys.stderr)
    return 1
  doc = {"tool": "bench_transducer_beam", "unit": "us per call", "device": torch.cuda.get_device_name(0),
         "shape": {"T": T, "V1": V1, "J": J, "context": CONTEXT, "max_symbols": MAX_SYMBOLS},
         "repeats": a.repeats, "calls": a.calls,
         "legs": [leg(torch, B, w, a.repeats, a.calls) for B in BATCHES for w in WIDTHS]}
  line = json.dumps(doc, sort_keys=True)
  print(line)
  if not a.no_save:
    with open(os.path.join(ROOT, "profiles", "transducer_beam.json"), "w") as f:
      f.write(line + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
