#!/usr/bin/env python
"""Measure the EVALUATION loop: greedy_cer / ctc_cer (ids to the host, Python strings, a pure-Python Levenshtein per
utterance) against train.device_cer (lr_edit_distance on the ids where they lie, one read per loader), and the
scoring kernel alone.  bench.py stays as it is; this tool is the scorer's yardstick.

  python tools/bench_score.py                      # one JSON document on stdout and profiles/score_loop.json
  python tools/bench_score.py --batches 8 --arms device --repeats 1 --no-kernel --no-save    # what the traces run
  python tools/bench_score.py --count-copies DIR   # copies by direction in a rocprofv3 --memory-copy-trace output (csv or rocpd)

Protocol: an in-memory synthetic set of fixed-length T = 75 landmark clips with 30-character labels, B = 32, an
untrained BiGRU-256 + CTC head (its greedy transcripts are long and wrong: the host scorer's expensive case, and the
common one early in training), decoders greedy and BeamCTCDecoder(beam_width=100).  Two warm-up passes per arm, then
`repeats` timed passes per arm with the arms alternated; the host clock around the call plus a device synchronise;
medians and min-max of ms per batch.  The kernel alone: 32 / 256 / 1000 pairs of 75 against 30 ids, `calls` launches
back to back between two device events (the launches overlap their own enqueue cost, so this is the cost a loop sees
per call, not a single launch's latency).

No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

T_FRAMES, N_LMK, VOCAB, LABEL_LEN, BATCH = 75, 68, 64, 30, 32


def synthetic_dataset(n_samples, seed=123456, distinct=64):
  rng = np.random.RandomState(seed)
  pool = [(rng.randn(T_FRAMES, N_LMK, 3), np.array([1] + list(rng.randint(4, VOCAB, LABEL_LEN)) + [2]))
          for _ in range(min(distinct, n_samples))]
  return [pool[i % len(pool)] for i in range(n_samples)]


def _summary(ms):
  return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def time_loops(dev, n_batches, repeats, arms, log):
  import torch
  from lipreading_amd import train as T
  from lipreading_amd.data import default_char2idx, make_collate_fn
  from lipreading_amd.dataset import BatchLoader
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.encoder import VideoEncoder
  torch.manual_seed(123456)
  c2i = default_char2idx()
  enc = VideoEncoder(N_LMK * 3, 256, rnn_type="GRU", num_layers=1, bidirectional=True, enable_ctc=True,
                     vocab_size=VOCAB, char2idx=c2i).to(dev).eval()
  loader = BatchLoader(synthetic_dataset(BATCH * n_batches), BATCH, make_collate_fn(dev))
  beam = BeamCTCDecoder(ctc_labels(c2i), beam_width=100, log_probs_input=True)
  runs = {
      "greedy_host": lambda: T.greedy_cer(enc, loader, dev, c2i),
      "greedy_device": lambda: T.device_cer(enc, loader, dev, c2i),
      "beam100_host": lambda: T.ctc_cer(enc, loader, dev, c2i, beam),
      "beam100_device": lambda: T.device_cer(enc, loader, dev, c2i, decoder=beam),
  }
  runs = {k: f for k, f in runs.items() if k.split("_")[1] in arms}

  def timed(f):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
      value = f()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / n_batches, value

  values = {}
  for name, f in runs.items():
    timed(f)
    values[name] = timed(f)[1]
  ms = {name: [] for name in runs}
  for r in range(repeats):
    for name, f in runs.items():
      t, v = timed(f)
      assert v == values[name], (name, v, values[name])
      ms[name].append(t)
    print("repeat %d: %s" % (r, {k: round(v[-1], 3) for k, v in ms.items()}), file=log, flush=True)
  out = {name: dict(_summary(v), cer=values[name]) for name, v in ms.items()}
  for dec in ("greedy", "beam100"):
    if dec + "_host" in out and dec + "_device" in out:
      assert values[dec + "_host"] == values[dec + "_device"], (dec, values)
      out[dec + "_speedup"] = out[dec + "_host"]["median"] / out[dec + "_device"]["median"]
  return out


def time_kernel(dev, calls, log):
  import torch
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.decoder import ctc_labels
  from lipreading_amd.scoring import EditScorer
  sc = EditScorer(ctc_labels(default_char2idx()))
  g = torch.Generator().manual_seed(1)
  out = {}
  for B in (32, 256, 1000):
    hyp = torch.randint(5, 65, (B, T_FRAMES), generator=g, dtype=torch.int32).to(dev)
    ref = torch.randint(5, 65, (B, LABEL_LEN), generator=g, dtype=torch.int32).to(dev)
    hl = torch.randint(T_FRAMES // 2, T_FRAMES + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    rl = torch.full((B,), LABEL_LEN, dtype=torch.int32, device=dev)
    row = {}
    for name, kw in (("char", {}), ("word", {"unit": "word"}), ("char_align", {"align": True})):
      for _ in range(5):
        sc.score(hyp, hl, ref, rl, **kw)
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      torch.cuda.synchronize(dev)
      e0.record()
      for _ in range(calls):
        sc.score(hyp, hl, ref, rl, **kw)
      e1.record()
      torch.cuda.synchronize(dev)
      row[name + "_us_per_call"] = e0.elapsed_time(e1) * 1e3 / calls
    out["pairs_%d" % B] = row
    print("kernel, %d pairs: %s" % (B, {k: round(v, 2) for k, v in row.items()}), file=log, flush=True)
  return out


def count_copies(directory):
  """Copies by direction in a rocprofv3 --memory-copy-trace output under `directory`: the *_memory_copy_trace.csv files
  of the csv format, or the `memory_copies` view of the *_results.db files of the default (rocpd) format."""
  counts = {}
  for path in glob.glob(os.path.join(directory, "**", "*memory_copy_trace.csv"), recursive=True):
    with open(path) as f:
      for row in csv.DictReader(f):
        d = row.get("Direction") or row.get("direction") or "?"
        counts[d] = counts.get(d, 0) + 1
  for path in glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True):
    import sqlite3
    with contextlib.closing(sqlite3.connect(path)) as db:
      for name, n in db.execute("select name, count(*) from memory_copies group by name"):
        counts[name] = counts.get(name, 0) + n
  return counts


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--batches", type=int, default=8)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--calls", type=int, default=200)
  ap.add_argument("--arms", default="host,device")
  ap.add_argument("--no-kernel", action="store_true")
  ap.add_argument("--no-save", action="store_true")
  ap.add_argument("--count-copies", metavar="DIR")
  a = ap.parse_args()
  if a.count_copies:
    print(json.dumps(count_copies(a.count_copies), sort_keys=True))
    return 0
  arms = [x for x in a.arms.split(",") if x]
  if not arms or any(x not in ("host", "device") for x in arms):
    ap.error("--arms takes host, device or both")
  import torch
  if not torch.cuda.is_available():
    print("bench_score: no GPU (this tool never falls back)", file=sys.stderr)
    return 2
  from lipreading_amd import _build
  _build.build_library()
  dev = torch.device("cuda:0")
  doc = {"shape": {"B": BATCH, "T": T_FRAMES, "label_len": LABEL_LEN, "hidden": 256, "batches": a.batches},
         "unit": "ms per batch of the whole evaluation pass (encoder + decoder + scoring)",
         "loops": time_loops(dev, a.batches, a.repeats, arms, sys.stderr)}
  if not a.no_kernel:
    doc["kernel"] = time_kernel(dev, a.calls, sys.stderr)
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(os.path.join(ROOT, "profiles", "score_loop.json"), "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
