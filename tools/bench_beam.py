"""CTC prefix beam search: ms per batch of lr_ctc_beam_decode (BeamCTCDecoder.decode_ids, device time by events, and
decode() end to end with its one device->host copy and the strings) next to the float64 CPU restatement of
tests/test_beam_cpu.py spread over a process pool.

  python tools/bench_beam.py [--iters 50] [--threads 16] [--cpu-batches 1] [--lm model.arpa [--alpha A --beta B]]
                             [--hotwords N [--hotword-weight X]]

B = 32, T = 75, C = 65 (the fallback vocabulary), model-like peaked frames; (W, n) in
{(1,1), (8,40), (100,40), (128,64)}.  With --lm the same rows follow again with the ARPA language model
(lr_ctc_beam_lm_decode; ctc_labels() of the fallback vocabulary, whose ' ' separates words; GPU columns only).
With --hotwords N the plain rows follow again with N seeded hotwords of 3-8 random classes (lr_ctc_beam_bias_decode,
not anchored: these labels have no ' '), each beside the plain row of the same run; with --lm too, the LM rows
follow with the hotwords anchored (lr_ctc_beam_lm_bias_decode).  One JSON line per row and a table at the end.
"""
import argparse
import json
import os
import sys
import time
import multiprocessing
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

B, T, C = 32, 75, 65
SHAPES = [(1, 1), (8, 40), (100, 40), (128, 64)]


def peaked(rng):
  x = rng.standard_normal((B, T, C)) * 0.8
  for b in range(B):
    t = 0
    while t < T:
      run = int(rng.integers(1, 5))
      c = 0 if rng.random() < 0.5 else int(rng.integers(1, C))
      x[b, t:t + run, c] += rng.uniform(3.0, 7.0)
      t += run
  x = np.exp(x - x.max(2, keepdims=True))
  return (x / x.sum(2, keepdims=True)).astype(np.float32)


def _ref_one(args):
  from tests.test_beam_cpu import beam_ref
  v, W, n = args
  return beam_ref(v, T, W, n)


def time_gpu(dec, pd, iters):
  """(decode_ids ms by events, decode() ms by wall clock), each per batch."""
  import torch
  for _ in range(5):
    dec.decode_ids(pd)
  torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(iters):
    dec.decode_ids(pd)
  e1.record()
  torch.cuda.synchronize()
  gpu_ms = e0.elapsed_time(e1) / iters
  t0 = time.perf_counter()
  for _ in range(iters):
    dec.decode(pd)
  return gpu_ms, (time.perf_counter() - t0) * 1e3 / iters


def random_hotwords(labels, count, seed=1):
  """`count` distinct strings of 3-8 one-character labels (never the blank's or ' ')."""
  rng = np.random.default_rng(seed)
  chars = [l for l in labels[1:] if len(l) == 1 and l != " "]
  out = set()
  while len(out) < count:
    out.add("".join(rng.choice(chars, int(rng.integers(3, 9)))))
  return sorted(out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--threads", type=int, default=16)
  ap.add_argument("--cpu-batches", type=int, default=1)
  ap.add_argument("--lm", default=None, help="an ARPA file: add rows with the language model")
  ap.add_argument("--alpha", type=float, default=0.5)
  ap.add_argument("--beta", type=float, default=1.0)
  ap.add_argument("--hotwords", type=int, default=0, help="N: add rows with N random hotwords")
  ap.add_argument("--hotword-weight", type=float, default=10.0)
  a = ap.parse_args()
  import torch
  from lipreading_amd import _build
  from lipreading_amd.decoder import BeamCTCDecoder
  _build.build_library()
  dev = torch.device("cuda:0")
  p = peaked(np.random.default_rng(0))
  pd = torch.tensor(p, device=dev)
  labels = ["_"] + [chr(ord("!") + i) for i in range(C - 1)]
  rows = []
  # spawned workers: fresh interpreters that never touch the GPU (a fork would inherit this process's device handles)
  with multiprocessing.get_context("spawn").Pool(a.threads) as pool:
    pool.map(_ref_one, [(p[b], 1, 1) for b in range(B)])   # start the workers outside the timed region
    for W, n in SHAPES:
      dec = BeamCTCDecoder(labels, beam_width=W, cutoff_top_n=n)
      for _ in range(5):
        dec.decode_ids(pd)
      torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(a.iters):
        dec.decode_ids(pd)
      e1.record()
      torch.cuda.synchronize()
      gpu_ms = e0.elapsed_time(e1) / a.iters
      t0 = time.perf_counter()
      for _ in range(a.iters):
        dec.decode(pd)
      e2e_ms = (time.perf_counter() - t0) * 1e3 / a.iters
      t0 = time.perf_counter()
      for _ in range(a.cpu_batches):
        pool.map(_ref_one, [(p[b], W, n) for b in range(B)])
      cpu_ms = (time.perf_counter() - t0) * 1e3 / a.cpu_batches
      row = dict(W=W, n=n, B=B, T=T, C=C, gpu_decode_ids_ms=round(gpu_ms, 4), gpu_decode_ms=round(e2e_ms, 4),
                 cpu_ref_ms=round(cpu_ms, 2), cpu_threads=a.threads)
      rows.append(row)
      print(json.dumps(row), flush=True)
  if a.lm:
    from lipreading_amd.data import default_char2idx
    from lipreading_amd.decoder import ctc_labels
    lm_labels = ctc_labels(default_char2idx())
    assert len(lm_labels) == C
    for W, n in SHAPES:
      dec = BeamCTCDecoder(lm_labels, lm_path=a.lm, alpha=a.alpha, beta=a.beta, beam_width=W, cutoff_top_n=n)
      gpu_ms, e2e_ms = time_gpu(dec, pd, a.iters)
      row = dict(W=W, n=n, B=B, T=T, C=C, lm=os.path.basename(a.lm), lm_order=dec.lm.order,
                 lm_ngrams=int(sum(dec.lm.counts)), gpu_decode_ids_ms=round(gpu_ms, 4),
                 gpu_decode_ms=round(e2e_ms, 4))
      rows.append(row)
      print(json.dumps(row), flush=True)
  if a.hotwords:
    plain = {(r["W"], r["n"]): r["gpu_decode_ids_ms"] for r in rows if "lm" not in r}
    with_lm = {(r["W"], r["n"]): r["gpu_decode_ids_ms"] for r in rows if "lm" in r}
    for W, n in SHAPES:
      dec = BeamCTCDecoder(labels, beam_width=W, cutoff_top_n=n, hotwords=random_hotwords(labels, a.hotwords),
                           hotword_weight=a.hotword_weight, hotword_anchor=False)
      gpu_ms, e2e_ms = time_gpu(dec, pd, a.iters)
      row = dict(W=W, n=n, B=B, T=T, C=C, hotwords=a.hotwords, gpu_decode_ids_ms=round(gpu_ms, 4),
                 gpu_decode_ms=round(e2e_ms, 4), plain_decode_ids_ms=plain[(W, n)])
      rows.append(row)
      print(json.dumps(row), flush=True)
    for W, n in SHAPES if a.lm else []:
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # random strings are no words of the model: only the lookups are timed
        dec = BeamCTCDecoder(lm_labels, lm_path=a.lm, alpha=a.alpha, beta=a.beta, beam_width=W, cutoff_top_n=n,
                             hotwords=random_hotwords(lm_labels, a.hotwords), hotword_weight=a.hotword_weight)
      gpu_ms, e2e_ms = time_gpu(dec, pd, a.iters)
      row = dict(W=W, n=n, B=B, T=T, C=C, hotwords=a.hotwords, lm=os.path.basename(a.lm),
                 gpu_decode_ids_ms=round(gpu_ms, 4), gpu_decode_ms=round(e2e_ms, 4),
                 plain_decode_ids_ms=with_lm[(W, n)])
      rows.append(row)
      print(json.dumps(row), flush=True)
  print("\n| W | n | GPU decode_ids ms | GPU decode() ms | CPU restatement ms (%d procs) |" % a.threads)
  print("|---|---|---|---|---|")
  for r in rows:
    if "lm" in r or "hotwords" in r:
      continue
    print("| %d | %d | %.3f | %.3f | %.1f |" % (r["W"], r["n"], r["gpu_decode_ids_ms"], r["gpu_decode_ms"],
                                               r["cpu_ref_ms"]))
  if a.lm:
    print("\nwith the language model %s:\n| W | n | GPU decode_ids ms | GPU decode() ms |\n|---|---|---|---|" % a.lm)
    for r in rows:
      if "lm" in r and "hotwords" not in r:
        print("| %d | %d | %.3f | %.3f |" % (r["W"], r["n"], r["gpu_decode_ids_ms"], r["gpu_decode_ms"]))
  if a.hotwords:
    print("\nwith %d hotwords:\n| W | n | LM | decode_ids ms, no hotwords | decode_ids ms, hotwords | ratio |\n"
          "|---|---|---|---|---|---|" % a.hotwords)
    for r in rows:
      if "hotwords" in r:
        print("| %d | %d | %s | %.3f | %.3f | %.2f |" % (r["W"], r["n"], r.get("lm", "-"), r["plain_decode_ids_ms"],
                                                        r["gpu_decode_ids_ms"],
                                                        r["gpu_decode_ids_ms"] / r["plain_decode_ids_ms"]))


if __name__ == "__main__":
  main()
