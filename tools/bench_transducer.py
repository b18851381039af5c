#!/usr/bin/env python
"""Measure the transducer head (lipreading_amd/transducer.py) at T = 75, U = 40, V1 = 65, J = 256 for
B = 1, 8, 32.  bench.py stays as it is.

  python tools/bench_transducer.py                  # one JSON line on stdout and profiles/transducer.json
  python tools/bench_transducer.py --no-save --repeats 1 --calls 5

Per B, us per call:
  fused_forward / fused_forward_backward   rnnt_loss through the front door (joint stage, alpha, reduction) and with its
                                           autograd backward (beta, the tiles' gradients, the combine)
  composed_forward / _forward_backward     the joint stage's arithmetic from torch device ops: broadcast add, tanh,
                                           matmul, log_softmax and the gather of the two log-probabilities a node needs
                                           (a (B, T, U+1, V1) and a (B, T, U+1, J) tensor exist); backward from random
                                           gradients of the gathered values.  The lattice is NOT in this arm: it is left
                                           to the new kernel, so the fused arm does strictly more
  greedy                                   one rnnt_greedy launch over the batch (random weights: the transcript length
                                           it decodes is reported beside it)
and once, at B = 32: transducer_step against an eager ctc_step on BiGRU-256 (ms per step, and the difference).
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

T, U, V1, J = 75, 40, 65, 256
BATCHES = (1, 8, 32)


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
    for _ in range(3):
      fn()
  out = {k: [] for k in arms}
  for _ in range(repeats):
    for k, fn in arms.items():
      out[k].append(_timed(torch, calls, fn))
  return {k: _summary(v) for k, v in out.items()}


def kernel_leg(torch, B, repeats, calls):
  from lipreading_amd import transducer as TR
  dev = torch.device("cuda")
  g = torch.Generator().manual_seed(B)
  r = lambda *s: torch.randn(*s, generator=g).to(dev)
  e, p = r(B, T, J).requires_grad_(True), r(B, U + 1, J).requires_grad_(True)
  W, b = (r(V1, J) * (3.0 / J ** 0.5)).requires_grad_(True), (r(V1) * 0.1).requires_grad_(True)
  mask = torch.ones(V1, device=dev)
  mask[2] = mask[5] = 0
  allowed = torch.tensor([c for c in range(1, V1) if c not in (2, 5)])
  labels = allowed[torch.randint(0, len(allowed), (B, U), generator=g)].to(torch.int32).to(dev)
  flens = torch.full((B,), T, dtype=torch.int32, device=dev)
  llens = torch.full((B,), U, dtype=torch.int32, device=dev)
  tables = r(2, V1, J) * 0.7
  gb, gl = r(B, T, U + 1), r(B, T, U)
  idx = labels.long()[:, None, :, None].expand(B, T, U, 1)

  def fused(backward):
    loss, _, _ = TR.rnnt_loss(e, p, W, b, mask, labels, flens, llens)
    if backward:
      for x in (e, p, W, b):
        x.grad = None
      loss.backward()

  def composed(backward):
    z = torch.tanh(e[:, :, None, :] + p[:, None, :, :])
    lp = torch.log_softmax((z @ W.t() + b).masked_fill(mask == 0, float("-inf")), dim=-1)
    blank, lab = lp[..., 0], lp[:, :, :U].gather(3, idx)[..., 0]
    if backward:
      for x in (e, p, W, b):
        x.grad = None
      torch.autograd.backward([blank, lab], [gb, gl])

  with torch.no_grad():
    bias0 = b.detach().clone()
    bias0[0] += 2.0
    dec = TR.rnnt_greedy(e.detach(), flens, tables, W.detach(), bias0, mask)
  arms = {"fused_forward": lambda: fused(False), "composed_forward": lambda: composed(False),
          "fused_forward_backward": lambda: fused(True), "composed_forward_backward": lambda: composed(True),
          "greedy": lambda: TR.rnnt_greedy(e.detach(), flens, tables, W.detach(), bias0, mask)}
  out = _rounds(torch, arms, repeats, calls)
  out["greedy_symbols_per_clip"] = float(dec["lens"].float().mean())
  out["B"] = B
  return out


def step_leg(torch, repeats, calls):
  import numpy as np
  from lipreading_amd import train as TN
  from lipreading_amd import transducer as TR
  from lipreading_amd.data import default_char2idx, make_collate_fn
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  dev = torch.device("cuda")
  c2i = default_char2idx()
  rng = np.random.RandomState(0)
  items = [(rng.randn(T, 68, 3).astype(np.float32), np.r_[1, rng.randint(4, 64, U - 1), 2]) for _ in range(32)]
  frames, frame_lens, chars, char_lens = make_collate_fn(dev)(items)
  torch.manual_seed(0)

  def encoder():
    return VideoEncoder(204, 256, rnn_type='GRU', bidirectional=True, enable_ctc=True, vocab_size=64,
                        char2idx=c2i).to(dev).train()
  enc_c, enc_t = encoder(), encoder()
  head = TR.TransducerHead(512, 64, c2i, joint_dim=J, embed_dim=64, context=2).to(dev).train()
  opt_c = FusedAdam(FlatParameters(enc_c), lr=1e-4)
  opts = (FusedAdam(FlatParameters(enc_t), lr=1e-4), FusedAdam(FlatParameters(head), lr=1e-4))
  arms = {"ctc_step": lambda: TN.ctc_step(enc_c, opt_c, frames, frame_lens, chars, char_lens, grad_norm=50, max_len=T),
          "transducer_step": lambda: TN.transducer_step(enc_t, head, opts, frames, frame_lens, chars, char_lens,
                                                        grad_norm=50, max_len=T)}
  out = _rounds(torch, arms, repeats, calls)
  out["delta_us"] = out["transducer_step"]["median"] - out["ctc_step"]["median"]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--calls", type=int, default=20)
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args()
  import torch
  if not torch.cuda.is_available():
    print("bench_transducer: no GPU (this tool never falls back)", file=sys.stderr)
    return 1
  doc = {"tool": "bench_transducer", "shape": {"T": T, "U": U, "V1": V1, "J": J}, "unit": "us per call",
         "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls": a.calls,
         "batches": [kernel_leg(torch, B, a.repeats, a.calls) for B in BATCHES],
         "step_bigru256_b32": step_leg(torch, a.repeats, a.calls)}
  line = json.dumps(doc, sort_keys=True)
  print(line)
  if not a.no_save:
    with open(os.path.join(ROOT, "profiles", "transducer.json"), "w") as f:
      f.write(line + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
