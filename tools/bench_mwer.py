#!/usr/bin/env python
"""Measure N-best minimum error rate training (lipreading_amd/mwer.py) at B = 32, T = 75, C = 65 and
N = 4, 8, 16 hypotheses of about 30 characters.  bench.py stays as it is.

  python tools/bench_mwer.py                  # one JSON document on stdout and profiles/mwer.json
  python tools/bench_mwer.py --no-save --repeats 1 --calls 20

Per N, us per call:
  launches_forward / _backward     the two new entries called directly on buffers made once: lr_ctc_nbest_risk (two
                                   kernels) and lr_ctc_nbest_risk_grad (one kernel)
  fused_forward / fused_backward   the same through the front door: nbest_risk_loss and its autograd backward (the
                                   host's share — checks, allocations, the autograd engine — is part of the figure)
  composed_forward / _backward     the only way to the same numbers without them, also called directly on buffers made
                                   once: lr_ctc_nll over the log-probs
                                   repeated N times (B * N rows), torch ops for the softmax and the risk, lr_ctc_grad
                                   with the risk coefficients as sample weights, and the sum over the N copies
  mwer_loss                        one whole MWERLoss call with its backward: beam search (beam_width 100), scoring, loss
  mwer_step / ctc_step             one whole train.mwer_step against one eager train.ctc_step (BiGRU-256)
Protocol: warm-up calls, then `repeats` rounds with the arms alternated; an arm is `calls` calls back to back between
two device events.  Medians and min-max.  The two arms' losses and gradients are compared before anything is timed.

Each N runs in a process of its own under a time limit (--leg-timeout seconds); the first leg that fails or runs out
of time ends the tool.  No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

B, T, C, L = 32, 75, 65, 30
SLOTS = (4, 8, 16)


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


def leg(N, repeats, calls):
  """The measurements of one N: a dict, printed as one JSON line by the child process."""
  import numpy as np
  import torch
  if not torch.cuda.is_available():
    print("bench_mwer: no GPU (this tool never falls back)", file=sys.stderr)
    return None
  import torch.nn.functional as F
  from lipreading_amd import _C, _build
  _build.build_library()
  from lipreading_amd import mwer as M
  from lipreading_amd import train as Tr
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  from tests import mwer_cases as K
  import bench
  dev = torch.device("cuda:0")
  lib = _C.lib()
  case = K.make_case(N, T, C, N, [L] * B)
  lp = F.log_softmax(torch.tensor(case["logits"], device=dev), dim=-1).requires_grad_(True)
  ids, lens = torch.tensor(case["hyp_ids"], device=dev), torch.tensor(case["hyp_lens"], device=dev)
  risk = torch.tensor(case["risk"], device=dev)
  sizes = torch.full((B,), T, dtype=torch.int32, device=dev)
  one = torch.ones((), device=dev)

  # ---- the fused arm
  def fused_forward():
    return M.nbest_risk_loss(lp, sizes, ids, lens, risk)[0]

  def fused_both():
    lp.grad = None
    fused_forward().backward(one)

  # ---- the composed arm: what the tree offered before
  W = ids.shape[2]
  lpN = lp.detach().repeat_interleave(N, dim=0).contiguous()
  labels = ids.reshape(B * N, W).clamp(1, C - 1).contiguous()      # (blank 0: the ids are the shifted labels already)
  fl = sizes.repeat_interleave(N).contiguous()
  ll_ = lens.reshape(B * N).contiguous()
  ws_bytes = lib.lr_ctc_workspace_bytes(B * N, T, C, W)
  ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
  nll = torch.empty(B * N, dtype=torch.float32, device=dev)
  gradN = torch.empty((B * N, T, C), dtype=torch.float32, device=dev)
  head = (lpN.data_ptr(), lpN.stride(0), lpN.stride(1), labels.data_ptr(), labels.stride(0), fl.data_ptr(),
          ll_.data_ptr())

  def composed_forward():
    _C.check(lib.lr_ctc_nll(*head, nll.data_ptr(), ws.data_ptr(), ws_bytes, B * N, T, C, W, _C.stream_handle()))
    p = torch.softmax(-nll.view(B, N), dim=1)
    R = (p * risk).sum(dim=1)
    return R.mean(), p, R

  def composed_both():
    loss, p, R = composed_forward()
    gw = (-(p * (risk - R.unsqueeze(1))) / B).reshape(B * N).contiguous()    # d loss / d nll
    _C.check(lib.lr_ctc_grad(*head, nll.data_ptr(), gw.data_ptr(), gradN.data_ptr(), ws.data_ptr(), ws_bytes, B * N, T,
                             C, W, _C.stream_handle()))
    return loss, gradN.view(B, N, T, C).sum(dim=1)

  # ---- the two new entries called as the composed arm calls the old ones: buffers made once, no autograd
  nb_bytes = lib.lr_ctc_nbest_workspace_bytes(B, T, C, N, W)
  nb_ws = torch.empty(nb_bytes, dtype=torch.uint8, device=dev)
  r_ll, r_post = torch.empty((B, N), device=dev), torch.empty((B, N), device=dev)
  r_utt, r_loss, r_gw = torch.empty(B, device=dev), torch.empty(1, device=dev), torch.empty(B, device=dev)
  r_hs = torch.empty((B, N), dtype=torch.int32, device=dev)
  r_st = torch.empty(1, dtype=torch.int32, device=dev)
  r_grad = torch.empty((B, T, C), device=dev)
  lpd = lp.detach()
  nb_head = (lpd.data_ptr(), lpd.stride(0), lpd.stride(1), sizes.data_ptr(), ids.data_ptr(), ids.stride(0),
             ids.stride(1), lens.data_ptr(), lens.stride(0), risk.data_ptr(), 0, 1)
  nb_tail = (nb_ws.data_ptr(), nb_bytes, B, T, C, N, W)

  def launches_forward():
    _C.check(lib.lr_ctc_nbest_risk(*nb_head, r_ll.data_ptr(), r_post.data_ptr(), r_hs.data_ptr(), r_utt.data_ptr(),
                                   r_loss.data_ptr(), r_st.data_ptr(), r_gw.data_ptr(), *nb_tail, _C.stream_handle()))

  def launches_both():
    launches_forward()
    _C.check(lib.lr_ctc_nbest_risk_grad(*nb_head, r_ll.data_ptr(), r_post.data_ptr(), r_hs.data_ptr(),
                                        r_utt.data_ptr(), r_gw.data_ptr(), None, r_grad.data_ptr(), *nb_tail,
                                        _C.stream_handle()))

  fused_both()
  launches_both()
  loss_c, grad_c = composed_both()
  loss_f = fused_forward().detach()
  assert torch.equal(r_grad, lp.grad) and torch.equal(r_loss.reshape(()), loss_f)     # the front door adds no arithmetic
  scale = float(grad_c.abs().max())
  agree = {"loss_rel": abs(float(loss_f) - float(loss_c)) / abs(float(loss_c)),
           "grad_rel": float((lp.grad - grad_c).abs().max()) / scale}
  assert agree["loss_rel"] < 1e-3 and agree["grad_rel"] < 1e-2, agree     # the same quantity (fp32 against fp64 lattices)

  # ---- the whole loss and the whole step
  labels65 = ctc_labels(default_char2idx())
  dec = BeamCTCDecoder(labels65, beam_width=100, log_probs_input=True)
  whole = M.MWERLoss(dec, nbest=N)
  ref, ref_lens = ids[:, 0].contiguous(), lens[:, 0].contiguous()

  def mwer_loss():
    lp.grad = None
    whole(lp, sizes, ref, ref_lens)[0].backward(one)

  torch.manual_seed(0)
  enc = VideoEncoder(204, 256, rnn_type='GRU', bidirectional=True, enable_ctc=True, vocab_size=64,
                     char2idx=default_char2idx()).to(dev).train()
  opt = FusedAdam(FlatParameters(enc), lr=1e-4)
  frames, fl_h, chars, cl = (x.to(dev) for x in bench.synth_batch(B, 1))

  def mwer_step():
    Tr.mwer_step(enc, opt, whole, frames, fl_h, chars, cl, grad_norm=50, max_len=T)

  def ctc_step():
    Tr.ctc_step(enc, opt, frames, fl_h, chars, cl, grad_norm=50, max_len=T)

  arms = (("launches_forward", launches_forward, calls), ("launches_both", launches_both, calls),
          ("fused_forward", fused_forward, calls), ("fused_both", fused_both, calls),
          ("composed_forward", composed_forward, calls), ("composed_both", composed_both, calls),
          ("mwer_loss", mwer_loss, max(calls // 10, 3)), ("mwer_step", mwer_step, max(calls // 10, 3)),
          ("ctc_step", ctc_step, max(calls // 10, 3)))
  for _, fn, _ in arms:
    for _ in range(3):
      fn()
  times = {name: [] for name, _, _ in arms}
  for r in range(repeats):
    for name, fn, n in arms:
      times[name].append(_timed(torch, n, fn))
    print("N=%d repeat %d: %s" % (N, r, ", ".join("%s %.1f" % (k, v[-1]) for k, v in times.items())),
          file=sys.stderr, flush=True)
  row = {k: _summary(v) for k, v in times.items()}
  for arm in ("launches", "fused", "composed"):
    row[arm + "_backward"] = {"median": row[arm + "_both"]["median"] - row[arm + "_forward"]["median"]}
  row["composed_over_launches"] = row["composed_both"]["median"] / row["launches_both"]["median"]
  row["agreement"] = agree
  row["workspace_bytes"] = {"fused": lib.lr_ctc_nbest_workspace_bytes(B, T, C, N, W), "composed": ws_bytes}
  return row


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--calls", type=int, default=100)
  ap.add_argument("--leg-timeout", type=int, default=240)
  ap.add_argument("--leg", type=int, default=0, help="(internal) run one N in this process and print its JSON line")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mwer.json"))
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args()
  if a.leg:
    row = leg(a.leg, a.repeats, a.calls)
    if row is None:
      return 2
    print("LEG " + json.dumps(row, sort_keys=True))
    return 0
  doc = {"unit": "us per call", "B": B, "T": T, "C": C, "hyp_len": L, "calls": a.calls, "slots": {}}
  for N in SLOTS:
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", str(N), "--repeats", str(a.repeats), "--calls",
           str(a.calls)]
    try:
      res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
    except subprocess.TimeoutExpired:
      print("bench_mwer: N=%d ran past %d s; stopping" % (N, a.leg_timeout), file=sys.stderr)
      return 3
    sys.stderr.write(res.stderr)
    lines = [l for l in res.stdout.splitlines() if l.startswith("LEG ")]
    if res.returncode != 0 or not lines:
      print("bench_mwer: N=%d failed (exit %d); stopping" % (N, res.returncode), file=sys.stderr)
      return res.returncode or 1
    doc["slots"]["N%d" % N] = json.loads(lines[-1][4:])
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(a.out, "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
