"""Attention-decoder beam search: ms per batch and per round of CharDecodingStep.beam_search (lr_decoder_beam_search,
device time by events), launches per round and the rounds run, next to a float32 CPU run of the per-utterance
restatement of tests/test_attn_beam_cpu.py (one oracle call per round over an utterance's live beams, as the
reference's inference() walks one utterance at a time).

  python tools/bench_attn_beam.py [--iters 10] [--cpu-utts 4] [--poll 8] [--ctc-weight W [--pre-beam P]]
                                  [--lm PATH [--lm-alpha A] [--lm-beta B]]

B = 32, T = 75, K = 10, Lmax = 100, V = 64, the three shipped decoder shapes (randomly initialised, so most
hypotheses run to the cap: the worst case of Lmax + 1 rounds).  One JSON line per row and a table at the end.
--ctc-weight W > 0 times the joint CTC/attention search (lr_decoder_joint_beam_search) on the seeded,
peaked, model-like CTC frames of tools/bench_beam.py, with P = --pre-beam candidates per hypothesis (default
min(V - 2, ceil(1.5 K))); the CPU column is then skipped.  W = 0 (the default) keeps today's rows exactly.
--lm PATH (an ARPA file) times the search with a word language model (lr_decoder_lm_beam_search) over
ctc_labels() of the fallback vocabulary, at --ctc-weight W (0: attention plus the model, no CTC frames).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

B, T, K, LMAX, V = 32, 75, 10, 100, 64
SHAPES = [("defaults.txt", "LSTM", "1_layer_nn", 700, 300),
          ("attn", "LSTM", "1_layer_nn", 1024, 300),
          ("ecd", "LSTM", "none", 1536, 300)]
# kernel launches of one round, by the structure of lr_decoder_beam_search's round (lr_attn_beam.hip)
ATTN_LAUNCHES = {"none": 0, "dot": 5, "general": 5, "1_layer_nn": 4, "concat": 6}


def launches_per_round(attn, layers=1):
  return 1 + 2 * layers + (layers - 1) + ATTN_LAUNCHES[attn] + 3   # gather, pack + step, W_ih, attention, head/select/reorder


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--cpu-utts", type=int, default=4, help="utterances of the CPU restatement timed (x B/n)")
  ap.add_argument("--poll", type=int, default=8)
  ap.add_argument("--ctc-weight", type=float, default=0.0)
  ap.add_argument("--pre-beam", type=int, default=None)
  ap.add_argument("--lm", default=None, help="ARPA word language model")
  ap.add_argument("--lm-alpha", type=float, default=0.5)
  ap.add_argument("--lm-beta", type=float, default=0.0)
  a = ap.parse_args()
  import numpy as np
  import torch
  from lipreading_amd import _build
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  from oracle import torch_oracle as O
  from tests.test_attn_beam_cpu import beam_ref
  _build.build_library()
  torch.set_num_threads(min(16, os.cpu_count() or 1))
  dev = torch.device("cuda:0")
  c2i = default_char2idx()
  lm = None
  if a.lm:
    from lipreading_amd.decoder import ctc_labels
    from lipreading_amd.lm import WordLM
    lm = WordLM(a.lm, ctc_labels(c2i), alpha=a.lm_alpha, beta=a.lm_beta)
  rows = []
  for name, rnn_type, attn, Hd, Cd in SHAPES:
    torch.manual_seed(0)
    odec = O.OracleCharDecodingStep(Hd, rnn_type, 1, Cd, V, c2i, attention_type=attn)
    enc_m = VideoEncoder(204, Hd, rnn_type=rnn_type, bidirectional=False)
    dec = CharDecodingStep(enc_m, char_dim=Cd, vocab_size=V, char2idx=c2i, attention_type=attn)
    dec.load_state_dict(odec.state_dict())
    dec = dec.to(dev).eval()
    enc = torch.randn(B, T, Hd)
    lens = torch.randint(T // 2, T + 1, (B,))
    prev = (torch.randn(1, B, Hd) * 0.5, torch.randn(1, B, Hd) * 0.5)
    encd, lensd, prevd = enc.to(dev), lens.to(dev), tuple(p.to(dev) for p in prev)
    joint = {}
    if a.ctc_weight > 0:
      from tools.bench_beam import peaked
      y = torch.tensor(np.log(peaked(np.random.default_rng(0))), device=dev)
      joint = dict(ctc_log_probs=y, ctc_weight=a.ctc_weight, pre_beam=a.pre_beam)
    if lm is not None:
      joint.update(lm=lm, pre_beam=a.pre_beam)
    for _ in range(2):
      dec.beam_search(encd, lensd, prevd, beam_width=K, max_label_len=LMAX, poll_every=a.poll, **joint)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
      dec.beam_search(encd, lensd, prevd, beam_width=K, max_label_len=LMAX, poll_every=a.poll, **joint)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    rounds = dec.beam_rounds
    n = max(1, min(a.cpu_utts, B))
    cpu_ms = float("nan")
    if not joint:
      t0 = time.perf_counter()
      beam_ref(odec, enc[:n], lens[:n], tuple(p[:, :n] for p in prev), K, LMAX, dtype=torch.float32)
      cpu_ms = (time.perf_counter() - t0) * 1e3 * B / n
    row = dict(shape=name, rnn=rnn_type, attention=attn, Hd=Hd, B=B, T=T, K=K, Lmax=LMAX, rounds=rounds,
               gpu_ms_per_batch=round(ms, 3), gpu_us_per_round=round(ms * 1e3 / max(rounds, 1), 1),
               launches_per_round=launches_per_round(attn) + (1 if joint else 0),
               cpu_f32_ms_per_batch=round(cpu_ms, 1) if joint == {} else None, cpu_utts_timed=n if not joint else 0,
               poll_every=a.poll)
    if lm is not None:
      row.update(lm=os.path.basename(a.lm), lm_alpha=a.lm_alpha, lm_beta=a.lm_beta)
    if joint:
      row.update(ctc_weight=a.ctc_weight, pre_beam=a.pre_beam if a.pre_beam is not None else min(V - 2, -(-3 * K // 2)))
    print(json.dumps(row), flush=True)
    rows.append(row)
  print("\n%-13s %6s %8s %10s %10s %9s %12s" % ("shape", "rounds", "ms/batch", "us/round", "launch/rd", "Hd",
                                                "cpu f32 ms"))
  for r in rows:
    print("%-13s %6d %8.2f %10.1f %10d %9d %12.1f" % (r["shape"], r["rounds"], r["gpu_ms_per_batch"],
                                                      r["gpu_us_per_round"], r["launches_per_round"], r["Hd"],
                                                      r["cpu_f32_ms_per_batch"] or float("nan")))


if __name__ == "__main__":
  main()
