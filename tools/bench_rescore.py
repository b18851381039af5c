"""Attention rescoring of CTC N-best lists (CharDecodingStep.rescore, lr_decoder_rescore): ms per call
(device time by events, median of --reps windows after a warm-up of every shape) next to the two ways the same
question was answered before:

  tiled   decode_sequence on enc / lens / state tiled N times, then the gather of each target's log-probability, the
          per-hypothesis sum, the weighted score and the sort, all in torch: the same N-best order, through
          [B*N][L][V] log-probabilities and N copies of the encoder states;
  joint   the one-pass alternative, beam_search(ctc_log_probs=...) at K = N (its rounds run to the cap on random
          weights; K <= 32).

  python tools/bench_rescore.py [--iters 10] [--reps 5] [--out PATH.json]

B in {1, 8, 32}, N in {4, 10, 32}, T = 75, W = 40, V = 64; the decoder sizes the flag files ship: GRU-256 with dot
attention, LSTM-1024 (1_layer_nn) and LSTM-1536 (none), char_dim 256.  The three are timed alternately inside each
repetition.  The outputs of `rescore` and `tiled` are compared on the same inputs before anything is timed.  One JSON
line per row and a table at the end.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

T, W, V, CD = 75, 40, 64, 256
SHAPES = [("gru256", "GRU", "dot", 256), ("lstm1024", "LSTM", "1_layer_nn", 1024), ("lstm1536", "LSTM", "none", 1536)]
BS, NS = (1, 8, 32), (4, 10, 32)
LAM, GAMMA = 0.3, 0.0


def hypotheses(B, N, seed):
  """Model-like N-best lists: lengths 10 .. W of character classes, ascending first-pass scores, no empty slot."""
  import numpy as np
  import torch
  g = np.random.RandomState(seed)
  ids = -np.ones((B, N, W), dtype=np.int32)
  lens = g.randint(10, W + 1, size=(B, N)).astype(np.int32)
  for b in range(B):
    for n in range(N):
      ids[b, n, :lens[b, n]] = g.randint(4, V, size=lens[b, n]) + 1
  first = np.sort(g.uniform(5.0, 60.0, size=(B, N)).astype(np.float32), axis=1)
  return torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(first)


def tiled(dec, enc, lens, prev, ids, hl, first, eos, bos, pad):
  """The parent commit's composition, on the device: -> (order, scores, attn) as rescore returns them."""
  import torch
  B, N, _ = ids.shape
  L = W + 1
  tok = (ids - 1).clamp(min=0)
  at = torch.arange(L, device=ids.device)[None, None, :]
  tgt = torch.cat((tok, tok.new_zeros(B, N, 1)), 2)
  tgt = torch.where(at == hl[:, :, None], torch.full_like(tgt, eos), tgt)          # the appended EOS (no EOS inside)
  live = at <= hl[:, :, None]
  inp = torch.cat((tgt.new_full((B, N, 1), bos), tgt[:, :, :-1]), 2)
  inp = torch.where(live, inp, torch.full_like(inp, pad)).view(B * N, L)
  tile = lambda t, d: t.repeat_interleave(N, dim=d)
  state = tuple(tile(p, 1) for p in prev) if isinstance(prev, tuple) else tile(prev, 1)
  lp = dec.decode_sequence(inp.to(torch.int32), state, tile(lens, 0), tile(enc, 0))[0]      # [B*N][L][V]
  terms = lp.view(B, N, L, V).gather(3, tgt.long()[..., None])[..., 0].double()
  a = (terms * live).sum(2)
  s = (1.0 - LAM) * a - LAM * first.double() + GAMMA * (hl + 1)
  order = torch.sort(s, dim=1, descending=True, stable=True)[1]
  return order.to(torch.int32), torch.gather(s, 1, order).float(), torch.gather(a, 1, order).float()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  import numpy as np
  import torch
  from lipreading_amd import _build
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import BOS, EOS, PAD, default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  _build.build_library()
  assert torch.cuda.is_available(), "the benchmark times the MI355X: there is nothing to measure without it"
  dev = torch.device("cuda:0")
  c2i = default_char2idx()
  bos, eos, pad = c2i[BOS], c2i[EOS], c2i[PAD]
  rows = []

  def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
      fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.iters

  for name, rnn_type, attn, Hd in SHAPES:
    torch.manual_seed(0)
    enc_m = VideoEncoder(204, Hd, rnn_type=rnn_type, bidirectional=False)
    dec = CharDecodingStep(enc_m, char_dim=CD, vocab_size=V, char2idx=c2i, attention_type=attn).to(dev).eval()
    for B in BS:
      for N in NS:
        g = torch.Generator().manual_seed(B * 100 + N)
        enc = torch.randn(B, T, Hd, generator=g).to(dev)
        lens = torch.randint(T // 2, T + 1, (B,), generator=g).to(dev)
        lens[0] = T
        h = (torch.randn(1, B, Hd, generator=g) * 0.5).to(dev)
        prev = (h, (torch.randn(1, B, Hd, generator=g) * 0.5).to(dev)) if rnn_type == "LSTM" else h
        ids, hl, first = (t.to(dev) for t in hypotheses(B, N, B * 100 + N))
        y = torch.log_softmax(torch.randn(B, T, V + 1, generator=g) * 3.0, dim=2).to(dev)
        with torch.no_grad():
          new = lambda: dec.rescore(enc, lens, prev, ids, hl, first, ctc_weight=LAM, length_bonus=GAMMA)
          old = lambda: tiled(dec, enc, lens, prev, ids, hl, first, eos, bos, pad)
          one = lambda: dec.beam_search(enc, lens, prev, beam_width=N, max_label_len=W, ctc_log_probs=y,
                                        ctc_weight=LAM)
          runs = [("rescore", new), ("tiled", old), ("joint", one)]
          got, want = new(), old()
          torch.cuda.synchronize()
          # the same answer first: two float32 runs of the same sums (tests/test_gpu_rescore.py holds each to its bound
          # against float64; here the difference is recorded and only a gross disagreement stops the run)
          err = float((got[2].double().sort(dim=1)[0] - want[2].double().sort(dim=1)[0]).abs().max())
          assert err <= 1e-3, (name, B, N, err)
          same_order = bool(torch.equal(got[0], want[0]))
          for _, fn in runs:   # warm-up of every shape the windows use
            for _ in range(2):
              fn()
          torch.cuda.synchronize()
          ms = {k: [] for k, _ in runs}
          for _ in range(a.reps):
            for k, fn in runs:
              ms[k].append(window(fn))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        row = dict(shape=name, rnn=rnn_type, attention=attn, Hd=Hd, B=B, N=N, T=T, W=W, V=V,
                   rescore_ms=round(med["rescore"], 3), tiled_ms=round(med["tiled"], 3), joint_ms=round(med["joint"], 3),
                   tiled_over_rescore=round(med["tiled"] / med["rescore"], 2),
                   joint_over_rescore=round(med["joint"] / med["rescore"], 2),
                   rescore_spread=round((max(ms["rescore"]) - min(ms["rescore"])) / med["rescore"], 3),
                   max_abs_diff_attn=err, same_order=same_order, iters=a.iters, reps=a.reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
  print("\n%-9s %3s %3s %11s %9s %9s %13s %13s" % ("shape", "B", "N", "rescore ms", "tiled ms", "joint ms",
                                                  "tiled/rescore", "joint/rescore"))
  for r in rows:
    print("%-9s %3d %3d %11.3f %9.3f %9.3f %13.2f %13.2f" % (r["shape"], r["B"], r["N"], r["rescore_ms"], r["tiled_ms"],
                                                           r["joint_ms"], r["tiled_over_rescore"],
                                                           r["joint_over_rescore"]))
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
