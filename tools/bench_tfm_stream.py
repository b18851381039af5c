#!/usr/bin/env python
"""Measure transformer encoder sessions (TransformerVideoEncoder.stream, lr_tfm_stream_*) against the
only thing there was without them — TransformerVideoEncoder.forward re-run at every chunk — in the same process, and the
one-shot training step under the chunk mask against the step without it.  bench.py stays as it is.

  python tools/bench_tfm_stream.py                   # one JSON document on stdout and profiles/tfm_stream.json
  python tools/bench_tfm_stream.py --no-save --repeats 3 --calls 3 --dims 204

The bench's encoder (d_model 256, 4 heads, 4 layers, feed-forward 1024, CTC head) at frame_dim I = 204 (landmarks) and
3456 (conv features of 96 x 96 crops), clips of T = 75 frames, attention chunk C in {4, 8, 16}, left context Lc in
{1, 3}, 1 and 8 slots.  Arms, us per call:
  session      a session reset and fed the clip C frames at a time (ceil(75 / C) advances, the last one ends the stream)
  reset        the reset alone
  prefix[m]    forward over the growing prefixes C, 2C, ... 75 — what a live caller had to do for exact results
  window[m]    forward over the last (Lc + 1) * C frames at every chunk — the approximation a live caller could afford
               (m = f32: exact fp32 products and softmax, the session's own arithmetic; fast: split-bf16 products and the
               fused bf16 attention, the pixel regime's one-shot modes)
From them: us per advance = (session - reset) / advances, and session over prefix / window per advance.
The training step: bench.py's --regime pixels_tfm step (train.ctc_step on the bench's model, batch and clips) with
attn_chunk = 8, attn_left_chunks = 3 against attn_chunk = 0, alternated, ms per step.
Protocol: warm-up calls of every arm, then `repeats` rounds with the arms alternated; an arm is `calls` calls back to back
between two device events.  Medians and min-max.  The session's rows are compared with the one-shot forward's before
anything is timed.  No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
  if p not in sys.path:
    sys.path.insert(0, p)

T = 75
DIMS = (204, 3456)
CHUNKS = (4, 8, 16)
LEFTS = (1, 3)
BATCHES = (1, 8)


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


def _alternate(torch, arms, repeats, calls):
  for fn in arms.values():
    for _ in range(2):
      fn()
  seen = {k: [] for k in arms}
  for _ in range(repeats):
    for k, fn in arms.items():
      seen[k].append(_timed(torch, calls, fn))
  return {k: _summary(v) for k, v in seen.items()}


def measure(torch, enc, B, C, Lc, repeats, calls):
  dev = torch.device("cuda:0")
  enc.attn_chunk, enc.attn_left_chunks = C, Lc
  frames = torch.randn(B, T, enc.frame_dim, generator=torch.Generator().manual_seed(B)).to(dev)
  lens = {t: torch.full((B,), t, dtype=torch.int32, device=dev) for t in range(1, T + 1)}
  st = enc.stream(B, dev)
  cuts = list(range(0, T, C))
  ends = [torch.full((B,), int(t0 + C >= T), dtype=torch.int32, device=dev) for t0 in cuts]

  def session():
    st.reset()
    return [st.feed(frames[:, t0:t0 + C], end=e) for t0, e in zip(cuts, ends)]

  def forward(mode, t0, t1):
    enc.input_projection, enc.attention = ('f32', 'f32') if mode == "f32" else ('bf16x3', 'bf16')
    with torch.no_grad():
      return enc(frames[:, t0:t1], lens[t1 - t0], max_len=t1 - t0)[0]

  def prefix(mode):
    for t0 in cuts:
      forward(mode, 0, min(T, t0 + C))

  def window(mode):
    for t0 in cuts:
      t1 = min(T, t0 + C)
      forward(mode, max(0, t1 - (Lc + 1) * C), t1)

  got = torch.cat([lp[:, :C] for lp, _ in session()], dim=1)[:, :T]
  err = float((forward("f32", 0, T) - got).abs().max())
  assert err < 1e-3, err
  arms = {"session": session, "reset": st.reset}
  for m in ("f32", "fast"):
    arms["prefix[%s]" % m] = lambda m=m: prefix(m)
    arms["window[%s]" % m] = lambda m=m: window(m)
  out = _alternate(torch, arms, repeats, calls)
  enc.input_projection, enc.attention = 'f32', 'f32'
  n = len(cuts)
  out["advances"] = n
  out["max_abs_diff_to_forward_f32"] = err
  out["us_per_advance"] = (out["session"]["median"] - out["reset"]["median"]) / n
  for k in ("prefix[f32]", "prefix[fast]", "window[f32]", "window[fast]"):
    out["us_per_chunk_" + k] = out[k]["median"] / n
    out["session_over_" + k] = (out["session"]["median"] - out["reset"]["median"]) / out[k]["median"]
  return out


def training_step(torch, repeats, calls):
  """bench.py's pixels_tfm step, the same objects, attn_chunk 8 / 3 against 0: ms per step"""
  import bench
  from lipreading_amd import train as Tr
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.frontend import ConvFrontend3D, PixelLipReader, feature_dim
  from lipreading_amd.optim import FlatParameters, FusedAdam
  from lipreading_amd.transformer import TransformerVideoEncoder
  dev = torch.device("cuda:0")
  B = 32
  torch.manual_seed(123456)
  enc = TransformerVideoEncoder(feature_dim(bench.IMG, bench.IMG), d_model=256, nhead=4, num_layers=4,
                                dim_feedforward=1024, enable_ctc=True, vocab_size=bench.VOCAB, char2idx=default_char2idx())
  model = PixelLipReader(enc, ConvFrontend3D()).to(dev).train()
  opt = FusedAdam(FlatParameters(model), lr=1e-4)
  opt.sum_squares_early(model.encoder)
  _, frame_lens, chars, char_lens = bench.synth_batch(B, 123456, dev)
  clips = bench.synth_clips(B, 123456, dev)
  graphs = Tr.StepGraphs(enabled=False)

  def step(chunk, left):
    enc.attn_chunk, enc.attn_left_chunks = chunk, left
    Tr.ctc_step(model, opt, clips, frame_lens, chars, char_lens, grad_norm=50, max_len=bench.T_FRAMES, graphs=graphs)

  out = _alternate(torch, {"attn_chunk=0": lambda: step(0, 0), "attn_chunk=8": lambda: step(8, 3)}, repeats, calls)
  for v in out.values():
    for k in ("median", "min", "max"):
      v[k] /= 1e3
  out["unit"] = "ms"
  out["batch"] = B
  out["chunk8_over_chunk0"] = out["attn_chunk=8"]["median"] / out["attn_chunk=0"]["median"]
  return out


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--calls", type=int, default=5)
  ap.add_argument("--dims", type=int, nargs="*", default=list(DIMS))
  ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
  ap.add_argument("--no-train", action="store_true")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tfm_stream.json"))
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    print("bench_tfm_stream: no GPU (this tool never falls back)", file=sys.stderr)
    return 1
  from lipreading_amd import _build
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.transformer import TransformerVideoEncoder
  _build.build_library()
  dev = torch.device("cuda:0")
  c2i = default_char2idx()
  doc = dict(shape=dict(T=T, d_model=256, nhead=4, layers=4, feedforward=1024, classes=len(c2i) + 1), unit="us",
             repeats=a.repeats, calls=a.calls, device=torch.cuda.get_device_name(0), sessions={})
  for I in a.dims:
    torch.manual_seed(0)
    enc = TransformerVideoEncoder(I, d_model=256, nhead=4, num_layers=4, dim_feedforward=1024, enable_ctc=True,
                                  vocab_size=len(c2i), char2idx=c2i, attn_chunk=8, attn_left_chunks=1).to(dev).eval()
    for B in a.batches:
      for C in CHUNKS:
        for Lc in LEFTS:
          key = "I=%d B=%d C=%d Lc=%d" % (I, B, C, Lc)
          r = doc["sessions"][key] = measure(torch, enc, B, C, Lc, a.repeats, a.calls)
          print("%-24s %7.0f us/advance | per chunk: prefix f32 %7.0f fast %7.0f  window f32 %7.0f fast %7.0f" % (
              key, r["us_per_advance"], r["us_per_chunk_prefix[f32]"], r["us_per_chunk_prefix[fast]"],
              r["us_per_chunk_window[f32]"], r["us_per_chunk_window[fast]"]), file=sys.stderr, flush=True)
  if not a.no_train:
    r = doc["training_step_pixels_tfm"] = training_step(torch, a.repeats, max(a.calls, 10))
    print("pixels_tfm step: attn_chunk=0 %.3f ms, attn_chunk=8 %.3f ms (ratio %.3f)" % (
        r["attn_chunk=0"]["median"], r["attn_chunk=8"]["median"], r["chunk8_over_chunk0"]), file=sys.stderr, flush=True)
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(a.out, "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
