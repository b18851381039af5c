#!/usr/bin/env python
"""Measure resumable encoder sessions (VideoEncoder.stream, lr_rnn_stream_*) against VideoEncoder.forward
on the same utterances in the same process.  bench.py stays as it is.

  python tools/bench_encoder_stream.py                   # one JSON document on stdout and profiles/encoder_stream.json
  python tools/bench_encoder_stream.py --no-save --repeats 3 --calls 5 --batches 1

Uni-directional GRU-256 x1 / x2 and LSTM-700 x1 at I = 204, C = 65, B in {1, 8, 32}, T = 75, head included.  Arms, us per
call:
  session[N]     a session reset and fed the 75 frames in chunks of N = 75, 25, 5, 1 frames (75 / N advances)
  reset          the reset alone
  forward[r]     VideoEncoder.forward over the whole utterance once, recurrence r = 'f32' and 'auto'
  prefix[N]      the prefix re-encode total, the only way without a session: VideoEncoder.forward (recurrence 'auto')
                 over the growing prefixes N, 2N, ... 75
From them: us per advance = (session - reset) / advances, us per frame = that / N, and session[N] / prefix[N].
Protocol: warm-up calls, then `repeats` rounds with the arms alternated; an arm is `calls` calls back to back between
two device events.  Medians and min-max.  Every chunking's log-probabilities and state are compared, bit for bit, with
the one-chunk session's before anything is timed.  No GPU, no numbers: the tool exits non-zero without one.
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

T, I = 75, 204
CHUNKS = (75, 25, 5, 1)
MODELS = (("GRU", 256, 1), ("GRU", 256, 2), ("LSTM", 700, 1))
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


def measure(torch, enc, B, repeats, calls):
  dev = torch.device("cuda:0")
  frames = torch.randn(B, T, I, generator=torch.Generator().manual_seed(B)).to(dev)
  lens = {t: torch.full((B,), t, dtype=torch.int32, device=dev) for t in range(1, T + 1)}
  st = enc.stream(B, dev)

  def session(n):
    st.reset()
    return torch.cat([st.feed(frames[:, t0:t0 + n]) for t0 in range(0, T, n)], dim=1)

  def forward(recurrence, t=T):
    enc.recurrence = recurrence
    with torch.no_grad():
      return enc(frames[:, :t], lens[t], max_len=t)[0]

  def prefix(n):
    for t in range(n, T + 1, n):
      forward('auto', t)

  # the same bits before anything is timed; the one-shot forward agrees to its own accuracy
  want, want_state = session(T), st.state_buf.clone()
  for n in CHUNKS:
    assert torch.equal(session(n), want) and torch.equal(st.state_buf, want_state), "chunks of %d differ" % n
  err = float((forward('f32') - want).abs().max())
  assert err < 1e-3, err
  arms = {"reset": st.reset, "forward[f32]": lambda: forward('f32'), "forward[auto]": lambda: forward('auto')}
  arms.update({"session[%d]" % n: (lambda n=n: session(n)) for n in CHUNKS})
  arms.update({"prefix[%d]" % n: (lambda n=n: prefix(n)) for n in CHUNKS})
  for fn in arms.values():
    for _ in range(2):
      fn()
  seen = {k: [] for k in arms}
  for _ in range(repeats):
    for k, fn in arms.items():
      seen[k].append(_timed(torch, calls, fn))
  out = {k: _summary(seen[k]) for k in ("reset", "forward[f32]", "forward[auto]")}
  out["max_abs_diff_to_forward_f32"] = err
  out["chunks"] = {}
  for n in CHUNKS:
    s, p = _summary(seen["session[%d]" % n]), _summary(seen["prefix[%d]" % n])
    advances = -(-T // n)
    per_advance = (s["median"] - out["reset"]["median"]) / advances
    out["chunks"][str(n)] = dict(session=s, prefix=p, advances=advances, us_per_advance=per_advance,
                                 us_per_frame=per_advance / n, session_over_prefix=s["median"] / p["median"],
                                 session_over_forward_auto=s["median"] / out["forward[auto]"]["median"],
                                 session_over_forward_f32=s["median"] / out["forward[f32]"]["median"])
  enc.recurrence = 'auto'
  return out


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--calls", type=int, default=10)
  ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_stream.json"))
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args(argv)
  import warnings
  import torch
  if not torch.cuda.is_available():
    print("bench_encoder_stream: no GPU (this tool never falls back)", file=sys.stderr)
    return 1
  from lipreading_amd import _build
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  _build.build_library()
  dev = torch.device("cuda:0")
  c2i = default_char2idx()
  doc = dict(shape=dict(T=T, I=I, C=len(c2i) + 1), unit="us", repeats=a.repeats, calls=a.calls,
             device=torch.cuda.get_device_name(0), models={})
  for rnn_type, H, layers in MODELS:
    torch.manual_seed(0)
    enc = VideoEncoder(I, H, rnn_type=rnn_type, num_layers=layers, bidirectional=False, enable_ctc=True,
                       vocab_size=len(c2i), char2idx=c2i, device=dev).to(dev).eval()
    name = "%s-%d x%d" % (rnn_type, H, layers)
    doc["models"][name] = {}
    for B in a.batches:
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (a shape without a one-launch kernel says so once)
        doc["models"][name]["B=%d" % B] = measure(torch, enc, B, a.repeats, a.calls)
      r = doc["models"][name]["B=%d" % B]
      print("%-12s B=%-2d forward f32 %8.0f auto %8.0f | " % (name, B, r["forward[f32]"]["median"],
                                                             r["forward[auto]"]["median"]) +
            "  ".join("[%s] %.0f (%.1f/frame) vs prefix %.0f = %.3f" % (
                n, c["session"]["median"], c["us_per_frame"], c["prefix"]["median"], c["session_over_prefix"])
                      for n, c in r["chunks"].items()), file=sys.stderr, flush=True)
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(a.out, "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
