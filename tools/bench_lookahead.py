#!/usr/bin/env python
"""Measure look-ahead sessions of a bidirectional encoder (VideoEncoder.stream_lookahead, lr_rnn_bistream_*, DESIGN.md
§29) against what a live caller pays without them: VideoEncoder.forward over the growing prefix at every chunk.  Same
utterances, same process.  bench.py stays as it is.

  python tools/bench_lookahead.py                   # one JSON document on stdout and profiles/encoder_lookahead.json
  python tools/bench_lookahead.py --no-save --repeats 3 --calls 3 --batches 1

BiGRU-256 x1 / x2 and BiLSTM-768 x1 at I = 204, C = 65, B in {1, 32}, T = 75, head included.  Arms, us per utterance
batch, for (chunk N, look-ahead R) in (75, 0), (25, 10), (5, 0), (5, 5), (5, 10), (1, 5):
  session[N,R]   a session reset and fed the 75 frames N at a time, each advance over a window of N + R frames (cut at
                 the utterance's end): ceil(75 / N) advances of layers x window step launches, a head and a commit
  prefix[N,R]    VideoEncoder.forward (recurrence 'auto', the library's offline path) over the growing prefixes
                 min(N + R, 75), min(2 N + R, 75), ... 75: the same frames seen at the same moments
  reset          the reset alone
  forward        VideoEncoder.forward over the whole utterance once
From them: us per advance = (session - reset) / advances, us per frame = that / N, and session / prefix.
Protocol: warm-up calls, then `repeats` rounds with the arms alternated; an arm is `calls` calls back to back between
two device events.  Medians and min-max.  Before anything is timed: full look-ahead in chunks of 5 and 1 gives the single
advance's log-probabilities and state bit for bit, every arm gives the same bits twice, and the single advance agrees
with VideoEncoder.forward (recurrence 'f32') to 1e-3.  At most 16 CPU threads.  No GPU, no numbers: the tool exits
non-zero without one.
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
CUTS = ((75, 0), (25, 10), (5, 0), (5, 5), (5, 10), (1, 5))
MODELS = (("GRU", 256, 1), ("GRU", 256, 2), ("LSTM", 768, 1))
BATCHES = (1, 32)


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
  ahead = {r: torch.full((B,), r, dtype=torch.int32, device=dev) for r in range(0, T + 1)}
  st = enc.stream_lookahead(B, dev)

  def session(n, r):
    st.reset()
    out = []
    for t0 in range(0, T, n):
      c = min(n, T - t0)
      t1 = min(T, t0 + c + r)
      out.append(st.feed(frames[:, t0:t1], None, ahead[t1 - t0 - c], chunk=c))
    return torch.cat(out, dim=1)

  def forward(recurrence, t=T):
    enc.recurrence = recurrence
    with torch.no_grad():
      return enc(frames[:, :t], lens[t], max_len=t, need_final_state=False)[0]

  def prefix(n, r):
    for t0 in range(0, T, n):
      forward('auto', min(T, t0 + n + r))

  want, want_state = session(T, 0), st.state_buf.clone()
  for n in (5, 1):
    assert torch.equal(session(n, T), want) and torch.equal(st.state_buf, want_state), "full look-ahead, chunks of %d" % n
  for n, r in CUTS:
    a, sa = session(n, r), st.state_buf.clone()
    assert torch.equal(session(n, r), a) and torch.equal(st.state_buf, sa), "(%d, %d) twice" % (n, r)
  err = float((forward('f32') - want).abs().max())
  assert err < 1e-3, err
  arms = {"reset": st.reset, "forward": lambda: forward('auto')}
  arms.update({"session[%d,%d]" % c: (lambda c=c: session(*c)) for c in CUTS})
  arms.update({"prefix[%d,%d]" % c: (lambda c=c: prefix(*c)) for c in CUTS})
  for fn in arms.values():
    for _ in range(2):
      fn()
  seen = {k: [] for k in arms}
  for _ in range(repeats):
    for k, fn in arms.items():
      seen[k].append(_timed(torch, calls, fn))
  out = {k: _summary(seen[k]) for k in ("reset", "forward")}
  out["max_abs_diff_to_forward_f32"] = err
  out["cuts"] = {}
  for n, r in CUTS:
    s, p = _summary(seen["session[%d,%d]" % (n, r)]), _summary(seen["prefix[%d,%d]" % (n, r)])
    advances = -(-T // n)
    per_advance = (s["median"] - out["reset"]["median"]) / advances
    out["cuts"]["%d,%d" % (n, r)] = dict(session=s, prefix=p, advances=advances, chunk=n, lookahead=r,
                                         us_per_advance=per_advance, us_per_frame=per_advance / n,
                                         session_over_prefix=s["median"] / p["median"],
                                         session_over_forward=s["median"] / out["forward"]["median"])
  enc.recurrence = 'auto'
  return out


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--calls", type=int, default=5)
  ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_lookahead.json"))
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args(argv)
  import warnings
  import torch
  torch.set_num_threads(min(16, torch.get_num_threads()))
  if not torch.cuda.is_available():
    print("bench_lookahead: no GPU (this tool never falls back)", file=sys.stderr)
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
    enc = VideoEncoder(I, H, rnn_type=rnn_type, num_layers=layers, bidirectional=True, enable_ctc=True,
                       vocab_size=len(c2i), char2idx=c2i, device=dev).to(dev).eval()
    name = "Bi%s-%d x%d" % (rnn_type, H, layers)
    doc["models"][name] = {}
    for B in a.batches:
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (a shape without a one-launch kernel says so once)
        doc["models"][name]["B=%d" % B] = measure(torch, enc, B, a.repeats, a.calls)
      r = doc["models"][name]["B=%d" % B]
      print("%-14s B=%-2d forward %8.0f | " % (name, B, r["forward"]["median"]) +
            "  ".join("[%s] %.0f (%.1f/frame) vs prefix %.0f = %.3f" % (
                k, c["session"]["median"], c["us_per_frame"], c["prefix"]["median"], c["session_over_prefix"])
                      for k, c in r["cuts"].items()), file=sys.stderr, flush=True)
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(a.out, "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
