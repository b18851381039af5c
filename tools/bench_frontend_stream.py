#!/usr/bin/env python
"""Measure conv frontend sessions (ConvFrontend3D.stream, lr_conv_stream_*) against ConvFrontend3D.forward
on the same clips in the same process.  bench.py stays as it is.

  python tools/bench_frontend_stream.py                   # one JSON document on stdout and profiles/frontend_stream.json
  python tools/bench_frontend_stream.py --no-save --repeats 3 --calls 2 --batches 1

uint8 clips (B, 75, 3, 96, 96), B in {1, 8, 32}.  Arms, us per call:
  session[N]     a session reset and fed the 75 frames in chunks of N = 75, 25, 5, 1 frames, the last chunk with `end`
  reset          the reset alone
  forward        (a) ConvFrontend3D.forward over the whole clip once
  prefix[N]      (b) the prefix re-run total: ConvFrontend3D.forward over the growing prefixes N, 2N, ... 75
  window[N]      (c) the window re-run total: per chunk, ConvFrontend3D.forward over the chunk and the 3 frames on either
                 side of it (N + 6 frames inside the clip): what yields the chunk's features without a session
From them: us per advance = (session - reset) / advances, us per frame = that / N, and session[N] over (a), (b), (c).
Protocol: warm-up calls of every arm, then `repeats` rounds with the arms alternated; an arm is `calls` calls back to
back between two device events.  Medians and min-max.  Every chunking's features and state bytes are compared, bit for
bit, with the one-chunk session's before anything is timed.  No GPU, no numbers: the tool exits non-zero without one.
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

T, H, W = 75, 96, 96
CHUNKS = (75, 25, 5, 1)
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


def measure(torch, fe, B, repeats, calls):
  dev = torch.device("cuda:0")
  clips = torch.randint(0, 256, (B, T, 3, H, W), generator=torch.Generator().manual_seed(B), dtype=torch.uint8).to(dev)
  st = fe.stream(B, H, W, dev)
  last = torch.ones((B,), dtype=torch.int32, device=dev)

  def session(n, keep=False):
    st.reset()
    out = []
    for t0 in range(0, T, n):
      f, c = st.feed(clips[:, t0:t0 + n], None, last if t0 + n >= T else None)
      if keep:
        k = c.cpu().tolist()
        assert len(set(k)) == 1
        out.append(f[:, :k[0]])
    return torch.cat(out, dim=1) if keep else None

  def forward(t0=0, t1=T):
    with torch.no_grad():
      return fe(clips[:, t0:t1])

  def prefix(n):
    for t in range(n, T + 1, n):
      forward(0, t)

  def window(n):
    for t0 in range(0, T, n):
      forward(max(0, t0 - 3), min(T, t0 + n + 3))

  # the same bits before anything is timed; the one-shot forward agrees on these unpadded clips
  want, want_state = session(T, keep=True), st.state_buf.clone()
  assert want.shape[1] == T
  for n in CHUNKS:
    assert torch.equal(session(n, keep=True), want) and torch.equal(st.state_buf, want_state), "chunks of %d differ" % n
  one = forward()
  scale = float(one.abs().max())
  err = float((one - want).abs().max()) / max(scale, 1e-6)
  assert err < 2e-2, err
  arms = {"reset": st.reset, "forward": forward}
  arms.update({"session[%d]" % n: (lambda n=n: session(n)) for n in CHUNKS})
  arms.update({"prefix[%d]" % n: (lambda n=n: prefix(n)) for n in CHUNKS})
  arms.update({"window[%d]" % n: (lambda n=n: window(n)) for n in CHUNKS})
  for fn in arms.values():
    for _ in range(2):
      fn()
  seen = {k: [] for k in arms}
  for _ in range(repeats):
    for k, fn in arms.items():
      seen[k].append(_timed(torch, calls, fn))
  out = {k: _summary(seen[k]) for k in ("reset", "forward")}
  out["max_rel_diff_to_forward"] = err
  out["chunks"] = {}
  for n in CHUNKS:
    s, p, w = (_summary(seen["%s[%d]" % (k, n)]) for k in ("session", "prefix", "window"))
    advances = -(-T // n)
    per_advance = (s["median"] - out["reset"]["median"]) / advances
    out["chunks"][str(n)] = dict(session=s, prefix=p, window=w, advances=advances, us_per_advance=per_advance,
                                 us_per_frame=per_advance / n, session_over_forward=s["median"] / out["forward"]["median"],
                                 session_over_prefix=s["median"] / p["median"],
                                 session_over_window=s["median"] / w["median"], mac_share_of_window=1.0 / (1.0 + 6.0 / n))
  return out


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--calls", type=int, default=3)
  ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_stream.json"))
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args(argv)
  import torch
  if not torch.cuda.is_available():
    print("bench_frontend_stream: no GPU (this tool never falls back)", file=sys.stderr)
    return 1
  from lipreading_amd import _build
  from lipreading_amd.frontend import ConvFrontend3D
  _build.build_library()
  dev = torch.device("cuda:0")
  torch.manual_seed(0)
  fe = ConvFrontend3D().to(dev).eval()
  doc = dict(shape=dict(T=T, H=H, W=W), unit="us", repeats=a.repeats, calls=a.calls,
             device=torch.cuda.get_device_name(0), batches={})
  for B in a.batches:
    r = doc["batches"]["B=%d" % B] = measure(torch, fe, B, a.repeats, a.calls)
    print("B=%-2d forward %8.0f | " % (B, r["forward"]["median"]) +
          "  ".join("[%s] %.0f (%.1f/frame) vs prefix %.0f = %.3f, window %.0f = %.3f" % (
              n, c["session"]["median"], c["us_per_frame"], c["prefix"]["median"], c["session_over_prefix"],
              c["window"]["median"], c["session_over_window"]) for n, c in r["chunks"].items()),
          file=sys.stderr, flush=True)
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(a.out, "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
