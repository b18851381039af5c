#!/usr/bin/env python
"""Measure resumable beam search sessions (BeamCTCDecoder.stream, lr_ctc_beam_stream_*) against the
one-shot lr_ctc_beam_decode on the same input in the same process.  bench.py stays as it is.

  python tools/bench_beam_stream.py                       # one JSON document on stdout and profiles/beam_stream.json
  python tools/bench_beam_stream.py --lm model.arpa --hotwords 20    # one more line: language model + hotwords
  python tools/bench_beam_stream.py --no-save --repeats 3 --calls 5

B = 32, T = 75, C = 65, beam width 100, cutoff_top_n 40 (tools/bench_beam.py's input).  Arms, us per call:
  one_shot            BeamCTCDecoder.decode_ids on the whole block: the comparison
  utterance[N]        a session reset and fed the 75 frames in chunks of N = 1, 5, 25, 75 frames (75 / N advances)
  reset, read         the reset alone and one read (all 100 hypotheses, width 75) alone
From them: us per advance = (utterance - reset) / advances, us per frame = that / N, and the whole utterance's total =
utterance + one read, against the one-shot call.
Protocol: warm-up calls, then `repeats` rounds with the arms alternated; an arm is `calls` calls back to back between
two device events.  Medians and min-max.  The session's answer is compared with the one-shot call's before anything
is timed.  No GPU, no numbers: the tool exits non-zero without one.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
  if p not in sys.path:
    sys.path.insert(0, p)

B, T, C, W, N_TOP = 32, 75, 65, 100, 40
CHUNKS = (1, 5, 25, 75)


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


def measure(torch, dec, pd, repeats, calls, chunks=CHUNKS):
  """The arms of one decoder: {"one_shot", "reset", "read", "chunks": {N: {...}}}, us."""
  st = dec.stream(B, T, pd.device)

  def utterance(n):
    st.reset()
    for t0 in range(0, T, n):
      st.feed(pd[:, t0:t0 + n])

  # the same bits before anything is timed
  want = dec.decode_ids(pd)
  for n in chunks:
    utterance(n)
    got = st.read_ids(W, T)
    for g, w in zip(got[:4], want):
      assert torch.equal(g.view(torch.int32), w.view(torch.int32)), "the session differs from the one-shot search"
  arms = {"one_shot": lambda: dec.decode_ids(pd), "reset": st.reset, "read": lambda: st.read_ids(W, T)}
  arms.update({"utterance[%d]" % n: (lambda n=n: utterance(n)) for n in chunks})
  for fn in arms.values():
    for _ in range(3):
      fn()
  seen = {k: [] for k in arms}
  for _ in range(repeats):
    for k, fn in arms.items():
      seen[k].append(_timed(torch, calls, fn))
  out = {k: _summary(seen[k]) for k in ("one_shot", "reset", "read")}
  out["chunks"] = {}
  one = out["one_shot"]["median"]
  for n in chunks:
    u = _summary(seen["utterance[%d]" % n])
    advances = -(-T // n)
    per_advance = (u["median"] - out["reset"]["median"]) / advances
    total = u["median"] + out["read"]["median"]
    out["chunks"][str(n)] = dict(utterance=u, advances=advances, us_per_advance=per_advance,
                                 us_per_frame=per_advance / n, total_with_one_read=total,
                                 total_over_one_shot=total / one)
  return out


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=7)
  ap.add_argument("--calls", type=int, default=10)
  ap.add_argument("--lm", default=None, help="an ARPA file: one more line with the language model and the hotwords")
  ap.add_argument("--alpha", type=float, default=0.5)
  ap.add_argument("--beta", type=float, default=1.0)
  ap.add_argument("--hotwords", type=int, default=20, help="with --lm: N random hotwords (tools/bench_beam.py's)")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_stream.json"))
  ap.add_argument("--no-save", action="store_true")
  a = ap.parse_args(argv)
  import numpy as np
  import torch
  if not torch.cuda.is_available():
    print("bench_beam_stream: no GPU (this tool never falls back)", file=sys.stderr)
    return 1
  import bench_beam
  from lipreading_amd import _build
  from lipreading_amd.decoder import BeamCTCDecoder
  _build.build_library()
  dev = torch.device("cuda:0")
  pd = torch.tensor(bench_beam.peaked(np.random.default_rng(0)), device=dev)
  labels = ["_"] + [chr(ord("!") + i) for i in range(C - 1)]
  doc = dict(shape=dict(B=B, T=T, C=C, beam_width=W, cutoff_top_n=N_TOP), unit="us", repeats=a.repeats, calls=a.calls,
             device=torch.cuda.get_device_name(0),
             plain=measure(torch, BeamCTCDecoder(labels, beam_width=W, cutoff_top_n=N_TOP), pd, a.repeats, a.calls))
  if a.lm:
    from lipreading_amd.data import default_char2idx
    from lipreading_amd.decoder import ctc_labels
    lm_labels = ctc_labels(default_char2idx())
    assert len(lm_labels) == C
    with warnings.catch_warnings():
      warnings.simplefilter("ignore")   # random strings are no words of the model: only the lookups are timed
      dec = BeamCTCDecoder(lm_labels, lm_path=a.lm, alpha=a.alpha, beta=a.beta, beam_width=W, cutoff_top_n=N_TOP,
                           hotwords=bench_beam.random_hotwords(lm_labels, a.hotwords))
    doc["lm_bias"] = dict(lm=os.path.basename(a.lm), lm_order=dec.lm.order, lm_ngrams=int(sum(dec.lm.counts)),
                          hotwords=a.hotwords, **measure(torch, dec, pd, a.repeats, a.calls, chunks=(5, 75)))
  text = json.dumps(doc, indent=1, sort_keys=True)
  print(text)
  if not a.no_save:
    with open(a.out, "w") as f:
      f.write(text + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
