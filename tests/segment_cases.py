"""Shared by tests/test_segment_cpu.py and tests/test_gpu_segment.py: the restatement of lr_ctc_segment (DESIGN.md §24,
include/lipreading_hip.h A6g) and the case generators both files grade on.

`viterbi` is the header's recursion, tie-break included, in NumPy float32: states s = 0..2L (even = blank, odd s =
y[(s-1)/2]); every v is -inf before frame 0; per frame `best` over stay (code 0), step (1), skip (2) and the fresh start
0.0f (3; s <= 1 and (t == 0 or FREE_START)) in this order, a later candidate winning only if strictly greater; v = best
+ lp[t][cls(s)].  One add per cell, so a float32 run is what an IEEE-faithful kernel computes bit for bit.  The end, the
walk back, spans and utterance sums are plain Python.
"""
import itertools

import numpy as np

from tests import align_cases as ac

FREE_START, FREE_END = 1, 2
INFEASIBLE, BAD_ID, BAD_LENGTH, BAD_UTTERANCE = 1, -1, -2, -3
f32 = np.float32
FAMILIES = ac.FAMILIES


def viterbi(lp, target, blank, flags):
  """lp (n, C) float32, target a list of L class ids -> (total, path, first): total a float32 scalar (-inf: no path, then
  path is None), path the states of frames first..first+len(path)-1."""
  lp = np.asarray(lp, dtype=f32)
  n, L = lp.shape[0], len(target)
  S = 2 * L + 1
  cls = np.full(S, blank, dtype=np.int64)
  cls[1::2] = target
  skip = np.zeros(S, dtype=bool)
  for s in range(3, S, 2):
    skip[s] = cls[s] != cls[s - 2]
  fresh = np.zeros(S, dtype=bool)
  fresh[:2] = True
  neg, zero = f32(-np.inf), f32(0)
  v = np.full(S, neg, dtype=f32)
  codes = np.zeros((n, S), dtype=np.uint8)
  pad = np.full(S + 2, neg, dtype=f32)
  ev, et, es = neg, -1, -1
  for t in range(n):
    pad[2:] = v
    c1 = pad[1:1 + S]
    c2 = np.where(skip, pad[0:S], neg)
    best = v.copy()
    code = np.zeros(S, dtype=np.uint8)
    m = c1 > best
    best[m] = c1[m]
    code[m] = 1
    m = c2 > best
    best[m] = c2[m]
    code[m] = 2
    if t == 0 or flags & FREE_START:
      m = fresh & (zero > best)
      best[m] = zero
      code[m] = 3
    v = best + lp[t, cls]
    assert v.dtype == f32
    codes[t] = code
    if flags & FREE_END or t == n - 1:
      if L > 0 and v[2 * L - 1] > ev:
        ev, et, es = v[2 * L - 1], t, 2 * L - 1
      if v[2 * L] > ev:
        ev, et, es = v[2 * L], t, 2 * L
  if ev == neg:
    return ev, None, -1
  path = []
  s, t = es, et
  while True:
    path.append(s)
    c = int(codes[t, s])
    if c == 3 or t == 0:
      break
    s -= c
    t -= 1
  return ev, path[::-1], t


def segment_one(lp, target, blank, flags, utts=()):
  """One sample's outputs as plain Python: dict(status, total, span, frame_token [n], tok [(start, end, logp)],
  utts [(start, end, frames, logp, worst)])."""
  lp = np.asarray(lp, dtype=f32)
  n = lp.shape[0]
  total, path, first = viterbi(lp, target, blank, flags)
  if path is None:
    return dict(status=INFEASIBLE, total=total)
  ft = [-1] * n
  for k, s in enumerate(path):
    if s & 1:
      ft[first + k] = (s - 1) // 2
  runs = [[] for _ in target]
  for t in range(first, first + len(path)):
    if ft[t] >= 0:
      runs[ft[t]].append(t)
  tok = []
  for frames, c in zip(runs, target):
    assert frames and frames == list(range(frames[0], frames[-1] + 1))
    sm = f32(0)
    for t in frames:
      sm = f32(sm + lp[t, c])
    tok.append((frames[0], frames[-1] + 1, sm))
  out = []
  for f, c in utts:
    if c == 0:
      out.append((-1, -1, 0, f32(0), -1))
      continue
    sm, fr, worst = f32(0), 0, f
    for i in range(f, f + c):
      sm = f32(sm + tok[i][2])
      fr += tok[i][1] - tok[i][0]
      if tok[i][2] < tok[worst][2]:
        worst = i
    out.append((tok[f][0], tok[f + c - 1][1], fr, sm, worst))
  return dict(status=0, total=total, span=(first, first + len(path)), frame_token=ft, tok=tok, utts=out)


UTT_KEYS = ("utt_start", "utt_end", "utt_frames", "utt_logp", "utt_worst")


def expected(lp, sizes, targets, target_lens, blank, flags, utt_first=None, utt_count=None, n_utts=None):
  """The whole batch as the kernels write it: lp (B, T, C) float32, sizes (B,) or None, targets (B, W) ints,
  target_lens (B,), utterance ranges (B, US) and n_utts (B,) or None -> dict of arrays named as lr_ctc_segment's
  outputs (-1 / 0 padding, statuses included).  Frames t >= n and ids past the lengths are not touched."""
  B, T, C = lp.shape
  W = targets.shape[1]
  out = dict(frame_token=np.full((B, T), -1, np.int32), tok_start=np.full((B, W), -1, np.int32),
             tok_end=np.full((B, W), -1, np.int32), tok_logp=np.zeros((B, W), f32), span=np.full((B, 2), -1, np.int32),
             total=np.full(B, -np.inf, f32), status=np.zeros(B, np.int32))
  US = 0
  if n_utts is not None:
    US = utt_first.shape[1]
    out.update(utt_start=np.full((B, US), -1, np.int32), utt_end=np.full((B, US), -1, np.int32),
               utt_frames=np.zeros((B, US), np.int32), utt_logp=np.zeros((B, US), f32),
               utt_worst=np.full((B, US), -1, np.int32))
  for b in range(B):
    n = T if sizes is None else int(sizes[b])
    L = int(target_lens[b])
    U = 0 if n_utts is None else int(n_utts[b])
    if n < 1 or n > T or L < 0 or L > W or U < 0 or U > US:
      out["status"][b] = BAD_LENGTH
      continue
    y = [int(c) for c in targets[b, :L]]
    if any(c < 0 or c >= C or c == blank for c in y):
      out["status"][b] = BAD_ID
      continue
    utts = [(int(utt_first[b, u]), int(utt_count[b, u])) for u in range(U)]
    if any(f < 0 or c < 0 or f + c > L for f, c in utts):
      out["status"][b] = BAD_UTTERANCE
      continue
    r = segment_one(np.asarray(lp[b, :n], dtype=f32), y, blank, flags, utts)
    out["status"][b] = r["status"]
    if r["status"] != 0:
      continue
    out["total"][b] = r["total"]
    out["span"][b] = r["span"]
    out["frame_token"][b, :n] = r["frame_token"]
    for i, (s, e, p) in enumerate(r["tok"]):
      out["tok_start"][b, i], out["tok_end"][b, i], out["tok_logp"][b, i] = s, e, p
    for u, vals in enumerate(r["utts"]):
      for k, x in zip(UTT_KEYS, vals):
        out[k][b, u] = x
  return out


def best_by_enumeration(lp, target, blank, flags):
  """The best score over every sub-span [t0, t1) of the n frames that the flags allow (t0 = 0 without FREE_START,
  t1 = n without FREE_END) and every class sequence on it that collapses to `target`; None if there is none.  float64,
  for tiny integer-valued shapes where every sum is exact."""
  lp = np.asarray(lp, dtype=np.float64)
  n, C = lp.shape
  best = None
  for t0 in (range(n) if flags & FREE_START else (0,)):
    for t1 in (range(t0 + 1, n + 1) if flags & FREE_END else (n,)):
      for seq in itertools.product(range(C), repeat=t1 - t0):
        if ac.collapse(seq, blank) == list(target):
          sc = sum(lp[t0 + k, c] for k, c in enumerate(seq))
          if best is None or sc > best:
            best = sc
  return best


# ---- cases -------------------------------------------------------------------------------------------------------------
def make_utts(rng, L, US):
  """Ranges over a target of L tokens as the GPU test wants them: an empty one, a one-token one, unowned tokens between
  ranges, and ranges out of order.  -> (first [US], count [US], n) with n <= US used."""
  if L < 16:
    ranges = [(0, 0)] + ([(0, 1)] if L >= 1 else []) + ([(L - 1, 1)] if L >= 2 else [])
  else:
    q = L // 4
    ranges = [(2 * q + 1, q), (0, 0), (1, 1), (3, q - 2), (q + 2, q - 3), (L - 1, 1), (3 * q + 2, L - 3 * q - 3)]
  ranges = ranges[:US]
  first = np.zeros(US, np.int32)
  count = np.zeros(US, np.int32)
  for u, (f, c) in enumerate(ranges):
    assert 0 <= f and 0 <= c and f + c <= L
    first[u], count[u] = f, c
  return first, count, len(ranges)


def batch(rng, family, B, T, C, W, sizes, lens, blank, US=8):
  """lp (B, T, C) of the family, doubled targets of the given lengths and make_utts ranges."""
  lp = family(rng, (B, T, C))
  targets = np.zeros((B, W), np.int32)
  uf, uc, nu = np.zeros((B, US), np.int32), np.zeros((B, US), np.int32), np.zeros(B, np.int32)
  for b in range(B):
    targets[b, :lens[b]] = ac.random_target(rng, lens[b], C, blank, doubled=True)
    uf[b], uc[b], nu[b] = make_utts(rng, lens[b], US)
  return lp, targets, np.asarray(sizes, np.int32), np.asarray(lens, np.int32), uf, uc, nu


def planted_stream(seed, C=12, blank=0, margin=8.0, utt_tokens=(20, 35, 15), gap=10):
  """A stream with a known answer: junk frames at the head and tail that avoid the first and last token, then per
  utterance its tokens in runs of 1 to 3 frames with 0 or 1 blank after each, and `gap` blank frames between utterances.
  The planted class of a frame has logit `margin`, the others 0.  -> (lp (n, C) float32, target, utts [(first, count)],
  planted [(start, end)] per utterance)."""
  rng = np.random.RandomState(seed)
  target, utts = [], []
  for c in utt_tokens:
    utts.append((len(target), c))
    target += ac.random_target(rng, c, C, blank)
  junk = [c for c in range(C) if c not in (blank, target[0], target[-1])]
  frames, planted = [], []
  frames += [junk[k] for k in rng.randint(0, len(junk), size=rng.randint(5, 15))]
  for u, (f, c) in enumerate(utts):
    start = len(frames)
    for i in range(f, f + c):
      if frames and frames[-1] == target[i]:
        frames.append(blank)   # (a repeated class needs its blank)
      frames += [target[i]] * rng.randint(1, 4)
      end = len(frames)
      if rng.randint(0, 2):
        frames.append(blank)
    planted.append((start, end))
    if u + 1 < len(utts):
      frames += [blank] * gap
  if frames[-1] != blank:
    frames.append(blank)
  frames += [junk[k] for k in rng.randint(0, len(junk), size=rng.randint(5, 15))]
  logits = np.zeros((len(frames), C), np.float64)
  logits[np.arange(len(frames)), frames] = margin
  lp = logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))
  return lp.astype(f32), target, utts, planted
