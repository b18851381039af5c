"""Shared by tests/test_align_cpu.py and tests/test_gpu_align.py: the restatement of lr_ctc_align and
the case generators both files grade on.

`viterbi` is the recursion of include/lipreading_hip.h, tie-break included, in NumPy at a chosen precision: states
s = 0..2L (even = blank, odd s = y[(s-1)/2]); v[0][0] = lp[0][blank], v[0][1] = lp[0][y[0]], -inf elsewhere; for t >= 1
v[t][s] = best + lp[t][cls(s)] with best over v[t-1][s] (code 0), v[t-1][s-1] (code 1), v[t-1][s-2] (code 2; s odd,
s >= 3, cls(s) != cls(s-2)) in this order, a later candidate winning only if strictly greater.  One add per cell, so a
float32 run is what an IEEE-faithful kernel computes bit for bit.  Spans, sums and word grouping are plain Python.
"""
import itertools

import numpy as np

INFEASIBLE, BAD_ID, BAD_LENGTH = 1, -1, -2
f32 = np.float32


def viterbi(lp, target, blank, dtype=np.float32):
  """lp (n, C), target a list of L class ids -> (total, path): total a `dtype` scalar (-inf: no alignment, path None),
  path the list of n states."""
  lp = np.asarray(lp, dtype=dtype)
  n, L = lp.shape[0], len(target)
  S = 2 * L + 1
  cls = np.full(S, blank, dtype=np.int64)
  cls[1::2] = target
  skip = np.zeros(S, dtype=bool)
  for s in range(3, S, 2):
    skip[s] = cls[s] != cls[s - 2]
  neg = dtype(-np.inf)
  v = np.full(S, neg, dtype=dtype)
  v[0] = lp[0, blank]
  if L >= 1:
    v[1] = lp[0, target[0]]
  codes = np.zeros((n, S), dtype=np.uint8)
  pad = np.full(S + 2, neg, dtype=dtype)
  for t in range(1, n):
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
    v = best + lp[t, cls]
    assert v.dtype == dtype
    codes[t] = code
  end = 0 if L == 0 else (2 * L if v[2 * L] > v[2 * L - 1] else 2 * L - 1)
  total = v[end]
  if total == neg:
    return total, None
  path = [0] * n
  s = end
  for t in range(n - 1, -1, -1):
    path[t] = s
    s -= int(codes[t, s])
  return total, path


def words_of(target, roles):
  """[(first, count)]: the maximal runs of consecutive role-1 tokens."""
  out = []
  for i, c in enumerate(target):
    if roles[c] != 1:
      continue
    if i == 0 or roles[target[i - 1]] != 1:
      out.append([i, 0])
    out[-1][1] += 1
  return [tuple(w) for w in out]


def align_one(lp, target, blank, roles=None, dtype=np.float32):
  """One sample's outputs as plain Python: dict(status, total, frame_token [n], tok [(start, end, logp)],
  words [(first, count, start, end, logp)])."""
  lp = np.asarray(lp, dtype=dtype)
  total, path = viterbi(lp, target, blank, dtype)
  if path is None:
    return dict(status=INFEASIBLE, total=total, frame_token=None, tok=[], words=[])
  n = len(path)
  ft = [(s - 1) // 2 if s & 1 else -1 for s in path]
  tok = []
  for i, c in enumerate(target):
    frames = [t for t in range(n) if ft[t] == i]
    assert frames and frames == list(range(frames[0], frames[-1] + 1))
    sm = dtype(0)
    for t in frames:
      sm = dtype(sm + lp[t, c])
    tok.append((frames[0], frames[-1] + 1, sm))
  words = []
  if roles is not None:
    for f, c in words_of(target, roles):
      sm = dtype(0)
      for i in range(f, f + c):
        sm = dtype(sm + tok[i][2])
      words.append((f, c, tok[f][0], tok[f + c - 1][1], sm))
  return dict(status=0, total=total, frame_token=ft, tok=tok, words=words)


def expected(lp, sizes, targets, target_lens, blank, roles=None):
  """The whole batch as the kernel writes it: lp (B, T, C) float32, sizes (B,) or None, targets (B, W) ints,
  target_lens (B,) -> dict of arrays named as lr_ctc_align's outputs (-1 / 0 padding, statuses included)."""
  lp = np.asarray(lp, dtype=np.float32)
  B, T, C = lp.shape
  W = targets.shape[1]
  out = dict(frame_token=np.full((B, T), -1, np.int32), tok_start=np.full((B, W), -1, np.int32),
             tok_end=np.full((B, W), -1, np.int32), tok_logp=np.zeros((B, W), np.float32),
             total=np.full(B, -np.inf, np.float32), status=np.zeros(B, np.int32))
  if roles is not None:
    out.update(word_first=np.full((B, W), -1, np.int32), word_count=np.full((B, W), -1, np.int32),
               word_start=np.full((B, W), -1, np.int32), word_end=np.full((B, W), -1, np.int32),
               word_logp=np.zeros((B, W), np.float32), n_words=np.zeros(B, np.int32))
  for b in range(B):
    n = T if sizes is None else int(sizes[b])
    L = int(target_lens[b])
    if n < 1 or n > T or L < 0 or L > W:
      out["status"][b] = BAD_LENGTH
      continue
    y = [int(c) for c in targets[b, :L]]
    if any(c < 0 or c >= C or c == blank for c in y):
      out["status"][b] = BAD_ID
      continue
    r = align_one(lp[b, :n], y, blank, roles)
    out["status"][b] = r["status"]
    if r["status"] != 0:
      continue
    out["total"][b] = r["total"]
    out["frame_token"][b, :n] = r["frame_token"]
    for i, (s, e, p) in enumerate(r["tok"]):
      out["tok_start"][b, i], out["tok_end"][b, i], out["tok_logp"][b, i] = s, e, p
    if roles is not None:
      out["n_words"][b] = len(r["words"])
      for w, (f, c, s, e, p) in enumerate(r["words"]):
        out["word_first"][b, w], out["word_count"][b, w] = f, c
        out["word_start"][b, w], out["word_end"][b, w], out["word_logp"][b, w] = s, e, p
  return out


def collapse(classes, blank):
  """Merge repeats, drop blanks."""
  out, prev = [], None
  for c in classes:
    if c != prev and c != blank:
      out.append(c)
    prev = c
  return out


def best_by_enumeration(lp, target, blank):
  """The best score over ALL class sequences of n frames that collapse to `target` (None if there is none), in
  float64 — for tiny shapes with integer values, where every sum is exact."""
  lp = np.asarray(lp, dtype=np.float64)
  n, C = lp.shape
  best = None
  for seq in itertools.product(range(C), repeat=n):
    if collapse(seq, blank) == list(target):
      sc = sum(lp[t, c] for t, c in enumerate(seq))
      if best is None or sc > best:
        best = sc
  return best


def repeats(target):
  return sum(1 for i in range(1, len(target)) if target[i] == target[i - 1])


# ---- value families and targets -----------------------------------------------------------------------------------
def quantised(rng, shape):
  """Multiples of 1/64 in (-16, 0]: every partial sum of up to 2048 of them is exact in float32 (21 bits)."""
  return (-rng.randint(0, 1024, size=shape) / 64.0).astype(np.float32)


def integers(rng, shape):
  """Integers in {-1, -2, -3}: ties everywhere."""
  return (-rng.randint(1, 4, size=shape)).astype(np.float32)


def log_softmax(rng, shape):
  x = rng.randn(*shape).astype(np.float32) * f32(3)
  x = x - x.max(axis=-1, keepdims=True)
  return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


FAMILIES = (("quantised", quantised), ("integers", integers), ("log_softmax", log_softmax))


def random_target(rng, L, C, blank, doubled=False):
  """L ids from [0, C) without the blank; doubled=True plants equal neighbours at the front, middle and end."""
  ids = [c for c in range(C) if c != blank]
  y = [ids[k] for k in rng.randint(0, len(ids), size=L)]
  if doubled and L >= 2:
    y[1] = y[0]
    y[L // 2] = y[L // 2 - 1] if L // 2 >= 1 else y[L // 2]
    y[L - 1] = y[L - 2]
  return y
