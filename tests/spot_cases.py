"""Shared by tests/test_spot_cpu.py, tests/test_gpu_spot.py and tools/bench_spot.py: the restatement of lr_ctc_spot
 and a brute-force enumerator for tiny shapes.

`ratios` is d[t][c] = lp[t][c] - max_c lp[t][c], one float32 subtraction.  `trace` is the recursion of
include/lipreading_hip.h in NumPy float32: states j = 0..2L-2 (even = y[j/2], odd = the blank between two tokens), every
state a pair (v, st); candidates stay, step, skip (j even, j >= 2, y[j/2] != y[j/2-1]) and, for j = 0, the fresh start
(0, t), in this order, a later one winning only if strictly greater; v = best.v + d[t][cls(j)], st = best.st or -1 when
v is -inf.  One add per cell, so a float32 run is what an IEEE-faithful kernel computes bit for bit.  `trace_batch` is
`trace` for many keywords at once (the same operations over a (K, states) array; tests/test_spot_cpu.py holds it to
`trace`), `hits` the greedy non-overlapping selection.  The value families and random_target are
tests/align_cases.py's.
"""
import itertools

import numpy as np

from tests.align_cases import FAMILIES, collapse, integers, log_softmax, quantised, random_target, repeats  # noqa: F401

BAD_ID, BAD_LENGTH = -1, -2
MAX_KW_LEN, MAX_T, MAX_HITS = 32, 2048, 16
f32 = np.float32
NEG = f32(-np.inf)


def ratios(lp):
  """lp (..., C) float32 -> lp - max over the classes (the blank included), float32."""
  lp = np.asarray(lp, dtype=np.float32)
  with np.errstate(invalid="ignore"):
    d = lp - lp.max(axis=-1, keepdims=True)
  assert d.dtype == np.float32
  return d


def trace(d, y, blank):
  """d (n, C) float32 ratios, y a list of L >= 1 class ids -> (end_score (n,) float32, end_start (n,) int32)."""
  d = np.asarray(d, dtype=np.float32)
  n, L = d.shape[0], len(y)
  S = 2 * L - 1
  cls = np.full(S, blank, dtype=np.int64)
  cls[0::2] = y
  skip = np.zeros(S, dtype=bool)
  for j in range(2, S, 2):
    skip[j] = y[j // 2] != y[j // 2 - 1]
  v = np.full(S, NEG, dtype=np.float32)
  st = np.full(S, -1, dtype=np.int32)
  end_score = np.full(n, NEG, dtype=np.float32)
  end_start = np.full(n, -1, dtype=np.int32)
  pv = np.full(S + 2, NEG, dtype=np.float32)
  ps = np.full(S + 2, -1, dtype=np.int32)
  for t in range(n):
    pv[2:], ps[2:] = v, st
    best, bs = v.copy(), st.copy()
    c1, s1 = pv[1:1 + S], ps[1:1 + S]
    m = c1 > best
    best[m], bs[m] = c1[m], s1[m]
    c2, s2 = np.where(skip, pv[0:S], NEG), ps[0:S]
    m = c2 > best
    best[m], bs[m] = c2[m], s2[m]
    if f32(0) > best[0]:
      best[0], bs[0] = f32(0), t
    v = best + d[t, cls]
    assert v.dtype == np.float32
    st = np.where(v == NEG, np.int32(-1), bs).astype(np.int32)
    end_score[t], end_start[t] = v[S - 1], st[S - 1]
  return end_score, end_start


def trace_batch(d, keywords, kw_lens, blank):
  """`trace` for K keywords at once (the same float32 operations, element by element, over a (K, states) array):
  keywords (K, W) ints with valid ids inside kw_lens (K,) -> (end_score (K, n) float32, end_start (K, n) int32)."""
  d = np.asarray(d, dtype=np.float32)
  n = d.shape[0]
  lens = np.asarray(kw_lens, dtype=np.int64)
  K, S = len(lens), 2 * int(lens.max()) - 1
  cls = np.full((K, S), blank, dtype=np.int64)
  skip = np.zeros((K, S), dtype=bool)
  for k in range(K):
    y = np.asarray(keywords[k][:lens[k]], dtype=np.int64)
    cls[k, 0:2 * lens[k] - 1:2] = y
    skip[k, 2:2 * lens[k] - 1:2] = y[1:] != y[:-1]
  last = 2 * lens - 2
  rows = np.arange(K)
  v = np.full((K, S), NEG, dtype=np.float32)
  st = np.full((K, S), -1, dtype=np.int32)
  end_score = np.full((K, n), NEG, dtype=np.float32)
  end_start = np.full((K, n), -1, dtype=np.int32)
  pv = np.full((K, S + 2), NEG, dtype=np.float32)
  ps = np.full((K, S + 2), -1, dtype=np.int32)
  for t in range(n):
    pv[:, 2:], ps[:, 2:] = v, st
    best, bs = v.copy(), st.copy()
    c1, s1 = pv[:, 1:1 + S], ps[:, 1:1 + S]
    m = c1 > best
    best[m], bs[m] = c1[m], s1[m]
    c2, s2 = np.where(skip, pv[:, 0:S], NEG), ps[:, 0:S]
    m = c2 > best
    best[m], bs[m] = c2[m], s2[m]
    m = f32(0) > best[:, 0]
    best[m, 0], bs[m, 0] = f32(0), t
    v = best + d[t][cls]
    assert v.dtype == np.float32
    st = np.where(v == NEG, np.int32(-1), bs).astype(np.int32)
    end_score[:, t], end_start[:, t] = v[rows, last], st[rows, last]
  return end_score, end_start


def hits(end_score, end_start, min_score, max_hits):
  """[(score, start, end)] in pick order: up to max_hits non-overlapping spans, the greatest score first, the smallest
  end on ties; candidates are the finite scores (>= min_score when it is not None)."""
  end_score = np.asarray(end_score, dtype=np.float32)
  starts = np.asarray(end_start, dtype=np.int64)
  ends = np.arange(1, len(end_score) + 1)
  free = np.isfinite(end_score)
  if min_score is not None:
    free &= end_score >= f32(min_score)
  taken = []
  while len(taken) < max_hits and free.any():
    pick = int(np.argmax(np.where(free, end_score, NEG)))   # (the first of equal maxima: the smallest end)
    s, e = int(starts[pick]), pick + 1
    taken.append((end_score[pick], s, e))
    free &= ~((starts < e) & (s < ends))
  return taken


def expected(lp, sizes, keywords, kw_lens, blank, min_scores=None, max_hits=4):
  """The whole call as the kernel writes it: lp (B, T, C) float32, sizes (B,) or None, keywords (K, kw_stride) ints,
  kw_lens (K,), min_scores (K,) or None -> dict of arrays named as lr_ctc_spot's outputs."""
  lp = np.asarray(lp, dtype=np.float32)
  B, T, C = lp.shape
  K, W = keywords.shape
  H = max_hits
  out = dict(hit_score=np.full((B, K, H), NEG, np.float32), hit_start=np.full((B, K, H), -1, np.int32),
             hit_end=np.full((B, K, H), -1, np.int32), n_hits=np.zeros((B, K), np.int32),
             status=np.zeros((B, K), np.int32), end_score=np.full((B, K, T), NEG, np.float32),
             end_start=np.full((B, K, T), -1, np.int32))
  ok = [k for k in range(K) if 1 <= int(kw_lens[k]) <= W]
  good = [k for k in ok if all(0 <= int(c) < C and int(c) != blank for c in keywords[k, :int(kw_lens[k])])]
  for b in range(B):
    n = T if sizes is None else int(sizes[b])
    if not 1 <= n <= T:
      out["status"][b] = BAD_LENGTH
      continue
    out["status"][b] = BAD_LENGTH
    out["status"][b, ok] = BAD_ID
    out["status"][b, good] = 0
    if not good:
      continue
    es, est = trace_batch(ratios(lp[b, :n]), [keywords[k] for k in good], [kw_lens[k] for k in good], blank)
    for i, k in enumerate(good):
      out["end_score"][b, k, :n], out["end_start"][b, k, :n] = es[i], est[i]
      got = hits(es[i], est[i], None if min_scores is None else min_scores[k], H)
      out["n_hits"][b, k] = len(got)
      for h, (sc, s, e) in enumerate(got):
        out["hit_score"][b, k, h], out["hit_start"][b, k, h], out["hit_end"][b, k, h] = sc, s, e
  return out


def best_by_enumeration(d, y, blank):
  """Per end frame t: (best score, set of the starts of the best paths) over ALL spans [s, t + 1) and ALL frame-level
  class sequences on the span that start on y[0], end on y[L-1] and collapse to y — (None, set()) if there is none.  In
  float64, for tiny shapes with integer values, where every sum is exact."""
  d = np.asarray(d, dtype=np.float64)
  n, C = d.shape
  y = list(y)
  out = []
  for t in range(n):
    best, starts = None, set()
    for s in range(t + 1):
      for seq in itertools.product(range(C), repeat=t + 1 - s):
        if seq[0] != y[0] or seq[-1] != y[-1] or collapse(seq, blank) != y:
          continue
        sc = sum(d[s + i, c] for i, c in enumerate(seq))
        if best is None or sc > best:
          best, starts = sc, {s}
        elif sc == best:
          starts.add(s)
    out.append((best, starts))
  return out


def keyword_batch(rng, lens, C, blank, stride=None, doubled_every=2):
  """keywords (K, stride) int32 with junk past the lengths, kw_lens (K,) int32: one keyword per entry of `lens`, every
  `doubled_every`-th with doubled letters."""
  W = stride or max(lens)
  kw = rng.randint(-5, 10 ** 6, size=(len(lens), W)).astype(np.int32)
  for k, L in enumerate(lens):
    kw[k, :L] = random_target(rng, L, C, blank, doubled=k % doubled_every == 1)
  return kw, np.array(lens, np.int32)
