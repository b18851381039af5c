"""The transducer beam search restated in plain Python and torch on the CPU, its named cases and their tolerances
(tests/test_transducer_beam_cpu.py, tests/test_gpu_transducer_beam.py).

Nothing here touches the package: the search is written out again from include/lipreading_hip.h (A6j), over the model of
tests/transducer_cases.py (A6i).  The joint stage runs in the `dtype` of the tensors it is given; scores are always
Python floats, i.e. float64.
"""
import itertools
import math

import torch

try:
  from tests import transducer_cases as TC
except ImportError:   # run as a script from this folder
  import transducer_cases as TC

NEG_INF = float("-inf")
MAX_WIDTH, MAX_SYMBOLS, MAX_U = 32, 8, 256


def logaddexp(a, b):
  m = max(a, b)
  if m == NEG_INF:
    return m
  return m + math.log(math.exp(a - m) + math.exp(b - m))


def log_probs(e_t, tables, W, b, mask, prefixes):
  """(len(prefixes), V1) masked log-softmax of the joint network at frame vector e_t for each prefix's context."""
  c0 = torch.tensor([p[-1] if len(p) > 0 else 0 for p in prefixes])
  pre = e_t[None, :] + tables[0][c0]
  if tables.shape[0] == 2:
    c1 = torch.tensor([p[-2] if len(p) > 1 else 0 for p in prefixes])
    pre = pre + tables[1][c1]
  logits = (torch.tanh(pre) @ W.t() + b).masked_fill(mask == 0, NEG_INF)
  return torch.log_softmax(logits, dim=-1).double()


def new_stats():
  """merges: prefixes merged in F.  gaps: every decision a rounding could flip: (what, gap)."""
  return dict(merges=0, gaps=[], label_rounds=0, frames=0)


def _top(entries, width, stats, what):
  """The first `width` of a stable descending sort by score; the gap between the last kept and the first dropped."""
  order = sorted(range(len(entries)), key=lambda i: -entries[i][1])   # sorted() is stable
  if stats is not None and len(order) > width:
    stats["gaps"].append((what, entries[order[width - 1]][1] - entries[order[width]][1]))
  return [entries[i] for i in order[:width]]


def new_state(B):
  return dict(beams=[[((), 0.0, ())] for _ in range(B)], truncated=[0] * B, frame_base=[0] * B)


def beam_search(e, sizes, tables, W, b, mask, beam_width=8, max_symbols=3, max_out=None, state=None, stats=None):
  """The search of lr_rnnt_beam_decode on (B, T, J) `e`; `state` (new_state) is continued in place and returned.
  state["beams"][i] is sample i's beam: a list of (prefix, score, frames), best first."""
  B, T, _ = e.shape
  V1 = W.shape[0]
  if max_out is None:
    max_out = min(T * max_symbols, MAX_U)
  st = new_state(B) if state is None else state
  labels = [k for k in range(1, V1) if mask[k] != 0]
  for i in range(B):
    n = max(0, min(int(sizes[i]), T)) if sizes is not None else T
    beam = st["beams"][i]
    for t in range(n):
      A = beam[:beam_width]
      F = {}   # prefix -> [score, frames, best own score]; dicts keep insertion order
      for s in range(max_symbols + 1):
        if not A:
          break
        lp = log_probs(e[i, t], tables, W, b, mask, [h[0] for h in A]).tolist()
        C = []
        for h, row in zip(A, lp):
          own = h[1] + row[0]
          if h[0] in F:
            ent = F[h[0]]
            ent[0] = logaddexp(ent[0], own)
            if stats is not None:
              stats["merges"] += 1
              if ent[1] != h[2]:
                stats["gaps"].append(("merge frames", abs(own - ent[2])))
            if own > ent[2]:
              ent[1], ent[2] = h[2], own
          else:
            F[h[0]] = [own, h[2], own]
          if s < max_symbols:
            if len(h[0]) < max_out:
              C += [(h[0] + (k,), h[1] + row[k], h[2] + (st["frame_base"][i] + t,)) for k in labels]
            else:
              st["truncated"][i] += 1
        if s == max_symbols:
          break
        assert len(set(c[0] for c in C)) == len(C), "a round's candidates hold a prefix twice"
        if stats is not None:
          stats["label_rounds"] += 1
        A = _top(C, beam_width, stats, "round")
      if stats is not None:
        stats["frames"] += 1
      beam = _top([(p, v[0], v[1]) for p, v in F.items()], beam_width, stats, "beam")
      assert len(set(h[0] for h in beam)) == len(beam)
    st["beams"][i] = beam
    st["frame_base"][i] += n
    if stats is not None:
      for x, y in zip(beam, beam[1:]):
        stats["gaps"].append(("reported", x[1] - y[1]))
  return st


def as_arrays(state, nbest, max_out):
  """The beams as lr_rnnt_beam_decode reports them: ids, frames (B, nbest, max_out), lens, scores (float64), count."""
  B = len(state["beams"])
  ids = torch.zeros((B, nbest, max_out), dtype=torch.int32)
  frames = torch.zeros((B, nbest, max_out), dtype=torch.int32)
  lens = torch.zeros((B, nbest), dtype=torch.int32)
  scores = torch.full((B, nbest), NEG_INF, dtype=torch.float64)
  count = torch.zeros(B, dtype=torch.int32)
  for i, beam in enumerate(state["beams"]):
    count[i] = min(len(beam), nbest)
    for n, (prefix, score, fr) in enumerate(beam[:nbest]):
      lens[i, n] = len(prefix)
      scores[i, n] = score
      if prefix:
        ids[i, n, :len(prefix)] = torch.tensor(prefix, dtype=torch.int32)
        frames[i, n, :len(prefix)] = torch.tensor(fr, dtype=torch.int32)
  return dict(ids=ids, frames=frames, lens=lens, scores=scores, count=count,
              truncated=torch.tensor(state["truncated"], dtype=torch.int32))


# ---- the exhaustive yardsticks -----------------------------------------------------------------------------------------
def prefix_log_probs(e_i, tables, W, b, mask, prefix):
  """(T, U + 1, V1): the joint network's log-probabilities over the lattice of `prefix` (A6i's lp(t, u))."""
  y = (0, 0) + tuple(prefix)
  p = torch.stack([tables[0][y[u + 1]] + (tables[1][y[u]] if tables.shape[0] == 2 else 0) for u in range(len(prefix) + 1)])
  return TC.joint_log_probs(e_i[None], p[None], W, b, mask)[0]


def brute_force_score(e_i, Tb, tables, W, b, mask, prefix, max_symbols):
  """log of the summed probability of every alignment of `prefix` over Tb frames that emits at most max_symbols labels
  in a frame and ends every frame with a blank, alignment by alignment.  -inf when there is none."""
  lp = prefix_log_probs(e_i, tables, W, b, mask, prefix).double()
  U, total = len(prefix), NEG_INF
  for per_frame in itertools.product(range(max_symbols + 1), repeat=Tb):
    if sum(per_frame) != U:
      continue
    u, s = 0, 0.0
    for t, n in enumerate(per_frame):
      for _ in range(n):
        s += float(lp[t, u, prefix[u]])
        u += 1
      s += float(lp[t, u, 0])
    total = logaddexp(total, s)
  return total


def lattice_score(e_i, Tb, tables, W, b, mask, prefix):
  """-nll(prefix) of A6i's loss: every alignment, without a cap on labels per frame."""
  lp = prefix_log_probs(e_i, tables, W, b, mask, prefix).double()
  return -float(TC.lattice_nll(lp, torch.tensor(prefix, dtype=torch.int64), Tb, len(prefix)))


def make_tensors(B, T, V1, J, context, seed, dtype=torch.float64):
  """Tensors drawn as transducer_cases.make_case draws them, from a seed of the caller's."""
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  mask = torch.ones(V1, dtype=torch.float64)
  for c in ((3,) if V1 < 9 else (2, 5)):
    mask[c] = 0
  W = r(V1, J) * (3.0 / J ** 0.5)
  b = r(V1) * 0.1
  b[0] += 2.0
  out = dict(e=r(B, T, J), W=W, b=b, mask=mask, tables=r(context, V1, J) * 0.7)
  return {k: v.to(dtype) for k, v in out.items()}


# Exhaustive inputs: V1 = 4 with class 3 masked leaves two labels.  (T, max_symbols, beam_width, prefixes that exist):
# T = 2 and two labels a frame reach every string of at most 4 labels, 31 of them, and no round has more than 28
# candidates, so a beam of 32 prunes nothing; T = 3 and one label a frame reach the 15 strings of at most 3.
EXHAUSTIVE = {"t2s2": (2, 2, 32, 31), "t3s1": (3, 1, 32, 15)}


def exhaustive_case(name, dtype=torch.float64):
  T, max_symbols, beam_width, nprefix = EXHAUSTIVE[name]
  c = make_tensors(1, T, 4, 8, 2, 4242 + T, dtype)
  c.update(sizes=torch.tensor([T], dtype=torch.int32), beam_width=beam_width, max_symbols=max_symbols,
           max_out=T * max_symbols, nprefix=nprefix, name=name)
  return c


# ---- the named cases ---------------------------------------------------------------------------------------------------
# name: (tensors, sizes, beam_width, max_symbols).  tensors: a case name of transducer_cases.CASES (its e, tables, W, b
# and mask) or (B, T, V1, J, context, seed) for make_tensors.  `ragged` has a sample without frames; `odd` a V1 (37)
# and a J (45) that are multiples of neither 32 nor 4; `ragged` is context 1, the others context 2; the widths are 1, 4,
# 8 and 32.  Seeds of the cases with their own tensors: chosen for the margin from the print-out of `python
# tests/transducer_beam_cases.py search NAME`.
CASES = {
    "ragged": ("ragged", [9, 0, 5], 4, 2),
    "vocab": ("vocab", [17, 12, 9, 17], 4, 2),
    "wide": ("wide", [5, 4], 4, 2),
    "odd": ("odd", [6, 5], 4, 2),
    "odd_w1": ("odd", [6, 5], 1, 2),
    "maxu": ("maxu", [2, 2], 4, 2),
    "small_w32": ((2, 7, 7, 12, 2, 7001), [7, 4], 32, 2),
    "workload": ((2, 75, 65, 256, 2, 7125), [75, 60], 8, 3),
}


def make_case(name, dtype=torch.float64):
  src, sizes, beam_width, max_symbols = CASES[name]
  if isinstance(src, str):
    c = TC.make_case(src, dtype)
    c = {k: c[k] for k in ("e", "tables", "W", "b", "mask")}
  else:
    c = make_tensors(*src, dtype=dtype)
  T = c["e"].shape[1]
  c.update(sizes=torch.tensor(sizes, dtype=torch.int32), beam_width=beam_width, max_symbols=max_symbols,
           max_out=min(T * max_symbols, MAX_U), name=name)
  return c


def run(c, **kw):
  """The restatement on a case dict; keyword arguments override the case's own settings."""
  a = dict(beam_width=c["beam_width"], max_symbols=c["max_symbols"], max_out=c["max_out"])
  a.update(kw)
  return beam_search(c["e"], c["sizes"], c["tables"], c["W"], c["b"], c["mask"], **a)


_REFERENCES = {}


def reference(name):
  """(case, state, stats, arrays) of the float64 restatement, computed once per process; callers leave it unchanged."""
  if name not in _REFERENCES:
    c = make_case(name) if name in CASES else exhaustive_case(name)
    stats = new_stats()
    st = run(c, stats=stats)
    _REFERENCES[name] = (c, st, stats, as_arrays(st, c["beam_width"], c["max_out"]))
  return _REFERENCES[name]


def smallest_gap(stats):
  return min((g for _, g in stats["gaps"]), default=float("inf"))


def fp32_error(name):
  """(float32 restatement's largest score error, largest |score|) over the beams; None when float32 took another path."""
  c, st, _, _ = reference(name)
  c32 = make_case(name, torch.float32) if name in CASES else exhaustive_case(name, torch.float32)
  st32 = run(c32)
  err, scale = 0.0, 0.0
  for b64, b32 in zip(st["beams"], st32["beams"]):
    if [h[0] for h in b64] != [h[0] for h in b32] or [h[2] for h in b64] != [h[2] for h in b32]:
      return None
    for h64, h32 in zip(b64, b32):
      err = max(err, abs(h64[1] - h32[1]))
      scale = max(scale, abs(h64[1]))
  return err, scale


# name: (the float32 restatement's score error relative to the largest |score|, the largest |score|, the smallest gap,
# merges).  MEASURED by `python tests/transducer_beam_cases.py` (torch on the CPU, the run of this file's commit).  A
# device score may differ from the float64 restatement's by TOL_FACTOR x the error (not below 2^-24: a float32 word holds
# no more) x the largest |score|; a case is a yardstick only while its smallest gap is MARGIN_FACTOR x the error, taken
# relative or absolute, whichever is larger.
FP32_ERROR = {
    "ragged": (5.07e-08, 5.34, 0.00184, 20),   # gap / error 5778, label rounds per frame 2.00
    "vocab": (6.7e-08, 37.6, 0.000665, 20),   # gap / error 264, label rounds per frame 2.00
    "wide": (6.66e-08, 24.6, 0.00355, 9),   # gap / error 2161, label rounds per frame 2.00
    "odd": (7.5e-08, 11.2, 0.0156, 7),   # gap / error 18551, label rounds per frame 2.00
    "odd_w1": (2.33e-09, 9.31, 0.0417, 0),   # gap / error 75135, label rounds per frame 2.00
    "maxu": (1.41e-07, 6.22, 0.023, 0),   # gap / error 26186, label rounds per frame 2.00
    "small_w32": (1.09e-07, 8.83, 0.00246, 287),   # gap / error 2550, label rounds per frame 2.00
    "workload": (2.61e-08, 85.2, 0.000764, 221),   # gap / error 150, label rounds per frame 3.00
    "t2s2": (4.27e-08, 17.1, 0.0293, 18),   # gap / error 28660, label rounds per frame 2.00
    "t3s1": (4.13e-08, 21.6, 0.0669, 8),   # gap / error 52053, label rounds per frame 1.00
}
TOL_FACTOR = TC.TOL_FACTOR
MARGIN_FACTOR = TC.MARGIN_FACTOR
FP32_HALF_ULP = TC.FP32_HALF_ULP


def score_tolerance(name):
  """The absolute tolerance of the case's device scores."""
  rel, scale = FP32_ERROR[name][0], FP32_ERROR[name][1]
  return TOL_FACTOR * max(rel, FP32_HALF_ULP) * max(scale, 1.0)


def margin_holds(name, stats=None):
  """The oracle's own condition: the smallest gap of the float64 run (`stats`: of a variant of the case) against the
  tabled float32 error."""
  rel, scale = FP32_ERROR[name][0], FP32_ERROR[name][1]
  rel = max(rel, FP32_HALF_ULP)
  return smallest_gap(reference(name)[2] if stats is None else stats) >= MARGIN_FACTOR * max(rel, rel * scale)


def measure(names):
  for name in names:
    _, _, stats, _ = reference(name)
    fe = fp32_error(name)
    gap = smallest_gap(stats)
    if fe is None:
      print('    # "%s": the float32 restatement takes another path (smallest gap %.3g)' % (name, gap))
      continue
    err, scale = fe
    rel = err / (scale if scale > 0 else 1.0)
    floor = max(rel, FP32_HALF_ULP)
    print('    "%s": (%.3g, %.3g, %.3g, %d),   # gap / error %.0f, label rounds per frame %.2f'
          % (name, rel, scale, gap, stats["merges"], gap / max(floor, floor * scale),
             stats["label_rounds"] / max(stats["frames"], 1)))


def search(name, tries=40):
  """Print the first seeds of an own-tensor case for which the margin condition holds."""
  src, sizes, beam_width, max_symbols = CASES[name]
  for seed in range(src[5], src[5] + tries):
    CASES[name] = (src[:5] + (seed,), sizes, beam_width, max_symbols)
    _REFERENCES.pop(name, None)
    fe = fp32_error(name)
    gap = smallest_gap(reference(name)[2])
    if fe is None:
      continue
    floor = max(fe[0] / max(fe[1], 1e-30), FP32_HALF_ULP)
    ratio = gap / max(floor, floor * fe[1])
    print("%s seed %d: gap %.3g ratio %.0f merges %d" % (name, seed, gap, ratio, reference(name)[2]["merges"]))
    if ratio >= 4 * MARGIN_FACTOR:
      break


if __name__ == "__main__":
  import sys
  if len(sys.argv) > 2 and sys.argv[1] == "search":
    search(sys.argv[2])
  else:
    measure(list(CASES) + list(EXHAUSTIVE))
