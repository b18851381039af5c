"""Shared by tests/test_frontend_stream_cpu.py and tests/test_gpu_frontend_stream.py: the conv frontend session
(lr_conv_stream_*) restated in torch float64, the exact-integer cases and the chunkings both
files use.  Host only: no GPU, no import of the extension.

A session keeps, per slot and per layer, the last two input frames (a ring, zero after a reset) and counters.  With n
clip frames consumed a slot holds p1 = n or max(0, n - 1) frames of pooled layer-1 output, p2 = p1 or max(0, p1 - 1) of
layer 2, p3 likewise of features: the first value once the stream has ended (the frame after the last one is the zero
padding), the second while it runs.  So E(n, ended) = n if ended else max(0, n - 3) feature frames have been emitted,
and an advance returns E(after) - E(before) of them.

The exact-integer argument is tests/frontend_exact_cases.py's: operands that are small integers, every pre-pool value
an integer whose positive part is <= 256 (a bf16 value), so that the bf16 / fp32 kernels equal fp64 exactly in any
summation order and a dropped, doubled or misplaced tap moves an output by at least 1.
"""
import collections
import functools

import torch

from tests.frontend_exact_cases import (BF16_EXACT, L1, L2, L3, clip_to_ndhwc, compare_exact,  # noqa: F401
                                        conv_forward, relu_pool)

LAYERS = (L1, L2, L3)
LOOKAHEAD = 3     # feature frame t needs clip frames up to t + 3
RING = 2          # input frames of a layer a slot keeps


def emitted(n, ended):
  """E(n, ended): feature frames a slot has emitted after n clip frames."""
  return n if ended else max(0, n - LOOKAHEAD)


def level_counts(n, ended, ahead=(1, 1, 1)):
  """[n, p1, p2, p3]: frames of every level a slot holds after n clip frames."""
  out = [n]
  for a in ahead:
    out.append(out[-1] if ended else max(0, out[-1] - a))
  return out


def feature_dim(H, W):
  return 96 * (H // 16) * (W // 16)


def bf16_round(x):
  return x.float().to(torch.bfloat16).double()


# ---------------------------------------------------------------------------------------------------------------
# one-shot fp64 frontend on one unpadded clip
# ---------------------------------------------------------------------------------------------------------------
def oneshot(x, ws, bs, round_bf16=False, keep_levels=False):
  """x [1][T][H][W][3] float64 -> features [T][F] ((h, w, c) order): conv_forward then relu_pool, three times; with
  round_bf16 every level is rounded to bf16 where the kernels store it.  keep_levels: also the pre-pool values and the
  pooled values of every level (for the exactness conditions)."""
  pre, pooled = [], []
  for L, w, b in zip(LAYERS, ws, bs):
    z = conv_forward(x, w, b, False, L.stride, L.pad)
    if round_bf16:
      z = bf16_round(z)
    x = relu_pool(z)[0]
    pre.append(z)
    pooled.append(x)
  feats = x.reshape(x.shape[1], -1)
  return (feats, pre, pooled) if keep_levels else feats


# ---------------------------------------------------------------------------------------------------------------
# the session in fp64: explicit rings, the emission rule, optional bf16 rounding between levels
# ---------------------------------------------------------------------------------------------------------------
class StreamRef(object):
  """One slot.  feed(frames [s][H][W][3] float64, end) -> the newly completed feature frames [count][F].

  The keyword arguments are the session's constants; the CPU test sets each to a wrong value and asks that the
  equality with the one-shot frontend breaks: ring (depth of the frame rings), zero_after (the plane after the last
  frame is zero; False: the last frame again), ahead (frames a layer waits for; (1, 1, 0) is an emission delay of 2,
  the missing frame read as zero), zero_before (the plane before frame 0 is zero; False: frame 0 again)."""

  def __init__(self, ws, bs, H, W, round_bf16=False, ring=RING, zero_after=True, ahead=(1, 1, 1), zero_before=True):
    self.ws, self.bs, self.round = ws, bs, round_bf16
    self.depth, self.zero_after, self.ahead, self.zero_before = ring, zero_after, tuple(ahead), zero_before
    dims = ((H, W, 3), (H // 4, W // 4, 32), (H // 8, W // 8, 64))
    self.rings = [[torch.zeros(d, dtype=torch.float64) for _ in range(ring)] for d in dims]
    self.first = [None, None, None]     # frame 0 of every level (zero_before=False reads it)
    self.n, self.ended = 0, False
    self.F = feature_dim(H, W)

  def _plane(self, l, g, before, after, new):
    zero = torch.zeros_like(self.rings[l][0])
    if g < 0:
      return zero if self.zero_before or self.first[l] is None else self.first[l]
    if g >= after:
      if self.ended and not self.zero_after and after > 0:
        return self._plane(l, after - 1, before, after, new)
      return zero
    if g >= before:
      return new[g - before]
    r = g - (before - self.depth)
    return self.rings[l][r] if r >= 0 else zero

  def feed(self, frames, end=False):
    if self.ended:
      assert frames.shape[0] == 0, "frames after the end"
      return torch.zeros((0, self.F), dtype=torch.float64)
    before = level_counts(self.n, False, self.ahead)
    self.n += frames.shape[0]
    self.ended = bool(end)
    after = level_counts(self.n, self.ended, self.ahead)
    new = list(frames.double())
    for l, (L, w, b) in enumerate(zip(LAYERS, self.ws, self.bs)):
      if self.first[l] is None and new:
        self.first[l] = new[0]
      outs = []
      for t in range(before[l + 1], after[l + 1]):
        x = torch.stack([self._plane(l, t - 1 + kt, before[l], after[l], new) for kt in range(3)])[None]
        z = conv_forward(x, w, b, False, L.stride, (0,) + tuple(L.pad[1:]))
        if self.round:
          z = bf16_round(z)
        outs.append(relu_pool(z)[0][0, 0])
      self.rings[l] = (self.rings[l] + new)[-self.depth:]
      new = outs
    return torch.stack(new).reshape(len(new), -1) if new else torch.zeros((0, self.F), dtype=torch.float64)


Call = collections.namedtuple("Call", "t0 chunk sizes end")


def schedule(lens, chunking, end_with=True):
  """The advances that feed clips of `lens` frames in chunks of `chunking` frames (a list summing to >= max(lens)):
  slot b consumes min(chunk, what it has left) frames of clips[:, t0:t0 + chunk] and ends with its last frames
  (end_with) or in the call after them, in which it is idle — an empty call if there is none."""
  calls, t0, pending = [], 0, [False] * len(lens)
  done = [False] * len(lens)
  for chunk in chunking:
    sizes = [min(chunk, max(0, n - t0)) for n in lens]
    end = [0] * len(lens)
    for b, n in enumerate(lens):
      last = not done[b] and t0 + sizes[b] >= n
      if pending[b]:
        end[b], pending[b] = 1, False
      elif last:
        done[b] = True
        if end_with:
          end[b] = 1
        else:
          pending[b] = True
    calls.append(Call(t0, chunk, tuple(sizes), tuple(end)))
    t0 += chunk
  assert t0 >= max(lens), "the chunking does not cover the clips"
  if any(pending):
    calls.append(Call(t0, 0, (0,) * len(lens), tuple(int(p) for p in pending)))
  return calls


def stream_ref(x, lens, ws, bs, calls, **kw):
  """x [B][T][H][W][3] float64, slot b holding lens[b] frames: the features [lens[b]][F] of every slot fed by `calls`,
  and per call the counts a session returns."""
  B, H, W = x.shape[0], x.shape[2], x.shape[3]
  slots = [StreamRef(ws, bs, H, W, **kw) for _ in range(B)]
  feats, counts = [[] for _ in range(B)], []
  for c in calls:
    row = []
    for b in range(B):
      got = slots[b].feed(x[b, c.t0:c.t0 + c.sizes[b]], bool(c.end[b])) if (c.sizes[b] or c.end[b]) else None
      row.append(0 if got is None else got.shape[0])
      if got is not None:
        feats[b].append(got)
    counts.append(row)
  F = feature_dim(H, W)
  return [torch.cat(f) if f else torch.zeros((0, F), dtype=torch.float64) for f in feats], counts


# ---------------------------------------------------------------------------------------------------------------
# exact-integer cases
# ---------------------------------------------------------------------------------------------------------------
# Clips of the bytes {0, 255} (density 0.5), ternary weights kept with probability KEEP per layer, integer biases in
# BIAS: sparse enough upstairs that every pre-pool value stays an integer with positive part <= 256, dense enough that
# at least 10 % of every level's pooled values are non-zero (test_frontend_stream_cpu.py asserts both for every case).
# A one-frame utterance sees one of the three temporal taps, so its sums are a third of a long clip's: the biases of
# layers 2 and 3 are milder than a long clip alone would allow ((-40, -20) and (-6, 2) leave 1 % of a one-frame slot's
# layer-2 values alive), and the conditions are asserted per SLOT, not per batch.  Measured over seeds 0-2: the largest
# pre-pool value is 221 (32 x 32, layer 3), the smallest non-zero share 0.11 (the one-frame slot, layer 2).
KEEP = (0.4, 0.03, 0.005)
BIAS = ((-4, 2), (-20, -6), (-4, 2))

Case = collections.namedtuple("Case", "name H W lens seed")
# utterances of 1, 2, 3 and 4 frames sit where the ring and the end logic can go wrong; 9 crosses every chunking
CASES = (Case("sq16", 16, 16, (1, 2, 3, 4, 9), 1),
         Case("sq32", 32, 32, (7, 4), 0),
         Case("r16x32", 16, 32, (5, 3), 0))
BY_NAME = {c.name: c for c in CASES}


def chunkings(T):
  """Chunkings of a batch whose longest clip has T frames."""
  out = [[T], [1] * T]
  if T == 9:
    out += [[2, 3, 4], [4, 1, 1, 3]]
  elif T >= 4:
    out += [[2] * ((T + 1) // 2), [3, 1] + [T - 4] * (T > 4), [T - 1, 1]]
  return out


class Problem(object):
  def __init__(self, case):
    self.case = case
    g = torch.Generator().manual_seed(case.seed)
    B, T = len(case.lens), max(case.lens)
    self.clip = (torch.rand((B, T, 3, case.H, case.W), generator=g) < 0.5).to(torch.uint8) * 255
    self.ws, self.bs = [], []
    for L, keep, (lo, hi) in zip(LAYERS, KEEP, BIAS):
      shape = (L.cout, L.cin) + L.k
      w = torch.randint(-1, 2, shape, generator=g).double() * (torch.rand(shape, generator=g) < keep).double()
      self.ws.append(w)
      self.bs.append(torch.randint(lo, hi + 1, (L.cout,), generator=g).double())
    self.x = clip_to_ndhwc(self.clip)

  @functools.cached_property
  def levels(self):
    """per slot: (features [len][F], pre-pool values per level, pooled values per level) of the one-shot frontend on
    the slot's unpadded clip"""
    return [oneshot(self.x[b:b + 1, :n], self.ws, self.bs, keep_levels=True) for b, n in enumerate(self.case.lens)]

  @functools.cached_property
  def features(self):
    return [lv[0] for lv in self.levels]


@functools.lru_cache(maxsize=None)
def problem(name):
  return Problem(BY_NAME[name])
