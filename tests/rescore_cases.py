"""Attention rescoring of CTC N-best lists (lipreading_amd/csrc/lr_attn_rescore.hip): the float64
restatement of the rule on oracle.torch_oracle.OracleCharDecodingStep, and the hypothesis lists the CPU and GPU tests
share.  The restatement is built on `rescore` of tests/test_attn_beam_cpu.py (one teacher-forced float64 pass per
hypothesis); `many=True` takes the batched pass of tests/test_gpu_attn_beam.py instead, which computes the same sums
for a whole utterance at once."""
import math

import numpy as np
import torch

from tests.test_attn_beam_cpu import BOS, EOS, PAD, rescore

SCORABLE, UNSCORABLE, EMPTY = 0, 1, 2
NEG_INF = float("-inf")


def scored_sequence(classes, length, first, V, bos=BOS, eos=EOS, pad=PAD):
  """One slot by the rule -> (class of the slot, q): q is None for an empty slot; else the decoder tokens up to and
  including the first EOS, or all of them and one EOS."""
  if math.isnan(first) or (length == 0 and first == float("inf")):
    return EMPTY, None
  q = []
  for k in list(classes)[:length]:
    q.append(int(k) - 1)
    if q[-1] == eos:
      break
  if not q or q[-1] != eos:
    q.append(eos)
  ok = all(0 <= v < V and v not in (pad, bos) for v in q)
  return (SCORABLE if ok else UNSCORABLE), q


def combined(a, f, n, lam, gamma):
  """s of the rule in float64; a term whose weight is exactly 0 is left out."""
  s = gamma * n
  if lam != 1.0:
    s += (1.0 - lam) * a
  if lam != 0.0:
    s -= lam * f
  return s


def rescore_ref(dec, enc, enc_lens, prev, hyp_ids, hyp_lens, first, lam, gamma, many=False):
  """The rule in float64.  hyp_ids [B][N][W] CTC classes, hyp_lens [B][N], first [B][N] (-log P of the first pass).
  Per utterance a dict: order (the input slot at each rank), s and a (ranked; -inf where the slot is not scored),
  cls (per SLOT: SCORABLE / UNSCORABLE / EMPTY), q (per slot, None for an empty one), s_slot and a_slot (per slot)."""
  V = dec.vocab_size
  out = []
  for b in range(len(hyp_ids)):
    N = len(hyp_ids[b])
    cls, qs = [], []
    for n in range(N):
      c, q = scored_sequence(hyp_ids[b][n], int(hyp_lens[b][n]), float(first[b][n]), V)
      cls.append(c)
      qs.append(q)
    live = [n for n in range(N) if cls[n] == SCORABLE]
    a_slot, s_slot = [NEG_INF] * N, [NEG_INF] * N
    if live:
      if many:
        from tests.test_gpu_attn_beam import rescore_many
        a_live = rescore_many(dec, enc, enc_lens, prev, b, [qs[n] for n in live])
      else:
        a_live = [rescore(dec, enc, enc_lens, prev, b, qs[n]) for n in live]
      for n, a in zip(live, a_live):
        s = combined(float(a), float(first[b][n]), len(qs[n]), lam, gamma)
        if math.isnan(s):
          cls[n] = UNSCORABLE
        else:
          a_slot[n], s_slot[n] = float(a), s
    order = (sorted((n for n in range(N) if cls[n] == SCORABLE), key=lambda n: -s_slot[n]) +   # stable
             [n for n in range(N) if cls[n] == UNSCORABLE] + [n for n in range(N) if cls[n] == EMPTY])
    out.append(dict(order=order, s=[s_slot[n] for n in order], a=[a_slot[n] for n in order], cls=cls, q=qs,
                    s_slot=s_slot, a_slot=a_slot))
  return out


KINDS = ("no_eos", "eos_mid", "len0", "pad", "blank", "empty")


def random_lists(B, N, W, V, seed, wide=(3, 5)):
  """Random N-best lists for B utterances -> (ids, lens, first): ids an int32 tensor (B, N + wide[0], W + wide[1])
  filled with -1 past each length (the caller passes ids[:, :N, :W], a strided view), lens (B, N) int32, first (B, N)
  float32.  Lengths are random in [0, W], tokens random over the characters (no marker), about half of the slots
  carry an EOS somewhere; a slot whose scored sequence another slot of the utterance already has is drawn again (two
  equal sequences tie exactly at lambda = 0).  Slot kinds every utterance holds when N >= 6, one slot each, at random places: no EOS; an
  EOS in the middle with junk (markers included) after it; length 0 with a finite score (the empty transcript); a PAD
  token; a blank (class 0); an empty slot (length 0, +inf).  With N < 6 the kinds go round over the utterances.  One
  utterance in four also holds a NaN score (an empty slot by the rule) when N >= 8.  The first-pass scores are random
  in [0, max(60, 4 N)): tens of nats apart, as the attention sums are, and wider for the long lists, whose number of
  close pairs grows with N squared."""
  g = np.random.RandomState(seed)
  ids = -np.ones((B, N + wide[0], W + wide[1]), dtype=np.int32)
  lens = np.zeros((B, N), dtype=np.int32)
  first = np.zeros((B, N), dtype=np.float32)
  chars = [v for v in range(V) if v not in (PAD, BOS, EOS)]
  for b in range(B):
    first[b] = g.uniform(0.0, max(60.0, 4.0 * N), size=N)
    kinds = list(KINDS) if N >= 6 else [KINDS[(b * N + i) % len(KINDS)] for i in range(N)]
    slots = g.permutation(N)[:len(kinds)]
    seen = set()   # the scored sequences so far: two slots with one sequence tie exactly at lambda = 0
    for kind, n in zip(kinds, slots):
      ln = min(W, max(1 if W == 1 else 2, int(g.randint(0, W + 1))))
      body = g.choice(chars, size=ln) + 1
      if kind == "eos_mid":
        at = int(g.randint(0, max(1, ln - 1)))
        body[at] = EOS + 1
        body[at + 1:] = g.choice([PAD + 1, BOS + 1, 0, V + 5, EOS + 1], size=ln - at - 1)   # junk: never looked at
      elif kind == "pad":
        body[int(g.randint(0, ln))] = PAD + 1
      elif kind == "blank":
        body[int(g.randint(0, ln))] = 0
      if kind in ("len0", "empty"):
        ln, body = 0, body[:0]
        if kind == "empty":
          first[b, n] = np.inf
      ids[b, n, :ln] = body
      lens[b, n] = ln
      seen.add(tuple(scored_sequence(body, ln, float(first[b, n]), V)[1] or ()))
    for n in range(N):
      if n in set(slots.tolist()):
        continue
      for _ in range(50):   # (W = 1 has too few sequences for a long list: what repeats then, repeats)
        ln = int(g.randint(0, W + 1))
        toks = g.choice(chars, size=ln)
        if ln and g.rand() < 0.5:
          toks[g.randint(0, ln)] = EOS
        q = tuple(scored_sequence(toks + 1, ln, 1.0, V)[1])
        if q not in seen:
          break
      seen.add(q)
      ids[b, n, :ln] = toks + 1
      lens[b, n] = ln
    if N >= 8 and b % 4 == 1:
      free = [n for n in range(N) if n not in set(slots.tolist())]
      first[b, free[0]] = np.nan
  return torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(first)
