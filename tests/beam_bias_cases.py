"""Helpers for the hotword tests (tests/test_beam_bias_cpu.py, tests/test_gpu_beam_bias.py; not collected): the
specification's bonus by brute force over substrings (no automaton, so it checks the automaton), beam_bias_ref, the
float64 restatement of lr_ctc_beam_bias_decode / lr_ctc_beam_lm_bias_decode (lipreading_amd/csrc/lr_ctc_beam.hip),
exhaustive enumeration with the end bonus, and the frames of the readable cases."""
import numpy as np

from tests.test_beam_cpu import beam_ref, enumerate_labellings, prune, softmax_frames  # noqa: F401
from tests.test_beam_lm_cpu import Dict, RefLM, enumerate_lm  # noqa: F401

NEG_INF = -np.inf


class Bias(object):
  """phrases [(class ids, weight)], anchor (class id or -1).  Prefixes are handled as bytes (class ids < 256) so that
  the substring searches are the interpreter's own."""

  def __init__(self, phrases, anchor=-1, partial_credit=True):
    self.phrases = [(bytes(q), float(w)) for q, w in phrases]
    self.anchor = anchor
    self.partial_credit = partial_credit
    self._end, self._run = {}, {}

  def admissible(self, y, i):
    return self.anchor < 0 or i == 0 or y[i - 1] == self.anchor

  def occ(self, y, q):
    """admissible i with y[i:i+m] == q; overlaps count"""
    n, i = 0, y.find(q)
    while i >= 0:
      n += self.admissible(y, i)
      i = y.find(q, i + 1)
    return n

  def bonus_end(self, y):
    y = bytes(y)
    if y not in self._end:
      self._end[y] = sum(w * self.occ(y, q) for q, w in self.phrases)
    return self._end[y]

  def partial(self, y):
    y = bytes(y)
    best = 0.0
    for q, w in self.phrases:
      for j in range(1, len(q)):
        if j <= len(y) and y.endswith(q[:j]) and self.admissible(y, len(y) - j):
          best = max(best, w * j / len(q))
    return best

  def bonus_run(self, y):
    y = bytes(y)
    if y not in self._run:
      self._run[y] = self.bonus_end(y) + (self.partial(y) if self.partial_credit else 0.0)
    return self._run[y]


def bonus_end(y, phrases, anchor=-1):
  return Bias(phrases, anchor).bonus_end(y)


def bonus_run(y, phrases, anchor=-1):
  return Bias(phrases, anchor).bonus_run(y)


def beam_bias_ref(v, size, beam_width, cutoff_top_n, bias, cutoff_prob=1.0, blank=0, log_input=False, lm=None,
                  dic=None, alpha=0.0, beta=0.0):
  """beam_ref (lm None) or beam_lm_ref plus the hotwords: the masses evolve as there, the selection key of a
  candidate is its score + bonus_run(its prefix), and the end re-sorts by log mass (+ the LM's end term) + bonus_end.
  Returns [(ids, offsets, -final score)], best first."""
  roles = dic.roles if lm is not None else None

  def term(node, ctx):
    return alpha * lm.lm_score(ctx, dic.word[node]) + beta if node else 0.0

  # (prefix, log p_blank, log p_nonblank, offsets, trie node, completed words, term)
  beam = [((), 0.0, NEG_INF, (), 0, (), 0.0)]
  for t in range(size):
    if not beam:   # the dictionary left no hypothesis (a narrow beam under a language model)
      break
    keep, lp = prune(v[t], cutoff_top_n, cutoff_prob, log_input)
    c2k = {int(c): k for k, c in enumerate(keep)}
    W = len(beam)
    pb = np.array([h[1] for h in beam])
    pnb = np.array([h[2] for h in beam])
    score = np.logaddexp(pb, pnb)
    last = np.array([h[0][-1] if h[0] else -1 for h in beam])
    own_pb = score + lp[c2k[blank]] if blank in c2k else np.full(W, NEG_INF)
    own_pnb = np.full(W, NEG_INF)
    for i in range(W):
      if last[i] in c2k:
        own_pnb[i] = pnb[i] + lp[c2k[int(last[i])]]
    ext = np.where(keep[None, :] == last[:, None], pb[:, None], score[:, None]) + lp[None, :]
    ext[:, keep == blank] = NEG_INF
    if lm is not None:
      kr = np.array([roles[int(c)] for c in keep])
      nodes = np.array([h[4] for h in beam], np.int64)
      child = dic.child[nodes][:, keep]
      ext = np.where((kr[None, :] == 1) & (child < 0), NEG_INF, ext)
      ext = ext + np.where(kr[None, :] == 2, np.array([h[6] for h in beam])[:, None], 0.0)
    rank = {h[0]: i for i, h in enumerate(beam)}
    for q, h in enumerate(beam):
      if h[0] and h[0][-1] in c2k and h[0][:-1] in rank:
        i, k = rank[h[0][:-1]], c2k[h[0][-1]]
        own_pnb[q] = np.logaddexp(own_pnb[q], ext[i, k])
        ext[i, k] = NEG_INF
    own = np.logaddexp(own_pb, own_pnb)
    sc = np.concatenate([own, ext.ravel()])
    par = np.concatenate([np.arange(W), np.repeat(np.arange(W), len(keep))])
    tb = np.concatenate([np.zeros(W, np.int64), np.tile(1 + keep.astype(np.int64), W)])
    valid = np.nonzero(sc > NEG_INF)[0]
    # the selection key: the bonus of the candidate's own prefix
    key = np.full(len(sc), NEG_INF)
    for s in valid:
      pre = beam[int(par[s])][0]
      if s >= W:
        pre = pre + (int(keep[(s - W) % len(keep)]),)
      key[s] = sc[s] + bias.bonus_run(pre)
    order = valid[np.lexsort((tb[valid], par[valid], -key[valid]))][:beam_width]
    nxt = []
    for s in order:
      i = int(par[s])
      pre, _, _, off, node, ctx, tm = beam[i]
      if s < W:
        nxt.append((pre, own_pb[i], own_pnb[i], off, node, ctx, tm))
        continue
      c = int(keep[(s - W) % len(keep)])
      if lm is None:
        nxt.append((pre + (c,), NEG_INF, sc[s], off + (t,), 0, (), 0.0))
      elif roles[c] == 1:
        nd = int(dic.child[node, c])
        nxt.append((pre + (c,), NEG_INF, sc[s], off + (t,), nd, ctx, term(nd, ctx)))
      else:
        ctx2 = ctx + (dic.word[node] or "\0oov",) if roles[c] == 2 and node else ctx
        nxt.append((pre + (c,), NEG_INF, sc[s], off + (t,), 0, ctx2, 0.0))
    beam = nxt
  fin = [float(np.logaddexp(h[1], h[2])) + h[6] + bias.bonus_end(h[0]) for h in beam]
  order = sorted(range(len(beam)), key=lambda r: (-fin[r], r))
  return [(beam[r][0], beam[r][3], -fin[r]) for r in order]


def enumerate_bias(v, bias, log_input=False, blank=0, labels=None, lm=None, dic=None, alpha=0.0, beta=0.0):
  """Every labelling's mass (enumerate_labellings, or enumerate_lm with a language model) and its bonus_end:
  [(labelling, -(log mass (+ LM terms) + bonus_end))], best first."""
  if lm is None:
    base = enumerate_labellings(v, log_input, blank)
  else:
    base = enumerate_lm(v, labels, lm, dic, alpha, beta, log_input, blank)
  return sorted(((lab, s - bias.bonus_end(lab)) for lab, s in base), key=lambda kv: kv[1])


# ------------------------------------------------------------------------------------------------------------------
# the readable cases
# ------------------------------------------------------------------------------------------------------------------
TRAP_LABELS = ["_", " "] + list("abcdefghijklmnopqrstuvwxyz")


def spell_ids(text, labels=TRAP_LABELS):
  return tuple(labels.index(ch) for ch in text)


def _frames(spec, labels=TRAP_LABELS):
  """One frame per dict {label: probability}, the rest spread over the other classes; a blank frame after each."""
  C = len(labels)
  out = []
  for f in spec:
    for d in (f, {"_": 0.97}):
      row = np.full(C, (1.0 - sum(d.values())) / (C - len(d)), np.float64)
      for l, p in d.items():
        row[labels.index(l)] = p
      out.append(row)
  return np.asarray(out, np.float32)


def homophene_frames():
  """'ban' a little ahead of 'pan' and 'man': the first letter is the only doubt."""
  return _frames([{"b": 0.45, "p": 0.35, "m": 0.15}, {"a": 0.95}, {"n": 0.95}])


def pruned_prefix_frames():
  """At beam_width 2 the first frame keeps 'b' and 'm'; 'p' survives only with the partial credit of 'pan'."""
  return _frames([{"b": 0.5, "m": 0.3, "p": 0.15}, {"a": 0.95}, {"n": 0.95}])


def channel_frames():
  """'chanmel' ahead of 'channel': 'ann' inside the word helps only when it may match anywhere."""
  return _frames([{"c": 0.95}, {"h": 0.95}, {"a": 0.95}, {"n": 0.95}, {"m": 0.55, "n": 0.40}, {"e": 0.95},
                  {"l": 0.95}])
