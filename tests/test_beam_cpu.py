"""CPU: a plain float64 restatement of lr_ctc_beam_decode's specification (lipreading_amd/csrc/lr_ctc_beam.hip),
checked against exhaustive enumeration of every alignment, and the host-side rejections of BeamCTCDecoder and the
C ABI (no device needed).  tests/test_gpu_beam.py holds the GPU against this restatement."""
import ctypes
import itertools

import numpy as np
import pytest

NEG_INF = -np.inf


def prune(v, n, cutoff_prob, log_input):
  """One frame's kept (classes, log p): by value descending, ties to the lower index; the first n; then the shortest
  prefix whose float64 cumulative probability reaches cutoff_prob (cutoff_prob < 1 only), at least one class."""
  v = np.asarray(v, dtype=np.float32)
  order = np.argsort(-v, kind="stable")[:min(n, len(v))]
  x = v[order].astype(np.float64)
  if cutoff_prob < 1.0:
    cum = np.cumsum(np.exp(x) if log_input else x)
    hit = np.nonzero(cum >= cutoff_prob)[0]
    if len(hit):
      order, x = order[:hit[0] + 1], x[:hit[0] + 1]
  with np.errstate(divide="ignore"):
    lp = x if log_input else np.log(x)
  return order, lp


def beam_ref(v, size, beam_width, cutoff_top_n, cutoff_prob=1.0, blank=0, log_input=False):
  """Prefix beam search over frames [0, size) of v (T, C).  Returns [(ids tuple, offsets tuple, -log P)], best
  first, ties by (parent rank, own continuation before extensions, class)."""
  beam = [((), 0.0, NEG_INF, ())]   # (prefix, log p_blank, log p_nonblank, offsets)
  for t in range(size):
    keep, lp = prune(v[t], cutoff_top_n, cutoff_prob, log_input)
    c2k = {int(c): k for k, c in enumerate(keep)}
    W = len(beam)
    pb = np.array([h[1] for h in beam])
    pnb = np.array([h[2] for h in beam])
    score = np.logaddexp(pb, pnb)
    last = np.array([h[0][-1] if h[0] else -1 for h in beam])
    # own continuations: blank, and a repeat of the last character
    own_pb = score + lp[c2k[blank]] if blank in c2k else np.full(W, NEG_INF)
    own_pnb = np.full(W, NEG_INF)
    for i in range(W):
      if last[i] in c2k:
        own_pnb[i] = pnb[i] + lp[c2k[int(last[i])]]
    # extensions (W, k)
    ext = np.where(keep[None, :] == last[:, None], pb[:, None], score[:, None]) + lp[None, :]
    ext[:, keep == blank] = NEG_INF
    # an extension already in the beam merges into it
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
    order = valid[np.lexsort((tb[valid], par[valid], -sc[valid]))][:beam_width]
    nxt = []
    for s in order:
      i = int(par[s])
      pre, _, _, off = beam[i]
      if s < W:
        nxt.append((pre, own_pb[i], own_pnb[i], off))
      else:
        c = int(keep[(s - W) % len(keep)])
        nxt.append((pre + (c,), NEG_INF, sc[s], off + (t,)))
    beam = nxt
  return [(h[0], h[3], -float(np.logaddexp(h[1], h[2]))) for h in beam]


def enumerate_labellings(v, log_input=False, blank=0):
  """Every labelling's probability: the sum over all C^T alignments that collapse to it (float64)."""
  p = np.exp(np.asarray(v, np.float64)) if log_input else np.asarray(v, np.float64)
  T, C = p.shape
  out = {}
  for a in itertools.product(range(C), repeat=T):
    lab, prev = [], None
    for c in a:
      if c != prev and c != blank:
        lab.append(c)
      prev = c
    pr = np.prod(p[np.arange(T), a])
    out[tuple(lab)] = out.get(tuple(lab), 0.0) + pr
  return sorted(((k, -np.log(P)) for k, P in out.items() if P > 0), key=lambda kv: kv[1])


def softmax_frames(rng, T, C, scale=1.5):
  x = rng.standard_normal((T, C)) * scale
  x = np.exp(x - x.max(1, keepdims=True))
  return (x / x.sum(1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("C,T,seed", [(2, 6, 0), (3, 5, 1), (3, 6, 2), (4, 4, 3), (4, 6, 4)])
@pytest.mark.parametrize("log_input", [False, True])
def test_restatement_matches_exhaustive_enumeration(C, T, seed, log_input):
  rng = np.random.default_rng(seed)
  p = softmax_frames(rng, T, C)
  v = np.log(p) if log_input else p
  want = enumerate_labellings(v, log_input)
  got = beam_ref(v, T, beam_width=len(want) + 5, cutoff_top_n=C, log_input=log_input)
  assert len(got) == len(want)
  for (ids, off, s), (lab, s_want) in zip(got, want):
    assert ids == lab
    assert abs(s - s_want) < 1e-9
    assert len(off) == len(ids) and list(off) == sorted(off)


def test_restatement_with_one_hypothesis_is_greedy():
  """beam_width 1, cutoff_top_n 1: argmax per frame (lower index on ties), collapse repeats, drop blanks; offsets are
  the first frame of each kept run."""
  rng = np.random.default_rng(5)
  for _ in range(20):
    T, C = 30, 6
    v = rng.integers(0, 3, (T, C)).astype(np.float32)   # frequent ties
    am = [int(np.argmax(r)) for r in v]
    ids, off = [], []
    for t, c in enumerate(am):
      if c != 0 and (t == 0 or am[t - 1] != c):
        ids.append(c)
        off.append(t)
    (got_ids, got_off, _), = beam_ref(v, T, 1, 1, log_input=True)
    assert list(got_ids) == ids and list(got_off) == off


def test_restatement_cutoff_prob_keeps_shortest_prefix():
  keep, lp = prune(np.array([0.1, 0.5, 0.3, 0.1], np.float32), 4, 0.8, False)
  assert list(keep) == [1, 2]
  keep, _ = prune(np.array([0.1, 0.5, 0.3, 0.1], np.float32), 4, 0.4, False)
  assert list(keep) == [1]
  keep, _ = prune(np.array([0.25, 0.25, 0.25, 0.25], np.float32), 3, 1.0, False)
  assert list(keep) == [0, 1, 2]


def test_lm_path_is_rejected():
  from lipreading_amd.decoder import BeamCTCDecoder
  with pytest.raises(NotImplementedError, match="KenLM"):
    BeamCTCDecoder(["_", "a", "b"], lm_path="lm.binary")
  # accepted and ignored, as ctcdecode does without a language model
  dec = BeamCTCDecoder(["_", "a", "b"], alpha=0.5, beta=1.0, num_processes=16)
  assert dec.beam_width == 100 and dec.cutoff_top_n == 40


def test_abi_rejects_bad_arguments_without_a_device():
  from lipreading_amd import _C
  lib = _C.lib()
  fake = ctypes.c_void_p(256)   # never dereferenced: every check below returns before any device call
  args = dict(probs=fake, sb=75 * 65, st=65, sizes=None, log_input=0, n=40, cp=1.0, W=100, blank=0, ids=fake,
              off=fake, lens=fake, scores=fake, ws=fake, wsb=1 << 40, B=32, T=75, C=65)

  def call(**kw):
    a = dict(args, **kw)
    return lib.lr_ctc_beam_decode(a["probs"], a["sb"], a["st"], a["sizes"], a["log_input"], a["n"], a["cp"], a["W"],
                                  a["blank"], a["ids"], a["off"], a["lens"], a["scores"], a["ws"], a["wsb"], a["B"],
                                  a["T"], a["C"], None)

  for name in ("probs", "ids", "off", "lens", "scores", "ws"):
    assert call(**{name: None}) == _C.LR_ERR_INVALID_ARG, name
  for kw in (dict(B=0), dict(T=0), dict(C=0), dict(W=0), dict(n=0), dict(blank=65), dict(blank=-1),
             dict(cp=float("nan"))):
    assert call(**kw) == _C.LR_ERR_INVALID_ARG, kw
  for kw in (dict(W=129), dict(n=65), dict(C=257)):
    assert call(**kw) == _C.LR_ERR_UNSUPPORTED, kw
  assert call(wsb=16) == _C.LR_ERR_WORKSPACE
  assert lib.lr_ctc_beam_workspace_bytes(32, 75, 65, 100, 40) > 0
  assert lib.lr_ctc_beam_workspace_bytes(0, 75, 65, 100, 40) == 0
  assert lib.lr_ctc_beam_workspace_bytes(32, 75, 65, 129, 40) == 0


def test_driver_decoder_flags():
  from lipreading_amd import driver
  f = driver.parse_flags([])
  assert f["ctc_decoder"] == "greedy" and f["beam_width"] == 100
  f = driver.parse_flags(["--ctc_decoder=beam", "--beam_width=8"])
  assert f["ctc_decoder"] == "beam" and f["beam_width"] == 8
  with pytest.raises(SystemExit):
    driver.parse_flags(["--ctc_decoder=prefix"])
