"""CPU: hotword biasing of the CTC prefix beam search.  beam_bias_ref (tests/beam_bias_cases.py), the float64
restatement of lr_ctc_beam_bias_decode's specification (lipreading_amd/csrc/lr_ctc_beam.hip), against exhaustive
enumeration; the readable cases; the packed automaton against a brute-force walk; the host-side rejections of the
packer, BeamCTCDecoder and the driver (no device needed).  tests/test_gpu_beam_bias.py holds the GPU against the
restatement."""
import ctypes
import warnings

import numpy as np
import pytest

from tests import beam_bias_cases as K
from tests.test_beam_cpu import beam_ref, softmax_frames
from tests.test_beam_lm_cpu import LABELS, TOY, Dict, load

OVERLAP = [((1, 2), 2.0), ((1, 2, 1), 3.5), ((2, 1, 2), 1.25)]   # ab, aba, bab over a = 1, b = 2


# ------------------------------------------------------------------------------------------------------------------
# the brute-force bonus, by hand
# ------------------------------------------------------------------------------------------------------------------
def test_bonus_by_hand():
  b = K.Bias(OVERLAP)
  y = (1, 2, 1, 2, 1)                        # ababa: ab x2, aba x2 (overlapping), bab x1
  assert b.bonus_end(y) == 2 * 2.0 + 2 * 3.5 + 1.25
  assert b.partial(y) == max(2.0 / 2, 3.5 / 3, 1.25 * 2 / 3)       # ends with a (ab, aba), ba (bab)
  assert b.partial((1, 2)) == max(3.5 * 2 / 3, 1.25 / 3)           # ab is complete: only aba[:2] and bab[:1] count
  assert b.bonus_run((1, 2)) == 2.0 + 3.5 * 2 / 3
  assert b.bonus_run(()) == 0.0
  # anchored on class 3: a phrase starts at 0 or right after a 3
  a = K.Bias([((1, 2), 2.0)], anchor=3)
  assert a.bonus_end((1, 2, 1, 2)) == 2.0 and a.bonus_end((1, 2, 3, 1, 2)) == 4.0
  assert a.partial((2, 1)) == 0.0 and a.partial((2, 3, 1)) == 1.0 and a.partial((1,)) == 1.0


# ------------------------------------------------------------------------------------------------------------------
# the restatement against exhaustive enumeration
# ------------------------------------------------------------------------------------------------------------------
def check_against_enumeration(got, want):
  assert len(got) == len(want)
  assert {g[0] for g in got} == {w[0] for w in want}
  ref = dict(want)
  for r, (ids, off, s) in enumerate(got):
    assert abs(s - ref[ids]) < 1e-9, (ids, s, ref[ids])
    assert len(off) == len(ids) and list(off) == sorted(off)
    sep = all(abs(want[r][1] - want[q][1]) > 1e-9 for q in (r - 1, r + 1) if 0 <= q < len(want))
    if sep:
      assert ids == want[r][0]


@pytest.mark.parametrize("C,T,seed,phrases,anchor", [
    (3, 6, 0, OVERLAP, -1),                                           # fail links, overlaps, the best partial
    (3, 5, 1, [((2,), 0.75), ((1, 1), 4.0)], -1),
    (4, 5, 2, [((2, 3), 2.0), ((3,), 0.5), ((2, 1, 3), 6.0)], 1),     # anchored on class 1; a phrase with the anchor
    (4, 6, 3, [((2, 3), 2.0), ((3,), 0.5), ((2, 1, 3), 6.0)], -1),    # the same phrases anywhere
    (4, 4, 4, [((3, 3), 1.5), ((3, 3), 2.5)], 1),                     # a phrase listed twice
])
@pytest.mark.parametrize("log_input", [False, True])
def test_restatement_matches_exhaustive_enumeration(C, T, seed, phrases, anchor, log_input):
  p = softmax_frames(np.random.default_rng(seed), T, C)
  v = np.log(p) if log_input else p
  bias = K.Bias(phrases, anchor)
  want = K.enumerate_bias(v, bias, log_input)
  got = K.beam_bias_ref(v, T, len(want) + 5, C, bias, log_input=log_input)
  check_against_enumeration(got, want)
  # the data exercise the feature: the bonus reorders the enumeration
  assert [w[0] for w in want] != [w[0] for w in K.enumerate_labellings(v, log_input)]


@pytest.fixture
def toy(tmp_path):
  p = tmp_path / "toy.arpa"
  p.write_text(TOY)
  return str(p)


@pytest.mark.parametrize("alpha,beta", [(0.5, 1.0), (2.0, -0.5)])
def test_restatement_with_the_toy_language_model(toy, alpha, beta):
  labels = LABELS[:4]                                   # _, ' ', a, b
  lm = load(toy)
  dic = Dict(lm, labels)
  T = 5
  p = softmax_frames(np.random.default_rng(7), T, len(labels))
  bias = K.Bias([((2, 3), 3.0), ((3, 3, 1, 2), 5.0), ((3, 2), 4.0)], anchor=1)   # ab, "bb a", ba (no vocabulary prefix)
  want = K.enumerate_bias(p, bias, labels=labels, lm=lm, dic=dic, alpha=alpha, beta=beta)
  got = K.beam_bias_ref(p, T, len(want) + 5, len(labels), bias, lm=lm, dic=dic, alpha=alpha, beta=beta)
  check_against_enumeration(got, want)
  assert not any(lab[:2] == (3, 2) for lab, _ in want)   # the dictionary still holds: "ba" is unreachable


# ------------------------------------------------------------------------------------------------------------------
# the readable cases
# ------------------------------------------------------------------------------------------------------------------
def text_of(ids):
  return "".join(K.TRAP_LABELS[c] for c in ids)


def test_homophene_trap():
  """The frames put "ban" ahead; told to expect "pan", the search returns it."""
  p = K.homophene_frames()
  C = len(K.TRAP_LABELS)
  plain = beam_ref(p, len(p), 8, C)
  assert text_of(plain[0][0]) == "ban"
  bias = K.Bias([(K.spell_ids("pan"), 10.0)], anchor=1)
  got = K.beam_bias_ref(p, len(p), 8, C, bias)
  assert text_of(got[0][0]) == "pan"
  strings = {text_of(g[0]): g[2] for g in got}
  masses = {text_of(g[0]): g[2] for g in plain}
  # the whole weight, once (the two beams prune differently: the masses agree to a few 1e-3)
  assert abs(strings["pan"] - (masses["pan"] - 10.0)) < 0.01


def test_partial_credit_keeps_the_prefix_in_a_narrow_beam():
  """beam_width 2: without partial credit 'p' is pruned at the first frame and "pan" can never complete."""
  p = K.pruned_prefix_frames()
  C = len(K.TRAP_LABELS)
  phrases = [(K.spell_ids("pan"), 10.0)]
  without = K.beam_bias_ref(p, len(p), 2, C, K.Bias(phrases, anchor=1, partial_credit=False))
  with_ = K.beam_bias_ref(p, len(p), 2, C, K.Bias(phrases, anchor=1))
  assert text_of(without[0][0]) == "ban" and "pan" not in [text_of(g[0]) for g in without]
  assert text_of(with_[0][0]) == "pan"
  # and the credit is gone at the end: the score is the mass plus the whole weight, once
  wide = dict((text_of(i), s) for i, _, s in beam_ref(p, len(p), 64, C))
  assert abs(with_[0][2] - (wide["pan"] - 10.0)) < 0.01


def test_anchor_on_channel():
  p = K.channel_frames()
  C = len(K.TRAP_LABELS)
  phrases = [(K.spell_ids("ann"), 10.0)]
  assert text_of(beam_ref(p, len(p), 8, C)[0][0]) == "chanmel"
  assert text_of(K.beam_bias_ref(p, len(p), 8, C, K.Bias(phrases, anchor=-1))[0][0]) == "channel"
  assert text_of(K.beam_bias_ref(p, len(p), 8, C, K.Bias(phrases, anchor=1))[0][0]) == "chanmel"


# ------------------------------------------------------------------------------------------------------------------
# the packer
# ------------------------------------------------------------------------------------------------------------------
def _pack(phrases, anchor, C, weights=None, nbytes=None):
  """-> (status, bytes the size call returned, blob) through the ABI, no device."""
  from lipreading_amd import _C
  lib = _C.lib()
  off = np.zeros(len(phrases) + 1, np.int64)
  off[1:] = np.cumsum([len(q) for q, _ in phrases])
  cls = np.asarray([c for q, _ in phrases for c in q] + [0], np.int32)
  w = np.asarray([x for _, x in phrases] if weights is None else weights, np.float32)
  vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
  need = lib.lr_ctc_beam_bias_pack_bytes(len(phrases), vp(off), vp(cls), anchor, C)
  out = np.zeros(max(need, 1 << 12), np.uint8)
  st = lib.lr_ctc_beam_bias_pack(vp(out), out.size if nbytes is None else nbytes, len(phrases), vp(off), vp(cls),
                                 vp(w), anchor, C)
  return st, need, out


def _tables(blob):
  head = blob[:64]
  nodes, stride, start = (int(x) for x in head[8:20].view(np.int32))
  next_off, out_off, part_off, nbytes = (int(x) for x in head[32:64].view(np.int64))
  nxt = blob[next_off:next_off + nodes * stride * 4].view(np.int32).reshape(nodes, stride)
  return nxt, blob[out_off:out_off + nodes * 4].view(np.float32), blob[part_off:part_off + nodes * 4].view(
      np.float32), start, nbytes


@pytest.mark.parametrize("anchor", [-1, 0])
def test_packed_automaton_against_a_brute_force_walk(anchor):
  """Every state is the longest suffix of the text that is a prefix of a pattern; walk all of them from the start."""
  from lipreading_amd import _C
  C = 3
  phrases = OVERLAP + [((2, 0, 1), 0.5)] if anchor >= 0 else OVERLAP
  st, need, blob = _pack(phrases, anchor, C)
  assert st == _C.LR_OK
  nxt, out, part, start, nbytes = _tables(blob)
  assert nbytes == need
  pre = (anchor,) if anchor >= 0 else ()
  pats = [(pre + tuple(q), w, len(q)) for q, w in phrases]
  prefixes = {p[:j] for p, _, _ in pats for j in range(len(p) + 1)}
  assert len(prefixes) == nxt.shape[0]

  def state_of(text):
    return next(text[i:] for i in range(len(text) + 1) if text[i:] in prefixes)

  ids = {(): 0, pre: start}
  todo = [(), pre] if pre else [()]
  while todo:
    s = todo.pop()
    u = ids[s]
    want_out = sum(w for p, w, _ in pats if len(p) <= len(s) and s[len(s) - len(p):] == p)
    want_part = max([w * (j - len(pre)) / m for p, w, m in pats for j in range(len(pre) + 1, len(p))
                     if j <= len(s) and s[len(s) - j:] == p[:j]] + [0.0])
    assert out[u] == np.float32(want_out), s
    assert part[u] == np.float32(want_part), s
    for c in range(C):
      t = state_of(s + (c,))
      if t not in ids:
        ids[t] = int(nxt[u, c])
        todo.append(t)
      assert ids[t] == int(nxt[u, c]), (s, c)
  assert len(ids) == len(prefixes) and len(set(ids.values())) == len(ids)


def test_packer_limits_and_rejections():
  from lipreading_amd import _C
  ok = [((1, 2), 1.0)]
  assert _pack(ok, -1, 3)[0] == _C.LR_OK
  assert _pack(ok, -1, 3, nbytes=16)[0] == _C.LR_ERR_WORKSPACE
  # 4096 nodes fit, 4097 do not: one phrase of m characters is m + 1 nodes, m + 2 with an anchor
  assert _pack([((1,) * 4095, 1.0)], -1, 3)[0] == _C.LR_OK
  st, need, _ = _pack([((1,) * 4096, 1.0)], -1, 3)
  assert st == _C.LR_ERR_UNSUPPORTED and need == 0
  assert _pack([((1,) * 4094, 1.0)], 2, 3)[0] == _C.LR_OK
  assert _pack([((1,) * 4095, 1.0)], 2, 3)[0] == _C.LR_ERR_UNSUPPORTED
  assert _pack([((1 + k % 2, 1 + k // 2 % 2, 1), 1.0) for k in range(1024)], -1, 3)[0] == _C.LR_OK
  assert _pack([((1,), 1.0)] * 1025, -1, 3)[0] == _C.LR_ERR_UNSUPPORTED
  assert _pack(ok, -1, 257)[0] == _C.LR_ERR_UNSUPPORTED
  for bad in ([((1, 2), 1.0), ((), 1.0)], [((1, 3), 1.0)], [((-1,), 1.0)]):
    st, need, _ = _pack(bad, -1, 3)
    assert st == _C.LR_ERR_INVALID_ARG and need == 0, bad
  for w in (0.0, -1.0, float("nan"), float("inf")):
    assert _pack(ok, -1, 3, weights=[w])[0] == _C.LR_ERR_INVALID_ARG, w
  assert _pack(ok, 3, 3)[0] == _C.LR_ERR_INVALID_ARG and _pack(ok, -2, 3)[0] == _C.LR_ERR_INVALID_ARG
  assert _pack([], -1, 3)[0] == _C.LR_ERR_INVALID_ARG


def test_abi_rejects_bad_arguments_without_a_device():
  from lipreading_amd import _C
  lib = _C.lib()
  fake = ctypes.c_void_p(256)   # never dereferenced: every check below returns before any device call
  args = dict(probs=fake, sb=75 * 65, st=65, sizes=None, log_input=0, n=40, cp=1.0, W=100, blank=0, lm=fake,
              roles=fake, alpha=0.5, beta=1.0, bias=fake, ids=fake, off=fake, lens=fake, scores=fake, ws=fake,
              wsb=1 << 40, B=32, T=75, C=65)

  def plain(**kw):
    a = dict(args, **kw)
    return lib.lr_ctc_beam_bias_decode(a["probs"], a["sb"], a["st"], a["sizes"], a["log_input"], a["n"], a["cp"],
                                       a["W"], a["blank"], a["bias"], a["ids"], a["off"], a["lens"], a["scores"],
                                       a["ws"], a["wsb"], a["B"], a["T"], a["C"], None)

  def with_lm(**kw):
    a = dict(args, **kw)
    return lib.lr_ctc_beam_lm_bias_decode(a["probs"], a["sb"], a["st"], a["sizes"], a["log_input"], a["n"], a["cp"],
                                          a["W"], a["blank"], a["lm"], a["roles"], a["alpha"], a["beta"], a["bias"],
                                          a["ids"], a["off"], a["lens"], a["scores"], a["ws"], a["wsb"], a["B"],
                                          a["T"], a["C"], None)

  for call, names in ((plain, ("probs", "bias", "ids", "off", "lens", "scores", "ws")),
                      (with_lm, ("probs", "lm", "roles", "bias", "ids", "off", "lens", "scores", "ws"))):
    for name in names:
      assert call(**{name: None}) == _C.LR_ERR_INVALID_ARG, name
    for kw in (dict(B=0), dict(T=0), dict(C=0), dict(W=0), dict(n=0), dict(blank=65), dict(cp=float("nan"))):
      assert call(**kw) == _C.LR_ERR_INVALID_ARG, kw
    for kw in (dict(W=129), dict(n=65), dict(C=257)):
      assert call(**kw) == _C.LR_ERR_UNSUPPORTED, kw
    assert call(wsb=16) == _C.LR_ERR_WORKSPACE
  assert with_lm(alpha=float("nan")) == _C.LR_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------------------
# BeamCTCDecoder and the driver
# ------------------------------------------------------------------------------------------------------------------
def test_constructor(toy):
  from lipreading_amd import _C
  from lipreading_amd.decoder import BeamCTCDecoder
  labels = ["_", " ", "a", "b", "<EOS>"]
  for none in (None, []):
    assert BeamCTCDecoder(labels, hotwords=none)._hotwords is None
  dec = BeamCTCDecoder(labels, hotwords=["ab", ("b a", 2.5)], hotword_weight=4.0)
  assert dec._hotwords.phrases == [("ab", 4.0), ("b a", 2.5)]
  assert dec._hotwords.ids == [[2, 3], [3, 1, 2]] and dec._hotwords.anchor == 1
  assert BeamCTCDecoder(labels, hotwords=["ab"], hotword_anchor=False)._hotwords.anchor == -1
  with pytest.raises(ValueError, match="no label spells 'c'"):
    BeamCTCDecoder(labels, hotwords=["abc"])
  with pytest.raises(ValueError, match="no label spells '_'"):      # the blank's label is no character
    BeamCTCDecoder(labels, hotwords=["a_b"])
  with pytest.raises(ValueError, match="hotword_anchor=False"):
    BeamCTCDecoder(["_", "a", "b"], hotwords=["ab"])
  assert BeamCTCDecoder(["_", "a", "b"], hotwords=["ab"], hotword_anchor=False)._hotwords.ids == [[1, 2]]
  with pytest.raises(ValueError, match="non-empty"):
    BeamCTCDecoder(labels, hotwords=["ab", ""])
  for w in (0.0, -2.0, float("nan"), float("inf")):
    with pytest.raises(ValueError, match="finite and > 0"):
      BeamCTCDecoder(labels, hotwords=[("ab", w)])
    with pytest.raises(ValueError, match="finite and > 0"):
      BeamCTCDecoder(labels, hotwords=["ab"], hotword_weight=w)
  with pytest.raises(_C.LipReadingHipError, match="lr_ctc_beam_bias_pack"):
    BeamCTCDecoder(labels, hotwords=["a" * 5000])
  # with a language model: one warning that names the phrases its dictionary keeps out
  with pytest.warns(UserWarning, match="'ba', 'a bab'") as rec:
    BeamCTCDecoder(labels, lm_path=toy, hotwords=["ab", "ba", "bb a", "a bab"])
  assert len(rec) == 1 and "'ab'" not in str(rec[0].message) and "'bb a'" not in str(rec[0].message)
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    BeamCTCDecoder(labels, lm_path=toy, hotwords=["ab", "bb a"])


def test_driver_hotword_flags():
  from lipreading_amd import driver
  f = driver.parse_flags([])
  assert f["hotwords"] == "" and f["hotword_weight"] == 10.0
  f = driver.parse_flags(["--ctc_decoder=beam", "--hotwords=pan,channel", "--hotword_weight=6.5"])
  assert f["hotwords"] == "pan,channel" and f["hotword_weight"] == 6.5
  for argv in (["--hotwords=pan"], ["--hotword_weight=3"], ["--ctc_decoder=greedy", "--hotwords=pan"]):
    with pytest.raises(SystemExit):
      driver.parse_flags(argv)
