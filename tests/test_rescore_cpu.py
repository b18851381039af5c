"""CPU: the rule of attention rescoring (lipreading_amd/csrc/lr_attn_rescore.hip) as restated in
tests/rescore_cases.py — its properties on small random decoders —, the driver's flags and routing, and the
rejections of CharDecodingStep.rescore and of the C ABI that need no device.  The GPU is checked against the same
restatement in tests/test_gpu_rescore.py."""
import math

import numpy as np
import pytest
import torch

from tests.rescore_cases import EMPTY, SCORABLE, UNSCORABLE, combined, random_lists, rescore_ref, scored_sequence
from tests.test_attn_beam_cpu import BOS, EOS, PAD, UNK, beam_ref, complete_hypotheses, rescore, small_case

INF = float("inf")


def lists(rows, W):
  """[[classes]] per utterance -> (ids [B][N][W] padded with -1, lens)."""
  ids = [[list(r) + [-1] * (W - len(r)) for r in utt] for utt in rows]
  return ids, [[len(r) for r in utt] for utt in rows]


def classes(tokens):
  return [v + 1 for v in tokens]


@pytest.mark.parametrize("rnn_type,attn", [("GRU", "dot"), ("LSTM", "concat"), ("RNN", "none")])
def test_weight_one_is_the_identity(rnn_type, attn):
  dec, enc, lens, prev = small_case(rnn_type, attn, seed=4)
  rows = [[classes(h) for h in ([4, 3, EOS], [3], [], [4, 4, 4], [EOS])]] * 2
  ids, hl = lists(rows, 3)
  first = [[0.5, 1.25, 1.25, 7.0, 9.5]] * 2   # ascending as the CTC searches leave it, two equal
  ref = rescore_ref(dec, enc, lens, prev, ids, hl, first, 1.0, 0.0)
  for b in range(2):
    assert ref[b]["order"] == [0, 1, 2, 3, 4]
    assert ref[b]["s"] == [-f for f in first[b]]
    assert all(math.isfinite(a) and a < 0 for a in ref[b]["a"])


@pytest.mark.parametrize("rnn_type,attn,Lmax", [("GRU", "dot", 2), ("LSTM", "none", 2), ("RNN", "concat", 2),
                                                ("GRU", "general", 3)])
def test_weight_zero_on_every_complete_hypothesis_is_the_full_beam(rnn_type, attn, Lmax):
  """Every complete hypothesis of the V = 5 decoder goes in as one list.  Those that end with EOS are scored as they
  are: among them the order and the scores are beam_ref's at K = all.  (A hypothesis the beam search capped at
  Lmax + 1 tokens without EOS gets one appended by the rule, so its rescoring score is not the beam's: those are
  passed too, but compared with their own float64 score.)"""
  dec, enc, lens, prev = small_case(rnn_type, attn, seed=3, scale=3.0)
  hyps = complete_hypotheses(5, Lmax)
  rows = [[classes(h) for h in hyps]] * enc.shape[0]
  ids, hl = lists(rows, Lmax + 1)
  first = [[float(i) for i in range(len(hyps))]] * enc.shape[0]
  ref = rescore_ref(dec, enc, lens, prev, ids, hl, first, 0.0, 0.0)
  beams = beam_ref(dec, enc, lens, prev, len(hyps), Lmax)
  for b in range(enc.shape[0]):
    want = [(h, s) for h, s in beams[b][0] if h[-1] == EOS]
    got = [(hyps[n], s) for n, s in zip(ref[b]["order"], ref[b]["s"]) if hyps[n][-1] == EOS]
    assert [h for h, _ in got] == [h for h, _ in want]
    np.testing.assert_allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-9)
    for n, s in zip(ref[b]["order"], ref[b]["s"]):
      if hyps[n][-1] != EOS:
        assert abs(s - rescore(dec, enc, lens, prev, b, hyps[n] + [EOS])) < 1e-12
    assert ref[b]["s"] == sorted(ref[b]["s"], reverse=True)


def test_eos_rules():
  V = 5
  assert scored_sequence(classes([4, EOS, 3, PAD]), 4, 1.0, V) == (SCORABLE, [4, EOS])     # EOS in the middle
  assert scored_sequence(classes([4, 3, EOS]), 3, 1.0, V) == (SCORABLE, [4, 3, EOS])       # EOS at the end
  assert scored_sequence(classes([4, 3, 3]), 3, 1.0, V) == (SCORABLE, [4, 3, 3, EOS])      # no EOS: one is appended
  assert scored_sequence([-1, -1, -1], 0, 1.0, V) == (SCORABLE, [EOS])                     # the empty transcript
  assert scored_sequence(classes([4, 3, EOS]), 2, 1.0, V) == (SCORABLE, [4, 3, EOS])       # ids past len are not read
  assert scored_sequence(classes([EOS, 0, 0]), 3, 1.0, V) == (SCORABLE, [EOS])             # nothing after EOS counts
  dec, enc, lens, prev = small_case("GRU", "dot", seed=9)
  rows = [[classes([4, EOS, 3]), classes([4, EOS]), classes([4]), classes([4, EOS, PAD])]] * 2
  ids, hl = lists(rows, 3)
  ref = rescore_ref(dec, enc, lens, prev, ids, hl, [[1.0, 2.0, 3.0, 4.0]] * 2, 0.0, 0.0)
  for b in range(2):
    a = rescore(dec, enc, lens, prev, b, [4, EOS])
    assert ref[b]["a_slot"] == [a, a, a, a] and ref[b]["order"] == [0, 1, 2, 3]


def test_unscorable_slots_follow_the_scorable_ones_and_empty_slots_come_last():
  dec, enc, lens, prev = small_case("LSTM", "dot", seed=5)
  V = dec.vocab_size
  rows = [[classes([4, PAD, EOS]),        # 0 PAD
           [],                            # 1 empty (+inf)
           classes([3, EOS]),             # 2 scorable
           classes([BOS, 4]),             # 3 BOS
           [0, 5],                        # 4 blank
           classes([4, V]),               # 5 out of range
           classes([4, 4]),               # 6 scorable
           classes([4]),                  # 7 empty by NaN
           classes([4, EOS, PAD])]] * 2   # 8 scorable: the PAD stands after the EOS
  ids, hl = lists(rows, 3)
  first = [[0.1, INF, 0.3, 0.4, 0.5, 0.6, 0.7, float("nan"), 0.9]] * 2
  for lam, gamma in ((0.0, 0.0), (0.3, 0.5), (1.0, 0.0)):
    ref = rescore_ref(dec, enc, lens, prev, ids, hl, first, lam, gamma)
    for b in range(2):
      r = ref[b]
      assert r["cls"] == [UNSCORABLE, EMPTY, SCORABLE, UNSCORABLE, UNSCORABLE, UNSCORABLE, SCORABLE, EMPTY, SCORABLE]
      assert sorted(r["order"][:3]) == [2, 6, 8] and r["order"][3:] == [0, 3, 4, 5, 1, 7]
      assert all(math.isfinite(x) for x in r["s"][:3] + r["a"][:3])
      assert r["s"][3:] == [-INF] * 6 and r["a"][3:] == [-INF] * 6
      assert r["s"][:3] == sorted(r["s"][:3], reverse=True)


def test_exact_ties_keep_first_pass_order():
  dec, enc, lens, prev = small_case("GRU", "none", seed=6)
  same = classes([4, 3, EOS])
  rows = [[classes([3, EOS]), same, same + [9], same, classes([4, 3])]] * 2   # slot 2: junk after the EOS
  ids, hl = lists(rows, 4)
  first = [[3.0, 2.0, 2.0, 2.0, 2.0]] * 2
  ref = rescore_ref(dec, enc, lens, prev, ids, hl, first, 0.4, 0.25)
  for b in range(2):
    r = ref[b]
    assert r["s_slot"][1] == r["s_slot"][2] == r["s_slot"][3]
    at = [r["order"].index(n) for n in (1, 2, 3)]
    assert at == sorted(at) and at[2] - at[0] == 2


def test_length_bonus_moves_a_longer_hypothesis_ahead():
  dec, enc, lens, prev = small_case("LSTM", "1_layer_nn", seed=8)
  short, longer = [4, EOS], [4, 3, 3, 4, EOS]
  rows = [[classes(short), classes(longer)]] * 2
  ids, hl = lists(rows, 5)
  first = [[1.0, 1.0]] * 2
  lam = 0.3
  for b in range(2):
    a0, a1 = (rescore(dec, enc, lens, prev, b, q) for q in (short, longer))
    assert a0 > a1   # five log-probabilities sum below two (V = 5: each is below zero)
    # s1 > s0  <=>  gamma (|q1| - |q0|) > (1 - lam)(a0 - a1): the value where the order turns
    turn = (1 - lam) * (a0 - a1) / (len(longer) - len(short))
    assert rescore_ref(dec, enc, lens, prev, ids, hl, first, lam, 0.0)[b]["order"] == [0, 1]
    assert rescore_ref(dec, enc, lens, prev, ids, hl, first, lam, 0.9 * turn)[b]["order"] == [0, 1]
    r = rescore_ref(dec, enc, lens, prev, ids, hl, first, lam, 1.1 * turn)[b]
    assert r["order"] == [1, 0]
    assert r["s"][0] == combined(a1, 1.0, len(longer), lam, 1.1 * turn)


def test_random_lists_hold_every_kind():
  ids, lens, first = random_lists(5, 10, 12, 64, seed=1)
  assert ids.shape == (5, 13, 17) and ids.dtype == torch.int32
  for b in range(5):
    seen = set()
    for n in range(10):
      c, q = scored_sequence(ids[b, n].tolist(), int(lens[b, n]), float(first[b, n]), 64)
      row = ids[b, n, :int(lens[b, n])].tolist()
      assert (ids[b, n, int(lens[b, n]):] == -1).all()
      if c == EMPTY:
        seen.add("empty")
      elif lens[b, n] == 0:
        seen.add("len0")
      elif c == UNSCORABLE:
        seen.add("blank" if -1 in q else "pad")   # class 0 is token -1; PAD is token 0
      elif EOS + 1 not in row:
        seen.add("no_eos")
      elif row.index(EOS + 1) < len(row) - 1:
        seen.add("eos_mid")
    assert {"empty", "len0", "pad", "blank", "no_eos", "eos_mid"} <= seen, (b, seen)


# ---- driver ---------------------------------------------------------------------------------------------------------
RESCORE = ["--attn_decode=rescore", "--enable_ctc=True", "--ctc_decoder=beam"]


def test_driver_rescore_flags_parse_and_reject():
  from lipreading_amd import driver
  f = driver.parse_flags([])
  assert (f["attn_rescore_nbest"], f["attn_length_bonus"]) == (10, 0.0)
  f = driver.parse_flags(RESCORE + ["--attn_rescore_nbest=4", "--attn_length_bonus=0.5", "--attn_ctc_weight=0.7",
                                    "--beam_width=16"])
  assert (f["attn_decode"], f["attn_rescore_nbest"], f["attn_length_bonus"], f["attn_ctc_weight"]) == \
      ("rescore", 4, 0.5, 0.7)
  f = driver.parse_flags(RESCORE + ["--stream_chunk=5", "--stream_encoder=True", "--bidirectional=False"])
  assert f["stream_encoder"] and f["attn_decode"] == "rescore"
  driver.parse_flags(RESCORE + ["--lm_path=some.arpa", "--hotwords=hello"])   # the first pass's, as today
  for bad, name in ((["--attn_decode=rescore", "--ctc_decoder=beam"], "enable_ctc"),
                    (["--attn_decode=rescore", "--enable_ctc=True"], "ctc_decoder"),
                    (RESCORE + ["--ctc_only=True"], "ctc_only"),
                    (RESCORE + ["--attn_rescore_nbest=0"], "attn_rescore_nbest"),
                    (RESCORE + ["--attn_rescore_nbest=129", "--beam_width=200"], "attn_rescore_nbest"),
                    (RESCORE + ["--attn_rescore_nbest=9", "--beam_width=8"], "attn_rescore_nbest"),
                    (RESCORE + ["--attn_length_bonus=nan"], "attn_length_bonus"),
                    (RESCORE + ["--attn_length_bonus=inf"], "attn_length_bonus"),
                    (RESCORE + ["--attn_ctc_weight=1.5"], "attn_ctc_weight")):
    with pytest.raises(SystemExit) as e:
      driver.parse_flags(bad)
    assert name in str(e.value), (bad, e.value)
  for bad in ("--attn_decode=sample", "--attn_decode=two_pass"):
    with pytest.raises(SystemExit):
      driver.parse_flags([bad])
  driver.parse_flags(["--ctc_decoder=beam", "--beam_width=4", "--ctc_only=True", "--enable_ctc=True"])   # untouched


def test_driver_rescore_refuses_the_other_sessions():
  from lipreading_amd import driver
  f = dict(driver.DEFAULTS, attn_decode="rescore", enable_ctc=True, ctc_decoder="beam", stream_chunk=5)
  driver.attn_rescore_check(f)
  for name, value in (("stream_lookahead", 2), ("stream_tfm", True), ("stream_frontend", True)):
    with pytest.raises(SystemExit) as e:
      driver.attn_rescore_check(dict(f, **{name: value}))
    assert name in str(e.value)
  for flags in (RESCORE + ["--stream_chunk=5", "--stream_lookahead=2", "--bidirectional=True"],
                RESCORE + ["--stream_chunk=5", "--stream_tfm=True", "--encoder=transformer", "--tfm_chunk=4"],
                RESCORE + ["--stream_chunk=5", "--stream_frontend=True", "--frontend=conv3d", "--stream_encoder=True",
                           "--bidirectional=False"]):
    with pytest.raises(SystemExit):
      driver.parse_flags(flags)


def test_driver_error_of_routes_rescore(monkeypatch):
  from lipreading_amd import driver, train
  calls = []
  monkeypatch.setattr(train, "rescored_cer", lambda *a, **k: (calls.append(("host", a[5], k)), 0.125)[1])
  monkeypatch.setattr(train, "device_scores", lambda *a, **k: (calls.append(("device", k)), {"cer": 0.375})[1])
  monkeypatch.setattr(train, "attention_cer", lambda *a, **k: (calls.append("beam"), 0.25)[1])
  monkeypatch.setattr(train, "eval", lambda *a, **k: (calls.append("eval"), (0.0, 3, 4, 0.0))[1])
  dec, ctc = object(), object()
  flags = RESCORE + ["--attn_rescore_nbest=4", "--attn_ctc_weight=0.7", "--attn_length_bonus=0.5"]
  err = driver.make_error_of(driver.parse_flags(flags), None, dec, ctc, "cpu", {})
  assert err([]) == 0.125
  assert calls == [("host", ctc, dict(nbest=4, ctc_weight=0.7, length_bonus=0.5))]
  calls.clear()
  err = driver.make_error_of(driver.parse_flags(flags + ["--score=device"]), None, dec, ctc, "cpu", {})
  assert err([]) == 0.375 and err.last_scores == {"cer": 0.375}
  assert calls == [("device", dict(decoder=ctc, decoding_step=dec, rescore_nbest=4, ctc_weight=0.7, length_bonus=0.5))]
  calls.clear()
  err = driver.make_error_of(driver.parse_flags([]), None, dec, None, "cpu", {})   # the default is untouched
  assert err([]) == pytest.approx(0.25) and calls == ["eval"]


# ---- rejections, without a device ----------------------------------------------------------------------------------
def _step(rnn_type="GRU", layers=1):
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  enc = VideoEncoder(204, 16, rnn_type=rnn_type, num_layers=layers, bidirectional=False)
  return CharDecodingStep(enc, char_dim=8, vocab_size=64, char2idx=default_char2idx(), attention_type="dot")


def test_rescore_raises_before_any_launch():
  dec = _step()
  h = torch.zeros(2, 5, 16)
  lens = torch.tensor([5, 4])
  prev = torch.zeros(1, 2, 16)
  ids = torch.zeros(2, 3, 4, dtype=torch.int32)
  hl = torch.zeros(2, 3, dtype=torch.int32)
  f = torch.zeros(2, 3)
  with pytest.raises(ValueError, match="GPU"):
    dec.rescore(h, lens, prev, ids, hl, f)          # CPU tensors
  for kw in (dict(ctc_weight=-0.1), dict(ctc_weight=1.5), dict(ctc_weight=float("nan")), dict(ctc_weight="0.5"),
             dict(ctc_weight=True), dict(length_bonus=float("nan")), dict(length_bonus=float("inf")),
             dict(length_bonus=None)):
    with pytest.raises(ValueError, match="ctc_weight|length_bonus"):
      dec.rescore(h, lens, prev, ids, hl, f, **kw)
  bad = [dict(hyp_ids=torch.zeros(2, 129, 4, dtype=torch.int32), hyp_lens=torch.zeros(2, 129, dtype=torch.int32),
              first_scores=torch.zeros(2, 129)),                                           # N > 128
         dict(hyp_ids=torch.zeros(2, 3, 1025, dtype=torch.int32)),                         # W > 1024
         dict(hyp_ids=ids[0]), dict(hyp_ids=ids[:1]), dict(hyp_ids=ids.long()),            # rank, batch, dtype
         dict(hyp_ids=torch.zeros(2, 0, 4, dtype=torch.int32)),
         dict(hyp_lens=hl[:, :2]), dict(first_scores=f[:, :2]), dict(first_scores=f.tolist()),
         dict(encoder_hidden_states=h[0]), dict(previous_state=torch.zeros(2, 2, 16)),
         dict(previous_state=(prev, prev)), dict(encoder_lens=torch.tensor([5, 4, 3]))]
  for kw in bad:
    args = dict(encoder_hidden_states=h, encoder_lens=lens, previous_state=prev, hyp_ids=ids, hyp_lens=hl,
                first_scores=f)
    args.update(kw)
    with pytest.raises(ValueError) as e:
      dec.rescore(**args)
    assert "GPU" not in str(e.value), kw
  with pytest.raises(ValueError, match="\\(h, c\\)"):
    _step("LSTM").rescore(h, lens, prev, ids, hl, f)


def test_workspace_query_rejects_bad_sizes():
  from lipreading_amd import _C
  q = _C.lib().lr_decoder_rescore_workspace_bytes
  ok = (1, 3, 1, 4, 10, 40, 75, 64, 32, 64, 0)   # LSTM, 1_layer_nn, 1 layer, B=4, N=10, W=40, T=75, Hd=64, Cd=32, V=64
  assert q(*ok) > 0
  for i, bad in [(4, 0), (4, 129), (4, -1), (5, 0), (5, 1025), (9, 1025), (9, 2), (3, 0), (3, 6554), (2, 0), (2, 9),
                 (7, 6), (7, 0), (6, 0), (8, 0), (0, 3), (1, 5), (1, -1)]:
    args = list(ok)
    args[i] = bad
    assert q(*args) == 0, (i, bad)
  assert q(1, 3, 1, 4, 128, 1024, 75, 64, 32, 1024, 0) > 0   # the limits themselves
  assert q(1, 3, 1, 511, 128, 1, 75, 64, 32, 64, 0) > 0       # B*N = 65408
  assert q(1, 3, 1, 512, 128, 1, 75, 64, 32, 64, 0) == 0      # B*N = 65536
  assert q(1, 3, 1, 511, 128, 1024, 75, 64, 32, 64, 0) == 0   # more (row, step) pairs than the products address
  assert q(1, 4, 1, 4, 10, 40, 75, 64, 32, 64, 0) == 0        # concat without an attention size
  assert q(1, 4, 1, 4, 10, 40, 75, 64, 32, 64, 16) > 0
  for mode in (0, 1, 2):
    for attn in range(5):
      for layers in (1, _C.LR_DEC_MAX_LAYERS):
        assert q(mode, attn, layers, 4, 10, 40, 75, 64, 32, 64, 16) > 0


def test_rescore_entry_rejects_without_a_device():
  import ctypes
  from lipreading_amd import _C
  L_ = _C.lib()
  nn_ = ctypes.c_void_p(64)   # a non-NULL pointer the entry must never reach a launch with

  def call(N=10, W=40, V=64, lam=0.5, gamma=0.0, params=None, ptr=None):
    return L_.lr_decoder_rescore(1, 3, params, None, ptr, ptr, ptr, ptr, ptr, 40, 1, ptr, ptr, 1, 2, 0, lam, gamma,
                                 ptr, ptr, ptr, ptr, 0, 4, N, W, 75, 64, 32, V, 0, None)
  assert call(N=0) == _C.LR_ERR_INVALID_ARG            # nonsense: invalid
  assert call(N=129) == _C.LR_ERR_UNSUPPORTED          # well-formed, beyond the kernels: unsupported
  assert call(W=1025) == _C.LR_ERR_UNSUPPORTED
  assert call(V=2000) == _C.LR_ERR_UNSUPPORTED
  assert call(W=0) == _C.LR_ERR_INVALID_ARG
  assert call() == _C.LR_ERR_INVALID_ARG               # NULL pointers
  for kw in (dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")), dict(gamma=float("nan")),
             dict(gamma=float("inf"))):
    assert call(ptr=nn_, **kw) == _C.LR_ERR_INVALID_ARG, kw
  assert call(ptr=nn_) == _C.LR_ERR_INVALID_ARG        # params still NULL
