"""Encoder sessions without a GPU: the reference of tests/test_gpu_encoder_stream.py restates torch.nn
and can tell the mistakes a session could make; the host-side size entries follow the header's formulas; the Python
front doors and the driver's flag refuse what a session cannot run before any device work.

Restatement, measured on this table: stream_ref in float64 over the four chunkings against ONE packed-sequence torch.nn
call, relative to the tensor's largest entry, y / log_probs / h / c: 1.1e-16 (sat_lstm) .. 6.7e-16 (gru256).  The bound
is 10 x the worst: 7e-15.  The wrong variants leave it by ten orders of magnitude and more (printed below).
"""
import pytest
import torch

from lipreading_amd import _C, driver
from lipreading_amd.encoder import VideoEncoder
from lipreading_amd import encoder_stream as ES
from tests import encoder_stream_cases as C

RESTATE = 7e-15


def _worst(case, got, want, fed):
  worst = 0.0
  for k in ("y", "lp", "h", "c"):
    if want[k] is None:
      continue
    a, b = got[k], want[k]
    if k == "lp":
      a, b = C.fed_rows(a, fed), C.fed_rows(b, fed)
    worst = max(worst, float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30))
  return worst


@pytest.mark.parametrize("name", list(C.CASES))
def test_stream_ref_restates_one_packed_call(name):
  case = C.CASES[name]
  w = C.weights(case)
  x, lens = C.inputs(case)
  one = C.one_shot_ref(case, w, x, lens, torch.float64)
  for make in (C.one_chunk, C.frame_by_frame, C.in_chunks, C.ragged):
    err = _worst(case, C.stream_ref(case, w, x, make(case, lens), torch.float64), one, lens)
    print("%-12s %-16s %.2e" % (name, make.__name__, err))
    assert err <= RESTATE, (name, make.__name__, err)


def _reset_plan(case, lens):
  """part of every utterance, a masked reset of every other slot, then those slots' utterances from the start"""
  mask = [b % 2 for b in range(case.B)]
  first = [min(n, 3) for n in lens]
  return ([("feed", 3, first), ("reset", mask)] +
          [("feed", case.T, [n if m else n - f for n, m, f in zip(lens, mask, first)])])


@pytest.mark.parametrize("variant,name,plan", [
    ("idle_zeroed", "lstm36_b17", C.ragged),
    ("c_not_reset", "lstm36_b17", _reset_plan),
    ("bhn_folded", "gru256", C.in_chunks),
    ("layer1_prev_frame", "gru256", C.frame_by_frame),
])
def test_wrong_variants_leave_the_bound(variant, name, plan):
  case = C.CASES[name]
  w = C.weights(case)
  x, lens = C.inputs(case)
  p = plan(case, lens)
  right = C.stream_ref(case, w, x, p, torch.float64)
  if plan is not _reset_plan:
    assert _worst(case, right, C.one_shot_ref(case, w, x, lens, torch.float64), lens) <= RESTATE
  wrong = C.stream_ref(case, w, x, p, torch.float64, variant=variant)
  err = _worst(case, wrong, right, lens)
  print("%-18s on %-12s %.2e" % (variant, name, err))
  assert err > 1e3 * RESTATE, (variant, err)


def test_a_masked_reset_in_the_reference_restarts_the_slot():
  case = C.CASES["lstm36_b17"]
  w = C.weights(case)
  x, lens = C.inputs(case)
  got = C.stream_ref(case, w, x, _reset_plan(case, lens), torch.float64)
  assert _worst(case, got, C.one_shot_ref(case, w, x, lens, torch.float64), lens) <= RESTATE


# ---- the size entries (host functions) ------------------------------------------------------------------------------

def a256(n):
  return (n + 255) // 256 * 256


def pack_bytes(G, I, H, layers):
  HT = (H + 15) // 16
  return (sum(a256(4 * HT * (((I if l == 0 else H) + 15) // 16 + HT) * G * 256) for l in range(layers)) +
          a256(4 * layers * 4 * 16 * HT))


def state_bytes(lstm, B, H, layers):
  Hp = (H + 15) // 16 * 16
  return a256(32 * B) + a256(4 * layers * B * Hp) * (2 if lstm else 1)


def ws_bytes(lstm, B, T, H, layers):
  Hp = (H + 15) // 16 * 16
  return a256(4 * layers * max(T, 1) * B * Hp) + (a256(4 * layers * B * Hp) if lstm else 0)


def test_size_entries_follow_the_headers_formulas():
  L = _C.lib()
  for case in C.CASES.values():
    mode, G, lstm = C.MODE[case.cell], C.GATES[case.cell], case.cell == "LSTM"
    assert L.lr_rnn_stream_pack_bytes(mode, case.I, case.H, case.layers) == pack_bytes(G, case.I, case.H, case.layers)
    assert L.lr_rnn_stream_state_bytes(mode, case.B, case.H, case.layers) == state_bytes(lstm, case.B, case.H, case.layers)
    for T in (0, 1, case.T):
      for Cc in (0, case.C):
        assert (L.lr_rnn_stream_workspace_bytes(mode, case.B, T, case.I, case.H, case.layers, Cc) ==
                ws_bytes(lstm, case.B, T, case.H, case.layers))


@pytest.mark.parametrize("mode", [-1, 3, _C.LR_RNN_GRU | _C.LR_RNN_RECUR_SPLIT, _C.LR_RNN_LSTM | _C.LR_RNN_PROJ_BF16X3,
                                  _C.LR_RNN_GRU | _C.LR_RNN_PROJ_BF16X1])
def test_size_entries_reject_flagged_and_unknown_modes(mode):
  L = _C.lib()
  assert L.lr_rnn_stream_pack_bytes(mode, 12, 20, 1) == 0
  assert L.lr_rnn_stream_state_bytes(mode, 2, 20, 1) == 0
  assert L.lr_rnn_stream_workspace_bytes(mode, 2, 4, 12, 20, 1, 5) == 0


def test_size_entries_reject_bad_shapes():
  L = _C.lib()
  for I, H, layers in ((0, 20, 1), (-3, 20, 1), (12, 0, 1), (12, 20, 0), (12, 20, 17)):
    assert L.lr_rnn_stream_pack_bytes(0, I, H, layers) == 0
  for B, H, layers in ((0, 20, 1), (-1, 20, 1), (2, 0, 1), (2, 20, 0), (2, 20, 17), (16 * 65535 + 1, 20, 1)):
    assert L.lr_rnn_stream_state_bytes(0, B, H, layers) == 0
    assert L.lr_rnn_stream_workspace_bytes(0, B, 4, 12, H, layers, 0) == 0
  for T, I, Cc in ((-1, 12, 0), (4, 0, 0), (4, 12, -1), (4, 12, 257), ((1 << 20) + 1, 12, 0)):
    assert L.lr_rnn_stream_workspace_bytes(0, 2, T, I, 20, 1, Cc) == 0
  assert L.lr_rnn_stream_workspace_bytes(0, 2, 4, 12, 20, 1, 256) > 0


def test_entry_points_reject_nulls_and_short_buffers_without_a_device():
  L = _C.lib()
  four = (C.ctypes.c_void_p * 1)(64)
  assert L.lr_rnn_stream_pack(None, 1 << 20, 0, four, four, four, four, 12, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_stream_pack(64, 16, 0, four, four, four, four, 12, 20, 1, None) == _C.LR_ERR_WORKSPACE
  assert L.lr_rnn_stream_pack(64, 1 << 20, 0x100, four, four, four, four, 12, 20, 1, None) == _C.LR_ERR_UNSUPPORTED
  assert L.lr_rnn_stream_reset(None, 1 << 20, None, 0, 2, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_stream_reset(64, 16, None, 0, 2, 20, 1, None) == _C.LR_ERR_WORKSPACE
  assert L.lr_rnn_stream_reset(64, 1 << 20, None, 0, 0, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_stream_reset(64, 1 << 20, None, 0x1000, 2, 20, 1, None) == _C.LR_ERR_UNSUPPORTED
  big = 1 << 24

  def adv(x=64, pack=64, pack_b=big, state=64, state_b=big, ws=64, ws_b=big, mode=0, B=2, T=4, head=(None, None, None),
          lp=None, Cc=0):
    return L.lr_rnn_stream_advance(mode, x, 12, 24, None, pack, pack_b, head[0], head[1], head[2], None, lp, state,
                                   state_b, ws, ws_b, B, T, 12, 20, 1, Cc, None)
  for kw in (dict(x=None), dict(pack=None), dict(state=None), dict(ws=None), dict(T=-1), dict(B=0),
             dict(head=(64, 64, None), lp=64, Cc=5), dict(head=(64, 64, 64), lp=None, Cc=5), dict(lp=64)):
    assert adv(**kw) == _C.LR_ERR_INVALID_ARG, kw
  for kw in (dict(pack_b=16), dict(state_b=16), dict(ws_b=16)):
    assert adv(**kw) == _C.LR_ERR_WORKSPACE, kw
  for kw in (dict(mode=0x1000), dict(mode=0x100 | 1), dict(mode=3), dict(head=(64, 64, 64), lp=64, Cc=257)):
    assert adv(**kw) == _C.LR_ERR_UNSUPPORTED, kw
  assert adv(T=0) == _C.LR_OK                                   # no frame: succeeds and launches nothing
  assert L.lr_rnn_stream_read(None, big, 64, None, 64, 64, 2, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_stream_read(64, big, None, None, None, None, 2, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_stream_read(64, 16, 64, None, 64, 64, 2, 20, 1, None) == _C.LR_ERR_WORKSPACE


# ---- Python front doors ---------------------------------------------------------------------------------------------

def _encoder(**kw):
  args = dict(frame_dim=12, hidden_size=20, rnn_type="GRU", num_layers=1, bidirectional=False)
  args.update(kw)
  return VideoEncoder(**args)


@pytest.mark.parametrize("make", [lambda e: ES.EncoderStream(e, 2, "cuda:0"), lambda e: ES.ChunkedEncoder(e, 5),
                                  lambda e: ES.LiveTranscriber(e, None, 2, 50, "cuda:0"), lambda e: e.stream(2, "cuda:0")])
def test_sessions_refuse_what_cannot_run_causally(make):
  with pytest.raises(ValueError, match="bidirectional"):
    make(_encoder(bidirectional=True))
  enc = _encoder()
  enc.input_projection = "bf16x3"
  with pytest.raises(ValueError, match="input_projection"):
    make(enc)


def test_encoder_stream_refuses_the_cpu_and_bad_batches():
  with pytest.raises(_C.LipReadingHipError, match="device cpu"):
    ES.EncoderStream(_encoder(), 2, "cpu")
  with pytest.raises(_C.LipReadingHipError, match="weights are on cpu"):
    ES.EncoderStream(_encoder(), 2, "cuda:0")          # a CPU encoder: refused before the library is touched
  with pytest.raises(ValueError, match="batch"):
    ES.EncoderStream(_encoder(), 0, "cuda:0")
  with pytest.raises(ValueError, match="chunk"):
    ES.ChunkedEncoder(_encoder(), 0)


def test_feed_refuses_wrong_inputs_before_device_work():
  st = ES.EncoderStream.__new__(ES.EncoderStream)     # the argument checks alone: no device behind it
  st.batch, st.I = 2, 12
  with pytest.raises(ValueError, match=r"frame_dim \(I\) is 12"):
    st._frames_3d(torch.zeros(2, 3, 11))
  with pytest.raises(ValueError, match=r"frame_dim \(I\) is 12"):
    st._frames_3d(torch.zeros(2, 3, 5, 3))
  with pytest.raises(ValueError, match=r"session \(batch\) 2"):
    st._frames_3d(torch.zeros(3, 3, 12))
  with pytest.raises(TypeError, match="float32"):
    st._frames_3d(torch.zeros(2, 3, 12, dtype=torch.float64))
  with pytest.raises(ValueError, match="frames must be"):
    st._frames_3d(torch.zeros(2, 12))
  with pytest.raises(_C.LipReadingHipError, match="cpu tensor"):
    st._frames_3d(torch.zeros(2, 3, 4, 3))


GOOD = ["--stream_encoder=True", "--stream_chunk=5", "--ctc_decoder=beam", "--enable_ctc=True", "--ctc_only=True"]


def test_driver_flag_and_its_checks():
  assert driver.DEFAULTS["stream_encoder"] is False and driver.parse_flags([])["stream_encoder"] is False
  f = driver.parse_flags(GOOD)
  assert f["stream_encoder"] is True and f["stream_chunk"] == 5
  for drop, extra, what in (("--stream_chunk=5", [], "stream_chunk"), ("--ctc_decoder=beam", [], "ctc_decoder=beam"),
                            (None, ["--bidirectional=True"], "bidirectional=False"),
                            (None, ["--encoder=transformer"], "encoder=rnn"),
                            (None, ["--frontend=conv3d"], "frontend=none")):
    with pytest.raises(SystemExit, match=what):
      driver.parse_flags([a for a in GOOD if a != drop] + extra)
  with pytest.raises(SystemExit, match="stream_chunk"):
    driver.stream_encoder_check(dict(driver.DEFAULTS, stream_encoder=True))
