"""Look-ahead sessions without a GPU: the reference of tests/test_gpu_lookahead.py restates torch.nn's
bidirectional stack and can tell the mistakes a look-ahead session could make; the host-side size entries follow the
header's formulas; the Python front doors and the driver's flag refuse what a session cannot run before any device work.

Restatement (float64, relative to the tensor's largest entry, y / log_probs / h / c): lc_ref over one advance against ONE
packed-sequence torch.nn call, and lc_ref with the whole rest as look-ahead in blocks of 4 against the single advance:
both within 1e-13 (measured: at most 8.2e-16).  The five wrong variants must move y by more than 1e-3 (printed below;
measured on bilstm36_b17 under blocks(5, 3) / ragged, relative to y's largest entry: carry_bwd 4.9e-1 / 4.7e-1,
commit_late 5.2e-1 / 4.3e-1, window_end 3.4e-1 / 3.5e-1, blind_upper 2.1e-1 / 2.5e-1, swapped 8.0e-1 / 7.5e-1), and each
plan is checked to hold an advance in which the variant's rule matters.
"""
import pytest
import torch

from lipreading_amd import _C, driver
from lipreading_amd.encoder import VideoEncoder
from lipreading_amd import encoder_lookahead as EL
from tests import lookahead_cases as C

RESTATE = 1e-13
MOVES = 1e-3


def _worst(got, want, fed, keys=("y", "lp", "h", "c")):
  worst = 0.0
  for k in keys:
    if want[k] is None:
      continue
    a, b = got[k], want[k]
    if k == "lp":
      a, b = C.fed_rows(a, fed), C.fed_rows(b, fed)
    worst = max(worst, float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30))
  return worst


_memo = {}


def setup(name):
  if name not in _memo:
    case = C.CASES[name]
    _memo[name] = (case, C.weights(case)) + C.inputs(case)
  return _memo[name]


@pytest.mark.parametrize("name", list(C.CASES))
def test_one_advance_restates_the_one_shot_model(name):
  case, w, x, lens = setup(name)
  one = C.one_shot_ref(case, w, x, lens, torch.float64)
  got = C.lc_ref(case, w, x, C.one_chunk(case, lens), torch.float64)
  err = _worst(got, one, lens)
  print("%-14s one_chunk vs one packed call %.2e" % (name, err))
  assert got["frames"] == lens and err <= RESTATE, (name, err)


@pytest.mark.parametrize("name", list(C.CASES))
def test_full_lookahead_restates_the_single_advance(name):
  case, w, x, lens = setup(name)
  one = C.lc_ref(case, w, x, C.one_chunk(case, lens), torch.float64)
  for plan in (C.blocks_4_full, C.frame_by_frame_full):
    got = C.lc_ref(case, w, x, plan(case, lens), torch.float64)
    err = _worst(got, one, lens)
    print("%-14s %-20s vs one_chunk %.2e" % (name, plan.__name__, err))
    assert got["frames"] == lens and err <= RESTATE, (name, plan.__name__, err)


def test_every_plan_consumes_every_frame_once():
  for name in C.CASES:
    case, w, x, lens = setup(name)
    for pname, make in C.PLANS.items():
      fed = [0] * len(lens)
      for op in make(case, lens):
        _, c, wdw, sizes, ahead = op
        assert 0 <= c <= wdw
        for b, (n, a) in enumerate(zip(sizes, ahead)):
          assert 0 <= n <= c and 0 <= a <= wdw - n and fed[b] + n + a <= lens[b], (name, pname, op)
          fed[b] += n
      assert fed == lens, (name, pname)


def _exercised(variant, case, plan):
  """the plan holds an advance in which the variant's rule matters"""
  feeds = [op for op in plan if op[0] == "feed"]
  if variant == "window_end":     # a slot whose own window ends before the window does
    return any(n > 0 and n + a < op[2] for op in feeds for n, a in zip(op[3], op[4]))
  if variant in ("commit_late", "blind_upper"):   # a consuming slot with look-ahead
    return any(n > 0 and a > 0 for op in feeds for n, a in zip(op[3], op[4]))
  if variant == "carry_bwd":      # a slot that consumes in two advances
    return any(sum(1 for op in feeds if op[3][b] > 0) > 1 for b in range(case.B))
  return case.layers > 1          # swapped


@pytest.mark.parametrize("plan", [C.blocks_5_3, C.ragged], ids=["blocks_5_3", "ragged"])
@pytest.mark.parametrize("variant", C.VARIANTS)
def test_wrong_variants_move_y(variant, plan):
  case, w, x, lens = setup("bilstm36_b17")
  p = plan(case, lens)
  assert _exercised(variant, case, p), (variant, "the plan does not exercise the rule")
  key = ("right", plan.__name__)
  if key not in _memo:
    _memo[key] = C.lc_ref(case, w, x, p, torch.float64)
  wrong = C.lc_ref(case, w, x, p, torch.float64, variant=variant)
  err = _worst(wrong, _memo[key], lens, keys=("y",))
  print("%-12s under %-10s moves y by %.2e" % (variant, plan.__name__, err))
  assert err > MOVES, (variant, err)


def test_bounded_lookahead_depends_on_the_cut_by_design():
  case, w, x, lens = setup("bilstm36_b17")
  one = C.lc_ref(case, w, x, C.one_chunk(case, lens), torch.float64)
  cut = C.lc_ref(case, w, x, C.blocks_5_3(case, lens), torch.float64)
  assert _worst(cut, one, lens, keys=("y",)) > MOVES
  # ... but layer 0's forward direction and its state do not know about the cut (the stack's first layer alone)
  first = case._replace(layers=1)
  a = C.lc_ref(first, w, x, C.blocks_5_3(case, lens), torch.float64)
  b = C.lc_ref(first, w, x, C.one_chunk(case, lens), torch.float64)
  assert _worst(a, b, lens, keys=("h", "c")) <= RESTATE
  assert float((a["y"][..., :case.H] - b["y"][..., :case.H]).abs().max()) <= RESTATE
  assert float((a["y"][..., case.H:] - b["y"][..., case.H:]).abs().max()) > MOVES


# ---- the size entries (host functions) ------------------------------------------------------------------------------

def a256(n):
  return (n + 255) // 256 * 256


def pack_bytes(G, I, H, layers):
  HT = (H + 15) // 16
  return (sum(2 * a256(4 * HT * (((I + 15) // 16 if l == 0 else 2 * HT) + HT) * G * 256) for l in range(layers)) +
          a256(4 * layers * 2 * 4 * 16 * HT))


def state_bytes(lstm, B, H, layers):
  Hp = (H + 15) // 16 * 16
  return a256(32 * B) + a256(4 * layers * B * Hp) * (2 if lstm else 1)


def ws_bytes(lstm, B, W, H, layers):
  Hp = (H + 15) // 16 * 16
  return (a256(4 * layers * 2 * max(W, 1) * B * Hp) +
          ((a256(4 * layers * 2 * B * Hp) + a256(4 * layers * B * Hp)) if lstm else 0))


def test_size_entries_follow_the_headers_formulas():
  L = _C.lib()
  for case in C.CASES.values():
    mode, G, lstm = C.MODE[case.cell], C.GATES[case.cell], case.cell == "LSTM"
    assert L.lr_rnn_bistream_pack_bytes(mode, case.I, case.H, case.layers) == pack_bytes(G, case.I, case.H, case.layers)
    assert (L.lr_rnn_bistream_state_bytes(mode, case.B, case.H, case.layers) ==
            state_bytes(lstm, case.B, case.H, case.layers) ==
            L.lr_rnn_stream_state_bytes(mode, case.B, case.H, case.layers))
    for T, W in ((0, 0), (0, 3), (1, 1), (1, 4), (case.T, case.T), (case.T, case.T + 7)):
      for Cc in (0, case.C):
        assert (L.lr_rnn_bistream_workspace_bytes(mode, case.B, T, W, case.I, case.H, case.layers, Cc) ==
                ws_bytes(lstm, case.B, W, case.H, case.layers)), (case.name, T, W)


@pytest.mark.parametrize("mode", [-1, 3, _C.LR_RNN_GRU | _C.LR_RNN_RECUR_SPLIT, _C.LR_RNN_LSTM | _C.LR_RNN_PROJ_BF16X3,
                                  _C.LR_RNN_GRU | _C.LR_RNN_PROJ_BF16X1])
def test_size_entries_reject_flagged_and_unknown_modes(mode):
  L = _C.lib()
  assert L.lr_rnn_bistream_pack_bytes(mode, 12, 20, 1) == 0
  assert L.lr_rnn_bistream_state_bytes(mode, 2, 20, 1) == 0
  assert L.lr_rnn_bistream_workspace_bytes(mode, 2, 4, 6, 12, 20, 1, 5) == 0


def test_size_entries_reject_bad_shapes():
  L = _C.lib()
  for I, H, layers in ((0, 20, 1), (-3, 20, 1), (12, 0, 1), (12, 20, 0), (12, 20, 17)):
    assert L.lr_rnn_bistream_pack_bytes(0, I, H, layers) == 0
  for B, H, layers in ((0, 20, 1), (-1, 20, 1), (2, 0, 1), (2, 20, 0), (2, 20, 17), (16 * 65535 + 1, 20, 1)):
    assert L.lr_rnn_bistream_state_bytes(0, B, H, layers) == 0
    assert L.lr_rnn_bistream_workspace_bytes(0, B, 4, 6, 12, H, layers, 0) == 0
  for T, W, I, Cc in ((-1, 4, 12, 0), (4, 3, 12, 0), (4, 6, 0, 0), (4, 6, 12, -1), (4, 6, 12, 257),
                      (4, (1 << 20) + 1, 12, 0)):
    assert L.lr_rnn_bistream_workspace_bytes(0, 2, T, W, I, 20, 1, Cc) == 0, (T, W, I, Cc)
  assert L.lr_rnn_bistream_workspace_bytes(0, 2, 4, 4, 12, 20, 1, 256) > 0


def test_entry_points_reject_nulls_and_short_buffers_without_a_device():
  L = _C.lib()
  two = (C.ctypes.c_void_p * 2)(64, 64)
  holed = (C.ctypes.c_void_p * 2)(64, None)
  assert L.lr_rnn_bistream_pack(None, 1 << 20, 0, two, two, two, two, 12, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_pack(64, 1 << 20, 0, two, None, two, two, 12, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_pack(64, 1 << 20, 0, two, two, holed, two, 12, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_pack(64, 16, 0, two, two, two, two, 12, 20, 1, None) == _C.LR_ERR_WORKSPACE
  assert L.lr_rnn_bistream_pack(64, 1 << 20, 0x100, two, two, two, two, 12, 20, 1, None) == _C.LR_ERR_UNSUPPORTED
  assert L.lr_rnn_bistream_pack(64, 1 << 20, 0, two, two, two, two, 0, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_reset(None, 1 << 20, None, 0, 2, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_reset(64, 16, None, 0, 2, 20, 1, None) == _C.LR_ERR_WORKSPACE
  assert L.lr_rnn_bistream_reset(64, 1 << 20, None, 0, 0, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_reset(64, 1 << 20, None, 0x1000, 2, 20, 1, None) == _C.LR_ERR_UNSUPPORTED
  big = 1 << 24

  def adv(x=64, pack=64, pack_b=big, state=64, state_b=big, ws=64, ws_b=big, mode=0, B=2, T=4, W=6, sb=12, st=24,
          head=(None, None, None), lp=None, Cc=0):
    return L.lr_rnn_bistream_advance(mode, x, sb, st, None, None, pack, pack_b, head[0], head[1], head[2], None, lp,
                                     state, state_b, ws, ws_b, B, T, W, 12, 20, 1, Cc, None)
  for kw in (dict(x=None), dict(pack=None), dict(state=None), dict(ws=None), dict(T=-1), dict(B=0), dict(W=3),
             dict(T=0, W=-1), dict(sb=-12), dict(st=-1), dict(state=72), dict(pack=68), dict(ws=65),
             dict(head=(64, 64, None), lp=64, Cc=5), dict(head=(64, 64, 64), lp=None, Cc=5), dict(lp=64)):
    assert adv(**kw) == _C.LR_ERR_INVALID_ARG, kw
  for kw in (dict(pack_b=16), dict(state_b=16), dict(ws_b=16)):
    assert adv(**kw) == _C.LR_ERR_WORKSPACE, kw
  for kw in (dict(mode=0x1000), dict(mode=0x100 | 1), dict(mode=3), dict(head=(64, 64, 64), lp=64, Cc=257),
             dict(W=(1 << 20) + 1)):
    assert adv(**kw) == _C.LR_ERR_UNSUPPORTED, kw
  assert adv(T=0) == _C.LR_OK and adv(T=0, W=0) == _C.LR_OK     # no frame consumed: succeeds and launches nothing
  assert L.lr_rnn_bistream_read(None, big, 64, None, 64, 64, 2, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_read(64, big, None, None, None, None, 2, 20, 1, None) == _C.LR_ERR_INVALID_ARG
  assert L.lr_rnn_bistream_read(64, 16, 64, None, 64, 64, 2, 20, 1, None) == _C.LR_ERR_WORKSPACE
  assert L.lr_rnn_bistream_read(64, big, 64, None, 64, 64, 0, 20, 1, None) == _C.LR_ERR_INVALID_ARG


# ---- Python front doors ---------------------------------------------------------------------------------------------

def _encoder(**kw):
  args = dict(frame_dim=12, hidden_size=20, rnn_type="GRU", num_layers=1, bidirectional=True)
  args.update(kw)
  return VideoEncoder(**args)


def test_the_classes_are_exported():
  import lipreading_amd
  assert lipreading_amd.LookaheadEncoderStream is EL.LookaheadEncoderStream
  assert lipreading_amd.ChunkedLookaheadEncoder is EL.ChunkedLookaheadEncoder
  assert lipreading_amd.LookaheadTranscriber is EL.LookaheadTranscriber
  with pytest.raises(AttributeError):
    lipreading_amd.no_such_name


@pytest.mark.parametrize("make", [lambda e: EL.LookaheadEncoderStream(e, 2, "cuda:0"),
                                  lambda e: EL.ChunkedLookaheadEncoder(e, 5, 2),
                                  lambda e: EL.LookaheadTranscriber(e, None, 2, 50, "cuda:0"),
                                  lambda e: e.stream_lookahead(2, "cuda:0")])
def test_sessions_refuse_what_cannot_look_ahead(make):
  with pytest.raises(ValueError, match=r"uni-directional.*VideoEncoder\.stream"):
    make(_encoder(bidirectional=False))
  enc = _encoder()
  enc.input_projection = "bf16x3"
  with pytest.raises(ValueError, match="input_projection"):
    make(enc)


def test_sessions_refuse_what_is_no_recurrent_encoder():
  with pytest.raises(TypeError, match="recurrent VideoEncoder"):
    EL.LookaheadEncoderStream(torch.nn.Linear(2, 2), 2, "cuda:0")


def test_the_causal_sessions_still_refuse_a_bidirectional_encoder():
  from lipreading_amd import encoder_stream as ES
  with pytest.raises(ValueError, match="bidirectional"):
    ES.EncoderStream(_encoder(), 2, "cuda:0")


def test_lookahead_stream_refuses_the_cpu_and_bad_arguments():
  with pytest.raises(_C.LipReadingHipError, match="device cpu"):
    EL.LookaheadEncoderStream(_encoder(), 2, "cpu")
  with pytest.raises(_C.LipReadingHipError, match="weights are on cpu"):
    EL.LookaheadEncoderStream(_encoder(), 2, "cuda:0")          # a CPU encoder: refused before the library is touched
  with pytest.raises(ValueError, match="batch"):
    EL.LookaheadEncoderStream(_encoder(), 0, "cuda:0")
  with pytest.raises(ValueError, match="chunk"):
    EL.ChunkedLookaheadEncoder(_encoder(), 0, 3)
  with pytest.raises(ValueError, match="lookahead"):
    EL.ChunkedLookaheadEncoder(_encoder(), 5, -1)
  with pytest.raises(ValueError, match="no final_state"):
    EL.ChunkedLookaheadEncoder(_encoder(), 5, 2)(torch.zeros(2, 3, 12), torch.tensor([3, 2]), need_final_state=True)
  with pytest.raises(ValueError, match="no CTC head"):
    EL.LookaheadTranscriber(_encoder(), None, 2, 50, "cuda:0")
  assert not hasattr(EL.LookaheadEncoderStream, "state")        # no final_state to offer: read() gives the forward halves


def test_feed_refuses_wrong_inputs_before_device_work():
  st = EL.LookaheadEncoderStream.__new__(EL.LookaheadEncoderStream)     # the argument checks alone: no device behind it
  st.batch, st.I = 2, 12
  with pytest.raises(ValueError, match=r"frame_dim \(I\) is 12"):
    st._frames_3d(torch.zeros(2, 3, 11))
  with pytest.raises(ValueError, match=r"frame_dim \(I\) is 12"):
    st._frames_3d(torch.zeros(2, 3, 5, 3))
  with pytest.raises(ValueError, match=r"session \(batch\) 2"):
    st._frames_3d(torch.zeros(3, 3, 12))
  with pytest.raises(TypeError, match="float32"):
    st._frames_3d(torch.zeros(2, 3, 12, dtype=torch.float64))
  with pytest.raises(TypeError, match="must be a tensor"):
    st._frames_3d([[0.0] * 12])
  with pytest.raises(ValueError, match="frames must be"):
    st._frames_3d(torch.zeros(2, 12))
  with pytest.raises(_C.LipReadingHipError, match="cpu tensor"):
    st._frames_3d(torch.zeros(2, 3, 4, 3))
  with pytest.raises(_C.LipReadingHipError, match="cpu tensor"):
    st.feed(torch.zeros(2, 3, 12))


GOOD = ["--stream_lookahead=2", "--stream_chunk=5", "--ctc_decoder=beam", "--enable_ctc=True", "--ctc_only=True",
        "--bidirectional=True", "--encoder=rnn", "--frontend=none"]


def test_driver_flag_and_its_checks():
  assert driver.DEFAULTS["stream_lookahead"] == -1 and driver.parse_flags([])["stream_lookahead"] == -1
  f = driver.parse_flags(GOOD)
  assert f["stream_lookahead"] == 2 and f["stream_chunk"] == 5 and f["stream_encoder"] is False
  assert driver.parse_flags([a.replace("lookahead=2", "lookahead=0") for a in GOOD])["stream_lookahead"] == 0
  for drop, extra, what in (("--stream_chunk=5", [], "stream_chunk"),
                            ("--ctc_decoder=beam", ["--stream_chunk=0"], "stream_chunk>0"),
                            ("--enable_ctc=True", [], "enable_ctc=True"),
                            ("--ctc_only=True", [], "ctc_only=True"),
                            ("--bidirectional=True", ["--bidirectional=False"], "bidirectional=True"),
                            (None, ["--encoder=transformer"], "encoder=rnn"),
                            (None, ["--frontend=conv3d"], "frontend=none"),
                            ("--stream_lookahead=2", ["--stream_lookahead=-2"], "stream_lookahead must be"),
                            ("--bidirectional=True", ["--bidirectional=False", "--stream_encoder=True"],
                             "does not go with --stream_encoder")):
    with pytest.raises(SystemExit, match=what):
      driver.parse_flags([a for a in GOOD if a != drop] + extra)
  with pytest.raises(SystemExit, match="ctc_decoder=beam"):
    driver.stream_lookahead_check(dict(driver.DEFAULTS, stream_lookahead=2, stream_chunk=5, enable_ctc=True,
                                       ctc_only=True))
  with pytest.raises(SystemExit, match="bidirectional=False"):          # stream_encoder_check stays as it is
    driver.parse_flags(GOOD + ["--stream_encoder=True"])
  driver.stream_lookahead_check(dict(driver.DEFAULTS))                  # off: nothing to check
