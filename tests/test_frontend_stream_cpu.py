"""Conv frontend sessions, host side: the fp64 restatement of a session equals the one-shot fp64
frontend on every slot's unpadded clip under every chunking; four wrong variants do not; the exact-integer cases meet
the conditions that let the GPU file ask for `==`; the emission rule; the size entry points; every rejection that
happens before device work; the driver's flag.  No GPU.
"""
import pytest
import torch

from lipreading_amd import _C, driver
from lipreading_amd import frontend_stream as FS
from lipreading_amd.frontend import ConvFrontend3D
from tests import frontend_stream_cases as C


def every_schedule(case):
  T = max(case.lens)
  return [(chunking, end_with, C.schedule(case.lens, chunking, end_with))
          for chunking in C.chunkings(T) for end_with in (True, False)]


# ---- 1: the session in fp64 equals the one-shot frontend ------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.BY_NAME))
def test_stream_ref_equals_the_one_shot_frontend_under_every_chunking(name):
  p = C.problem(name)
  for chunking, end_with, calls in every_schedule(p.case):
    feats, counts = C.stream_ref(p.x, p.case.lens, p.ws, p.bs, calls)
    for b, n in enumerate(p.case.lens):
      C.compare_exact(feats[b], p.features[b], "%s slot %d, chunks %s, end %s" % (name, b, chunking, end_with),
                      axes=("frame", "feature"))
      assert sum(row[b] for row in counts) == n


WRONG = {"ring depth 1": dict(ring=1), "no zero plane after the last frame": dict(zero_after=False),
         "emission delay 2": dict(ahead=(1, 1, 0)), "no zero plane before frame 0": dict(zero_before=False)}


@pytest.mark.parametrize("what", list(WRONG))
def test_a_wrong_session_leaves_the_equality(what):
  p = C.problem("sq16")
  T = max(p.case.lens)
  calls = C.schedule(p.case.lens, [1] * T, True)
  feats, _ = C.stream_ref(p.x, p.case.lens, p.ws, p.bs, calls, **WRONG[what])
  with pytest.raises(AssertionError, match="differ|shape"):
    for b in range(len(p.case.lens)):
      C.compare_exact(feats[b], p.features[b], what, axes=("frame", "feature"))


# ---- 2: the conditions of exactness -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.BY_NAME))
def test_exact_cases_meet_their_conditions(name):
  """A condition on the inputs: at every level every pre-pool value of the reference is an integer whose positive part
  is <= 256 (a bf16 value: the stored ReLU output is exact, and what ReLU removes never mattered), every fp32 partial
  sum is far below 2^24, and at least 10 % of every level's pooled values are non-zero (a dropped tap shows)."""
  p = C.problem(name)
  for b, (feats, pre, pooled) in enumerate(p.levels):
    for l, (z, q) in enumerate(zip(pre, pooled)):
      assert torch.equal(z, z.round()), (name, b, l)
      assert float(z.max()) <= C.BF16_EXACT, (name, b, l, float(z.max()))
      assert float(z.abs().max()) < 1 << 20, (name, b, l)
      assert float((q != 0).double().mean()) >= 0.10, (name, b, l, float((q != 0).double().mean()))
      assert torch.equal(C.bf16_round(q), q)


def test_bf16_rounding_between_levels_changes_nothing_on_exact_cases():
  p = C.problem("r16x32")
  calls = C.schedule(p.case.lens, [2, 2, 1], True)
  feats, _ = C.stream_ref(p.x, p.case.lens, p.ws, p.bs, calls, round_bf16=True)
  for b in range(len(p.case.lens)):
    C.compare_exact(feats[b], p.features[b], "rounded", axes=("frame", "feature"))


# ---- 3: the emission rule ---------------------------------------------------------------------------------------------

def test_emitted_and_counts_for_short_utterances():
  assert [C.emitted(n, False) for n in range(6)] == [0, 0, 0, 0, 1, 2]
  assert [C.emitted(n, True) for n in range(6)] == [0, 1, 2, 3, 4, 5]
  ws = [torch.zeros((L.cout, L.cin) + L.k, dtype=torch.float64) for L in C.LAYERS]
  bs = [torch.zeros(L.cout, dtype=torch.float64) for L in C.LAYERS]
  for n in range(6):
    x = torch.zeros((1, max(n, 1), 16, 16, 3), dtype=torch.float64)
    for end_with in (True, False):
      for chunking in ([max(n, 1)], [1] * max(n, 1)):
        calls = C.schedule((n,), chunking, end_with)
        if n == 0:   # nothing to end with: the end comes in a call of its own
          calls = [C.Call(0, 0, (0,), (1,))]
        _, counts = C.stream_ref(x, (n,), ws, bs, calls)
        fed, ended = 0, False
        for c, row in zip(calls, counts):
          before = C.emitted(fed, ended)
          fed, ended = fed + c.sizes[0], ended or bool(c.end[0])
          assert row[0] == C.emitted(fed, ended) - before, (n, end_with, chunking, c)
          assert row[0] <= c.chunk + (3 if any(c.end) else 0)
        assert ended and fed == n and sum(r[0] for r in counts) == n
  assert C.level_counts(5, False) == [5, 4, 3, 2] and C.level_counts(5, True) == [5, 5, 5, 5]
  assert C.level_counts(1, False) == [1, 0, 0, 0]


# ---- 4: the size entry points follow the header's formulas --------------------------------------------------------------

def a256(n):
  return (n + 255) // 256 * 256


def plane(h, w, c):
  return a256(2 * h * w * c)


def state_bytes(B, H, W):
  return a256(32 * B) + B * 2 * (plane(H, W, 4) + plane(H // 4, W // 4, 32) + plane(H // 8, W // 8, 64))


def ws_bytes(B, T, H, W):
  return (a256(48 * B) + a256(48 * B * (T + 3)) + B * T * plane(H, W, 4) + B * (T + 1) * plane(H // 4, W // 4, 32) +
          B * (T + 2) * plane(H // 8, W // 8, 64))


def test_size_entries_follow_the_headers_formulas():
  L = _C.lib()
  for B, H, W in ((1, 16, 16), (5, 16, 32), (2, 32, 32), (8, 96, 96), (3, 48, 32)):
    assert L.lr_conv_stream_state_bytes(B, H, W) == state_bytes(B, H, W)
    for T in (0, 1, 5, 9):
      assert L.lr_conv_stream_workspace_bytes(B, T, H, W) == ws_bytes(B, T, H, W)
  assert state_bytes(1, 96, 96) - a256(32) == 258048    # about 258 KB per slot at 96 x 96


def test_size_entries_reject_bad_shapes():
  L = _C.lib()
  for B, H, W in ((0, 16, 16), (-1, 16, 16), (2, 0, 16), (2, 16, 0), (2, 24, 16), (2, 16, 40), (2, 8, 16), (2, 1040, 16),
                  (65536, 16, 16)):
    assert L.lr_conv_stream_state_bytes(B, H, W) == 0
    assert L.lr_conv_stream_workspace_bytes(B, 4, H, W) == 0
  assert L.lr_conv_stream_workspace_bytes(2, -1, 16, 16) == 0
  assert L.lr_conv_stream_workspace_bytes(8, 65535 // 8 - 2, 16, 16) == 0     # B * (chunk_T + 3) > 65535
  assert L.lr_conv_stream_workspace_bytes(8, 65535 // 8 - 3, 16, 16) > 0


def test_entry_points_reject_nulls_and_short_buffers_without_a_device():
  L = _C.lib()
  p = 4096   # a non-NULL, aligned address that nothing dereferences: every check happens before any launch
  n = L.lr_conv_stream_state_bytes(2, 16, 16)
  w = L.lr_conv_stream_workspace_bytes(2, 3, 16, 16)
  bad, short = _C.LR_ERR_INVALID_ARG, _C.LR_ERR_WORKSPACE
  assert L.lr_conv_stream_reset(None, n, None, 2, 16, 16, None) == bad
  assert L.lr_conv_stream_reset(p, n, None, 2, 24, 16, None) == bad
  assert L.lr_conv_stream_reset(p, n, None, 0, 16, 16, None) == bad
  assert L.lr_conv_stream_reset(p + 4, n, None, 2, 16, 16, None) == bad
  assert L.lr_conv_stream_reset(p, n - 1, None, 2, 16, 16, None) == short
  assert L.lr_conv_stream_read(None, n, p, p, p, p, 2, 16, 16, None) == bad
  assert L.lr_conv_stream_read(p, n, None, None, None, None, 2, 16, 16, None) == bad
  assert L.lr_conv_stream_read(p, n - 1, p, None, None, None, 2, 16, 16, None) == short

  def advance(**kw):
    a = dict(x=p, flags=0, sb=9 * 768, st=768, sizes=None, end=None, w1=p, w2=p, w3=p, b1=p, b2=p, b3=p, feat=p,
             counts=p, state=p, nstate=n, ws=p, nws=w, B=2, T=3, H=16, W=16)
    a.update(kw)
    return L.lr_conv_stream_advance(a["x"], a["flags"], a["sb"], a["st"], a["sizes"], a["end"], a["w1"], a["w2"], a["w3"],
                                    a["b1"], a["b2"], a["b3"], a["feat"], a["counts"], a["state"], a["nstate"], a["ws"],
                                    a["nws"], a["B"], a["T"], a["H"], a["W"], None)
  for kw in (dict(x=None), dict(w1=None), dict(w2=None), dict(w3=None), dict(b1=None), dict(b2=None), dict(b3=None),
             dict(feat=None), dict(counts=None), dict(state=None), dict(ws=None), dict(B=0), dict(T=-1), dict(H=24),
             dict(W=8), dict(sb=-1), dict(st=-1), dict(flags=2), dict(state=p + 8), dict(ws=p + 8), dict(w2=p + 2),
             dict(x=p + 2, flags=_C.LR_CONV_STREAM_F32)):
    assert advance(**kw) == bad, kw
  assert advance(nstate=n - 1) == short and advance(nws=w - 1) == short
  assert advance(B=65535, nstate=1 << 40, nws=1 << 40) == _C.LR_ERR_UNSUPPORTED
  assert advance(T=0, x=None, feat=None, counts=None) == _C.LR_OK     # nothing to do, and nothing launched
  assert _C.LR_CONV_STREAM_MISMATCH == 1 and _C.LR_CONV_STREAM_AFTER_END == 2


# ---- 5: the Python front doors refuse before any device work -------------------------------------------------------------

def test_frontend_stream_refuses_before_device_work():
  fe = ConvFrontend3D()
  with pytest.raises(_C.LipReadingHipError, match="no CPU fallback"):
    FS.FrontendStream(fe, 2, 16, 16, "cpu")
  with pytest.raises(_C.LipReadingHipError, match="weights are on cpu"):
    FS.FrontendStream(fe, 2, 16, 16, "cuda")
  with pytest.raises(TypeError, match="ConvFrontend3D"):
    FS.FrontendStream(torch.nn.Linear(2, 2), 2, 16, 16, "cuda")
  with pytest.raises(ValueError, match="batch"):
    FS.FrontendStream(fe, 0, 16, 16, "cuda")
  for H, W in ((24, 16), (16, 0), (8, 16)):
    with pytest.raises(ValueError, match="multiples of 16"):
      FS.FrontendStream(fe, 2, H, W, "cuda")
  with pytest.raises(ValueError, match="chunk"):
    FS.ChunkedFrontend(fe, 0)
  with pytest.raises(TypeError, match="ConvFrontend3D"):
    FS.ChunkedFrontend(None, 4)
  assert callable(ConvFrontend3D.stream)
  import lipreading_amd
  for name in ("FrontendStream", "ChunkedFrontend", "ChunkedPixelLipReader", "PixelLiveTranscriber"):
    assert getattr(lipreading_amd, name) is getattr(FS, name)


def test_feed_refuses_wrong_clips_before_device_work():
  st = FS.FrontendStream.__new__(FS.FrontendStream)    # the checks read these three only
  st.batch, st.H, st.W = 2, 16, 32
  good = torch.zeros((2, 3, 3, 16, 32), dtype=torch.uint8)
  with pytest.raises(_C.LipReadingHipError, match="no CPU fallback"):
    st.feed(good)                                                            # a CPU tensor
  for clips, err, what in ((good.numpy(), TypeError, "tensor"), (good.to(torch.int16), TypeError, "uint8 or float32"),
                           (good.double(), TypeError, "uint8 or float32"), (good[0], ValueError, "batch, t, 3, H, W"),
                           (good[:1], ValueError, "1 utterances"), (good[:, :, :2], ValueError, "2 channels"),
                           (good[..., :16], ValueError, "16 x 16"), (good[:, :, :, :8], ValueError, "8 x 32")):
    with pytest.raises(err, match=what):
      st.feed(clips)


def _encoder(bidirectional=False, ctc=True, rnn_type="GRU"):
  from lipreading_amd.data import BOS, EOS, PAD
  from lipreading_amd.encoder import VideoEncoder
  c2i = {PAD: 0, BOS: 1, EOS: 2, "a": 3, "b": 4}
  return VideoEncoder(96, 8, rnn_type=rnn_type, num_layers=1, bidirectional=bidirectional, enable_ctc=ctc,
                      vocab_size=len(c2i), char2idx=c2i, device="cpu")


def test_any_projection_lets_a_bf16x3_encoder_in_and_the_default_stays():
  from lipreading_amd.encoder_lookahead import ChunkedLookaheadEncoder, LookaheadEncoderStream
  from lipreading_amd.encoder_stream import ChunkedEncoder, EncoderStream
  from lipreading_amd.frontend import PixelLipReader
  uni, bi = _encoder(), _encoder(bidirectional=True)
  PixelLipReader(uni), PixelLipReader(bi)
  assert uni.input_projection == bi.input_projection == 'bf16x3'
  msg = "a session runs the exact fp32 projection \\('f32'\\) only"
  with pytest.raises(ValueError, match=msg):
    EncoderStream(uni, 2, "cuda")
  with pytest.raises(ValueError, match=msg):
    ChunkedEncoder(uni, 4)
  with pytest.raises(ValueError, match=msg):
    LookaheadEncoderStream(bi, 2, "cuda")
  with pytest.raises(ValueError, match=msg):
    ChunkedLookaheadEncoder(bi, 4, 2)
  assert ChunkedEncoder(uni, 4, any_projection=True).any_projection
  assert ChunkedLookaheadEncoder(bi, 4, 2, any_projection=True).any_projection
  # the projection is past; what comes next is the device
  with pytest.raises(_C.LipReadingHipError, match="no CPU fallback"):
    EncoderStream(uni, 2, "cpu", any_projection=True)
  with pytest.raises(_C.LipReadingHipError, match="no CPU fallback"):
    LookaheadEncoderStream(bi, 2, "cpu", any_projection=True)
  with pytest.raises(ValueError, match="bidirectional"):
    ChunkedEncoder(bi, 4, any_projection=True)


def test_pixel_front_doors_refuse_what_they_cannot_run():
  from lipreading_amd.frontend import PixelLipReader
  from lipreading_amd.transformer import TransformerVideoEncoder

  class Dec(object):
    log_probs_input = True
  with pytest.raises(TypeError, match="PixelLipReader"):
    FS.PixelLiveTranscriber(_encoder(), Dec(), 2, 20, 16, 16, "cuda")
  with pytest.raises(ValueError, match="bidirectional"):
    FS.PixelLiveTranscriber(PixelLipReader(_encoder(bidirectional=True)), Dec(), 2, 20, 16, 16, "cuda")
  with pytest.raises(ValueError, match="no CTC head"):
    FS.PixelLiveTranscriber(PixelLipReader(_encoder(ctc=False)), Dec(), 2, 20, 16, 16, "cuda")
  with pytest.raises(ValueError, match="log_probs_input"):
    FS.PixelLiveTranscriber(PixelLipReader(_encoder()), object(), 2, 20, 16, 16, "cuda")
  from lipreading_amd.data import BOS, EOS, PAD
  c2i = {PAD: 0, BOS: 1, EOS: 2, "a": 3}
  tfm = TransformerVideoEncoder(96, d_model=8, nhead=2, num_layers=1, dim_feedforward=16, enable_ctc=True,
                                vocab_size=len(c2i), char2idx=c2i)
  with pytest.raises(TypeError, match="recurrent VideoEncoder"):
    FS.PixelLiveTranscriber(PixelLipReader(tfm), Dec(), 2, 20, 16, 16, "cuda")
  with pytest.raises(TypeError, match="recurrent VideoEncoder"):
    FS.ChunkedPixelLipReader(PixelLipReader(tfm), 4)
  with pytest.raises(TypeError, match="PixelLipReader"):
    FS.ChunkedPixelLipReader(_encoder(), 4)
  with pytest.raises(ValueError, match="uni-directional"):
    FS.ChunkedPixelLipReader(PixelLipReader(_encoder()), 4, lookahead=2)
  with pytest.raises(ValueError, match="bidirectional"):
    FS.ChunkedPixelLipReader(PixelLipReader(_encoder(bidirectional=True)), 4)
  ok = FS.ChunkedPixelLipReader(PixelLipReader(_encoder(bidirectional=True)), 4, lookahead=2)
  assert ok.enable_ctc and ok.lookahead == 2


# ---- 6: the driver's flag ----------------------------------------------------------------------------------------------

GOOD = ["--frontend=conv3d", "--encoder=rnn", "--ctc_decoder=beam", "--stream_chunk=5", "--stream_frontend=True",
        "--stream_encoder=True", "--bidirectional=False"]


def test_driver_flag_and_its_requirements():
  assert driver.DEFAULTS["stream_frontend"] is False and driver.parse_flags([])["stream_frontend"] is False
  f = driver.parse_flags(GOOD)
  assert f["stream_frontend"] is True and f["stream_encoder"] is True and f["frontend"] == "conv3d"
  ahead = [a for a in GOOD if a not in ("--stream_encoder=True", "--bidirectional=False")]
  f = driver.parse_flags(ahead + ["--stream_lookahead=4", "--bidirectional=True", "--enable_ctc=True", "--ctc_only=True"])
  assert f["stream_frontend"] is True and f["stream_lookahead"] == 4
  for drop, extra in (("--frontend=conv3d", []), ("--encoder=rnn", ["--encoder=transformer"]), ("--stream_chunk=5", []),
                      ("--stream_encoder=True", []), (None, ["--stream_lookahead=2"]),
                      ("--bidirectional=False", ["--bidirectional=True"])):
    with pytest.raises(SystemExit, match="stream_frontend"):
      driver.parse_flags([a for a in GOOD if a != drop] + extra)
  with pytest.raises(SystemExit, match="stream_frontend"):
    driver.stream_frontend_check(dict(driver.DEFAULTS, stream_frontend=True))


def test_the_old_rejections_still_fire_without_the_flag():
  base = ["--ctc_decoder=beam", "--stream_chunk=5"]
  with pytest.raises(SystemExit) as e:
    driver.parse_flags(base + ["--stream_encoder=True", "--bidirectional=False", "--frontend=conv3d"])
  assert str(e.value) == "--stream_encoder needs --encoder=rnn and --frontend=none"
  with pytest.raises(SystemExit) as e:
    driver.parse_flags(base + ["--stream_lookahead=3", "--bidirectional=True", "--enable_ctc=True", "--ctc_only=True",
                               "--frontend=conv3d"])
  assert str(e.value) == "--stream_lookahead needs --encoder=rnn and --frontend=none"
  with pytest.raises(SystemExit) as e:
    driver.parse_flags(base + ["--stream_encoder=True", "--bidirectional=False", "--encoder=transformer"])
  assert str(e.value) == "--stream_encoder needs --encoder=rnn and --frontend=none"
