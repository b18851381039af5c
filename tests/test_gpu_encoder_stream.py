"""Encoder sessions on the MI355X (lr_rnn_stream_*, lipreading_amd/encoder_stream.py).

Every case runs with NaN-filled outputs, a 0xFF-filled workspace, guard words either side of y and log_probs, ragged
sizes per slot, NaN in the rows of a chunk no frame was fed for, and a head mask with two zeros (tests/
encoder_stream_cases.py).  The reference of every number is torch.nn on the CPU fed chunk by chunk (stream_ref).

Against float64 (hold's rule of tests/test_gpu_transformer_fp64.py as it stands: element-wise, relative to the float64
tensor's largest entry, 4 x the error torch.nn's float32 CPU run makes on the same case, never less than 4 ulp): the
figures of the table are printed by the test; the figures below are what an MI355X gave.

MEASURED (an MI355X; float32 CPU error, the bound = 4 x max(that, 1 ulp = 1.19e-7), the device's error):
  gru20_i7 y                               cpu fp32 1.57e-07  bound 6.30e-07  device 1.15e-07
  gru20_i7 log_probs                       cpu fp32 7.61e-08  bound 4.77e-07  device 6.81e-08
  gru20_i7 h                               cpu fp32 7.83e-08  bound 4.77e-07  device 7.83e-08
  gru20_i7 log_probs of the zero row       cpu fp32 2.12e-08  bound 4.77e-07  device 2.12e-08
  lstm36_b17 y                             cpu fp32 2.85e-07  bound 1.14e-06  device 2.34e-07
  lstm36_b17 log_probs                     cpu fp32 1.03e-07  bound 4.77e-07  device 1.03e-07
  lstm36_b17 h                             cpu fp32 1.73e-07  bound 6.94e-07  device 1.39e-07
  lstm36_b17 c                             cpu fp32 7.60e-08  bound 4.77e-07  device 7.77e-08
  lstm36_b17 log_probs of the zero row     cpu fp32 2.15e-08  bound 4.77e-07  device 2.15e-08
  rnn16 y                                  cpu fp32 8.58e-08  bound 4.77e-07  device 1.06e-07
  rnn16 log_probs                          cpu fp32 9.27e-08  bound 4.77e-07  device 5.30e-08
  rnn16 h                                  cpu fp32 8.03e-08  bound 4.77e-07  device 9.76e-08
  rnn16 log_probs of the zero row          cpu fp32 9.88e-09  bound 4.77e-07  device 9.88e-09
  gru256 y                                 cpu fp32 2.51e-07  bound 1.00e-06  device 1.97e-07
  gru256 log_probs                         cpu fp32 9.91e-08  bound 4.77e-07  device 7.45e-08
  gru256 h                                 cpu fp32 2.47e-07  bound 9.88e-07  device 2.13e-07
  gru256 log_probs of the zero row         cpu fp32 1.70e-08  bound 4.77e-07  device 1.70e-08
  lstm700 y                                cpu fp32 3.92e-07  bound 1.57e-06  device 4.11e-07
  lstm700 log_probs                        cpu fp32 8.29e-08  bound 4.77e-07  device 8.39e-08
  lstm700 h                                cpu fp32 3.92e-07  bound 1.57e-06  device 3.41e-07
  lstm700 c                                cpu fp32 3.89e-07  bound 1.56e-06  device 3.42e-07
  lstm700 log_probs of the zero row        cpu fp32 5.25e-08  bound 4.77e-07  device 5.25e-08
  sat_gru y                                cpu fp32 7.79e-08  bound 4.77e-07  device 8.41e-08
  sat_gru log_probs                        cpu fp32 8.38e-08  bound 4.77e-07  device 9.71e-08
  sat_gru h                                cpu fp32 6.74e-08  bound 4.77e-07  device 6.62e-08
  sat_gru log_probs of the zero row        cpu fp32 2.87e-09  bound 4.77e-07  device 2.87e-09
  sat_lstm y                               cpu fp32 4.63e-08  bound 4.77e-07  device 5.68e-08
  sat_lstm log_probs                       cpu fp32 8.90e-08  bound 4.77e-07  device 8.52e-08
  sat_lstm h                               cpu fp32 3.15e-08  bound 4.77e-07  device 3.90e-08
  sat_lstm c                               cpu fp32 7.65e-09  bound 4.77e-07  device 1.26e-08
  sat_lstm log_probs of the zero row       cpu fp32 1.35e-08  bound 4.77e-07  device 1.35e-08
The device lands at 0.6 .. 1.7 of the float32 CPU run's own error; no bound was tuned to it.
"""
import re

import pytest
import torch

from tests import encoder_stream_cases as C
from tests.test_gpu_transformer_fp64 import hold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


_memo = {}


def setup(name):
  """(case, weights, x, lens), made once"""
  if name not in _memo:
    case = C.CASES[name]
    _memo[name] = (case, C.weights(case)) + C.inputs(case)
  return _memo[name]


def ref(name, plan_name, dtype):
  key = (name, plan_name, dtype)
  if key not in _memo:
    case, w, x, lens = setup(name)
    _memo[key] = C.stream_ref(case, w, x, getattr(C, plan_name)(case, lens), dtype)
  return _memo[key]


def session_run(name, dev, plan_name, **kw):
  key = (name, plan_name, "gpu", tuple(sorted(kw.items())))
  if key not in _memo:
    case, w, x, lens = setup(name)
    _memo[key] = C.Session(case, w, dev).run(x, getattr(C, plan_name)(case, lens), **kw)
  return _memo[key]


def same_bits(a, b, what):
  for k in ("y", "lp", "h", "c", "frames", "state", "zero_row"):
    if a[k] is None or b[k] is None:
      assert a[k] is None and b[k] is None, (what, k)
      continue
    u, v = (C.fed_rows(a[k], a["fed"]), C.fed_rows(b[k], b["fed"])) if k == "lp" else (a[k], b[k])
    assert torch.equal(u, v), (what, k)


# ---- 1: against float64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.CASES))
def test_session_matches_float64(dev, name):
  case, w, x, lens = setup(name)
  got = session_run(name, dev, "in_chunks")
  r64, r32 = ref(name, "in_chunks", torch.float64), ref(name, "in_chunks", torch.float32)
  assert got["fed"] == lens and got["frames"].cpu().tolist() == lens
  hold(name + " y", got["y"], r64["y"], r32["y"])
  hold(name + " log_probs", C.fed_rows(got["lp"], lens), C.fed_rows(r64["lp"], lens), C.fed_rows(r32["lp"], lens))
  hold(name + " h", got["h"], r64["h"], r32["h"])
  if case.cell == "LSTM":
    hold(name + " c", got["c"], r64["c"], r32["c"])
  if got["zero_row"] is not None:   # rows past a slot's frames: the head of the zero row
    z = torch.zeros(1, case.H)
    hold(name + " log_probs of the zero row", got["zero_row"].view(1, -1), C.head(case, w, z, torch.float64),
         C.head(case, w, z, torch.float32))
  lp = C.fed_rows(got["lp"], lens)
  assert (lp[:, 1] < -90).all() and (lp[:, case.C - 1] < -90).all() and torch.isfinite(lp).all()   # masked: finite, ~-103


# ---- 2: bit for bit under chunking ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.BIT_CASES)
def test_every_chunking_gives_the_same_bits(dev, name):
  one = session_run(name, dev, "one_chunk")
  for plan in ("frame_by_frame", "in_chunks", "ragged"):
    same_bits(session_run(name, dev, plan), one, plan)
  case, w, x, lens = setup(name)
  again = C.Session(case, w, dev).run(x, C.ragged(case, lens), read_between=True)   # a second run, reads between feeds
  same_bits(again, session_run(name, dev, "ragged"), "second run")


# ---- 3: slots are independent ---------------------------------------------------------------------------------------

def test_a_permuted_batch_gives_the_permuted_bits(dev):
  case, w, x, lens = setup("gru256")
  perm = [2, 0, 3, 1]
  base = session_run("gru256", dev, "one_chunk")
  got = C.Session(case, w, dev).run(x[perm], C.one_chunk(case, [lens[p] for p in perm]))
  assert torch.equal(got["y"], base["y"][perm]) and torch.equal(got["h"], base["h"][:, perm])
  for i, p in enumerate(perm):
    assert torch.equal(got["lp"][i, :lens[p]], base["lp"][p, :lens[p]])


def test_alone_equals_slot_16_of_17(dev):
  case, w, x, lens = setup("lstm36_b17")
  base = session_run("lstm36_b17", dev, "one_chunk")
  got = C.Session(case, w, dev, B=1).run(x[16:17], [("feed", case.T, [lens[16]])])
  n = lens[16]
  assert torch.equal(got["y"][0], base["y"][16]) and torch.equal(got["lp"][0, :n], base["lp"][16, :n])
  assert torch.equal(got["h"][:, 0], base["h"][:, 16]) and torch.equal(got["c"][:, 0], base["c"][:, 16])


def test_a_masked_reset_restarts_only_its_slots(dev):
  case, w, x, lens = setup("lstm36_b17")
  base = session_run("lstm36_b17", dev, "one_chunk")
  s = C.Session(case, w, dev)
  first = [min(n, 3) for n in lens]
  mask = [b % 2 for b in range(case.B)]
  keep = [b for b in range(case.B) if not mask[b]]
  gone = [b for b in range(case.B) if mask[b]]
  s.feed(x[:, :3].to(dev), first)
  h0, c0, f0, _ = s.read()
  s.reset(mask)
  h1, c1, f1, st1 = s.read()
  assert torch.equal(h1[:, keep], h0[:, keep]) and torch.equal(c1[:, keep], c0[:, keep]) and torch.equal(f1[keep], f0[keep])
  assert not h1[:, gone].any() and not c1[:, gone].any() and not f1[gone].any() and not st1.any()
  # the reset slots from their first frame, the others go on: everybody ends where a fresh session ends
  xc = torch.full((case.B, case.T, case.I), float("nan"))
  sizes = []
  for b, n in enumerate(lens):
    lo = 0 if mask[b] else first[b]
    xc[b, :n - lo] = x[b, lo:n]
    sizes.append(n - lo)
  y, lp = s.feed(xc.to(dev), sizes)
  for b in gone:
    assert torch.equal(y[b], base["y"][b]) and torch.equal(lp[b, :lens[b]], base["lp"][b, :lens[b]])
  assert torch.equal(s.state, base["state"])


# ---- 4, 7: the Python front doors -------------------------------------------------------------------------------------

def _char2idx():
  from lipreading_amd.data import BOS, EOS, PAD
  c2i = {PAD: 0, BOS: 1, EOS: 2}
  for ch in " abcdefgh":
    c2i[ch] = len(c2i)
  return c2i


def _encoder(dev, rnn_type="GRU", H=32, layers=2, ctc=True):
  from lipreading_amd.encoder import VideoEncoder
  torch.manual_seed(11)
  c2i = _char2idx()
  return VideoEncoder(204, H, rnn_type=rnn_type, num_layers=layers, bidirectional=False, enable_ctc=ctc,
                      vocab_size=len(c2i), char2idx=c2i, device=dev).to(dev).eval()


def test_strided_views_go_in_without_a_copy(dev):
  enc = _encoder(dev)
  g = torch.Generator().manual_seed(3)
  frames = torch.randn(3, 20, 68, 3, generator=g).to(dev)
  a, b = enc.stream(3, dev), enc.stream(3, dev)
  for t0, t1 in ((0, 7), (7, 8), (8, 20)):
    view = frames[:, t0:t1]
    assert not view.is_contiguous() and a._frames_3d(view).data_ptr() == view.data_ptr()
    lp_v, y_v = a.feed(view, need_hidden=True)
    lp_c, y_c = b.feed(view.contiguous().view(3, t1 - t0, 204), need_hidden=True)
    assert torch.equal(lp_v, lp_c) and torch.equal(y_v, y_c)
  assert torch.equal(a.state_buf, b.state_buf) and a.frames().cpu().tolist() == [20, 20, 20]
  assert a.state().shape == (2, 3, 32)


def test_live_transcriber_equals_the_one_shot_search(dev):
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.encoder_stream import LiveTranscriber
  enc = _encoder(dev)
  dec = BeamCTCDecoder(ctc_labels(_char2idx()), beam_width=8, log_probs_input=True)
  g = torch.Generator().manual_seed(4)
  frames = torch.randn(3, 23, 204, generator=g).to(dev)
  lens = torch.tensor([23, 11, 17], dtype=torch.int32, device=dev)
  lp = enc.stream(3, dev).feed(frames, lens)          # the one-chunk session
  want, want_off = dec.decode(lp, lens)
  live = LiveTranscriber(enc, dec, 3, 23, dev)
  for t0 in range(0, 23, 5):
    t1 = min(23, t0 + 5)
    live.feed(frames[:, t0:t1], (lens - t0).clamp(0, t1 - t0))
  got, got_off = live.result()
  assert got == want and [[o.tolist() for o in r] for r in got_off] == [[o.tolist() for o in r] for r in want_off]
  assert [p[0] for p in live.partial()] == [s[0] for s in want]
  live.reset(torch.tensor([0, 1, 0], device=dev))
  live.feed(frames[1:2].expand(3, -1, -1), torch.tensor([0, 11, 0], dtype=torch.int32, device=dev))
  assert live.result()[0] == want


@pytest.mark.parametrize("rnn_type", ["GRU", "LSTM"])
def test_state_is_a_decoders_previous_state(dev, rnn_type):
  from lipreading_amd.attention_decoder import CharDecodingStep
  enc = _encoder(dev, rnn_type=rnn_type, layers=1)
  c2i = _char2idx()
  step = CharDecodingStep(enc, char_dim=8, vocab_size=len(c2i), char2idx=c2i, device=dev).to(dev).eval()
  g = torch.Generator().manual_seed(5)
  frames = torch.randn(2, 9, 204, generator=g).to(dev)
  lens = torch.tensor([9, 6], dtype=torch.int32, device=dev)
  st = enc.stream(2, dev)
  _, hidden = st.feed(frames, lens, need_hidden=True)
  state = st.state()
  with torch.no_grad():
    _, want_hidden, want_state = enc(frames, lens, max_len=9)
  hs, ws = (state, want_state) if rnn_type == "LSTM" else ((state,), (want_state,))
  for a, b in zip(hs, ws):
    assert a.shape == b.shape == (1, 2, 32)
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)      # shapes and convention; the numbers are test 1's
  torch.testing.assert_close(hidden, want_hidden, rtol=1e-4, atol=1e-5)
  tokens = torch.tensor([[1, 4, 5], [1, 6, 2]], device=dev)
  with torch.no_grad():
    out = step.decode_sequence(tokens, state, lens, hidden)
  assert out[0].shape == (2, 3, len(c2i)) and torch.isfinite(out[0]).all()


def test_chunked_encoder_goes_through_ctc_cer(dev):
  from lipreading_amd import train as T
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.encoder_stream import ChunkedEncoder
  enc = _encoder(dev)
  c2i = _char2idx()
  dec = BeamCTCDecoder(ctc_labels(c2i), beam_width=8, log_probs_input=True)
  g = torch.Generator().manual_seed(6)
  frames = torch.randn(3, 14, 68, 3, generator=g)
  frame_lens = torch.tensor([14, 9, 12])
  chars = torch.tensor([[1, 4, 5, 2], [1, 6, 2, 0], [1, 7, 8, 2]])
  char_lens = torch.tensor([4, 3, 4])
  loader = [(frames, frame_lens, chars, char_lens)]
  chunked = ChunkedEncoder(enc, 4)
  lp, hidden, state = chunked(frames.to(dev), frame_lens.to(dev), max_len=14)
  one = enc.stream(3, dev).feed(frames.to(dev), frame_lens.to(dev), need_hidden=True)
  assert torch.equal(lp, one[0]) and torch.equal(hidden, one[1]) and state.shape == (2, 3, 32)
  with torch.no_grad():
    want = enc(frames.to(dev), frame_lens.to(dev), max_len=14)
  torch.testing.assert_close(lp, want[0], rtol=1e-4, atol=1e-4)
  cer = T.ctc_cer(chunked, loader, dev, c2i, dec)
  assert 0.0 <= cer and cer == T.ctc_cer(ChunkedEncoder(enc, 14), loader, dev, c2i, dec)


def test_driver_streams_the_encoder(dev, tmp_path, capsys):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=6, captions_per_video=4, seed=7)
  common = ["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True", "--ctc_only=True",
            "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=0", "--ctc_decoder=beam", "--beam_width=8",
            "--stream_chunk=5", "--stream_encoder=True"]
  cers = []
  for score in ("host", "device"):   # the device's scoring loop takes the chunked encoder as well
    capsys.readouterr()
    out = driver.run(**driver.parse_flags(common + ["--score=" + score]))
    text = capsys.readouterr().out
    assert re.search(r"Commit delay \(chunks of 5 frames\): .*\(encoder streamed\)", text), text
    cers.append(float(re.search(r"\tCER:\s+(\S+)", text).group(1)))
    assert "commit_delay" in out
  assert 0.0 <= cers[0] == cers[1]


# ---- 5: traps -------------------------------------------------------------------------------------------------------

def _status_words(state, B):
  return state[:32 * B].view(torch.int32).view(B, 8)[:, 6]


@pytest.mark.parametrize("how", ["H", "layers", "cell"])
def test_an_advance_of_another_configuration_leaves_the_state_alone(dev, how):
  from lipreading_amd import _C
  case, w, x, lens = setup("lstm36_b17")
  s = C.Session(case, w, dev)
  s.feed(x[:, :3].to(dev), [min(n, 3) for n in lens])
  before = s.state.clone()
  kw = dict(H=20) if how == "H" else dict(layers=1) if how == "layers" else dict(mode=0)
  ws = torch.full((1 << 22,), 0xFF, dtype=torch.uint8, device=dev)
  y = torch.full((case.B, 2, 64), float("nan"), device=dev)
  _C.check(s.advance_raw(x[:, 3:5].to(dev), None, y, None, ws, **kw), "advance")
  after = s.state.clone()
  assert (_status_words(after, case.B) == _C.LR_RNN_STREAM_MISMATCH).all()
  _status_words(after, case.B).zero_()
  assert torch.equal(after, before)
  h, c, frames, status = s.read()
  assert (status == _C.LR_RNN_STREAM_MISMATCH).all() and frames.cpu().tolist() == [min(n, 3) for n in lens]
  s.reset([1] * case.B)   # the bit stays until a reset of the slot
  assert not s.read()[3].any()


def test_short_buffers_write_nothing(dev):
  from lipreading_amd import _C
  case, w, x, lens = setup("gru20_i7")
  s = C.Session(case, w, dev)
  before = s.state.clone()
  nws = s.L.lr_rnn_stream_workspace_bytes(s.mode, 1, case.T, case.I, case.H, 1, case.C)
  ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=dev)
  y = torch.full((1, case.T, case.H), float("nan"), device=dev)
  lp = torch.full((1, case.T, case.C), float("nan"), device=dev)
  xd = x.to(dev)
  for kw in (dict(state_bytes=s.state.numel() - 1), dict(pack_bytes=s.pack.numel() - 1), dict(ws_bytes=nws - 1)):
    assert s.advance_raw(xd, None, y, lp, ws, **kw) == _C.LR_ERR_WORKSPACE
  torch.cuda.synchronize()
  assert torch.equal(s.state, before) and torch.isnan(y).all() and torch.isnan(lp).all() and (ws == 0xFF).all()


def test_encoder_stream_names_the_slot(dev):
  from lipreading_amd import _C
  a, b = _encoder(dev, H=32).stream(2, dev), _encoder(dev, H=16).stream(2, dev)
  b.state_buf = a.state_buf                       # a session of another encoder let loose on this state
  b.feed(torch.zeros(2, 1, 204, device=dev))
  with pytest.raises(_C.LipReadingHipError, match="slot 0 has status"):
    a.state()
  a.reset()
  assert a.state().shape == (2, 2, 32)


# ---- 6: capture -----------------------------------------------------------------------------------------------------

def test_a_one_frame_advance_replays_as_a_linear_graph(dev):
  from lipreading_amd import _C
  case, w, x, lens = setup("gru20_i7")
  eager = C.Session(case, w, dev)
  want = [eager.feed(x[:, t:t + 1].to(dev), None) for t in range(5)]
  s = C.Session(case, w, dev)
  nws = s.L.lr_rnn_stream_workspace_bytes(s.mode, 1, 1, case.I, case.H, 1, case.C)
  ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=dev)
  xb = torch.zeros(1, 1, case.I, device=dev)
  y = torch.full((1, 1, case.H), float("nan"), device=dev)
  lp = torch.full((1, 1, case.C), float("nan"), device=dev)
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):                     # a warm-up outside the capture, then back to the empty state
    _C.check(s.advance_raw(xb, None, y, lp, ws), "warm-up")
  torch.cuda.current_stream().wait_stream(side)
  s.reset()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    _C.check(s.advance_raw(xb, None, y, lp, ws), "captured advance")
  for t in range(5):
    xb.copy_(x[:, t:t + 1])
    graph.replay()
    assert torch.equal(y, want[t][0]) and torch.equal(lp, want[t][1]), t
  assert torch.equal(s.state, eager.state)
