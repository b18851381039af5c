"""Transformer sessions on the MI355X (lr_tfm_stream_*, lipreading_amd/transformer_stream.py).

Every raw case runs through tests/tfm_stream_cases.Session: NaN-filled outputs, a 0xFF-filled workspace, guard words
either side of h_out, log_probs, the state and the workspace, ragged sizes per slot, NaN in the rows of a chunk no frame
was fed for.  The reference of every number is torch.nn on the CPU fed chunk by chunk from an explicit key / value cache
(stream_ref), which tests/test_tfm_stream_cpu.py pins to nn.TransformerEncoder under the chunk mask.

Against float64 (hold's rule of tests/test_gpu_transformer_fp64.py as it stands: element-wise, relative to the float64
tensor's largest entry, 4 x the error the float32 CPU run makes on the same case, never less than 4 ulp): the figures
are printed by the test; MEASURED below is what an MI355X gave.  No bound was tuned to it.

MEASURED (an MI355X; float32 CPU error, the bound = 4 x max(that, 1 ulp = 1.19e-7), the device's error):
  d64_t97_c5_l1 h                                cpu fp32 2.63e-07  bound 1.05e-06  device 2.10e-07
  d64_t97_c5_l1 lp                               cpu fp32 1.01e-07  bound 4.77e-07  device 6.99e-08
  d64_t97_c5_l1 log_probs of the zero row        cpu fp32 4.35e-08  bound 4.77e-07  device 4.35e-08
  d128_t96_c8_l3 h                               cpu fp32 2.44e-07  bound 9.74e-07  device 2.32e-07
  d128_t96_c8_l3 lp                              cpu fp32 9.54e-08  bound 4.77e-07  device 7.07e-08
  d128_t96_c8_l3 log_probs of the zero row       cpu fp32 5.74e-08  bound 4.77e-07  device 5.74e-08
  d64_t21_c1_l0 h                                cpu fp32 1.89e-07  bound 7.55e-07  device 2.29e-07
  d64_t21_c1_l0 lp                               cpu fp32 8.77e-08  bound 4.77e-07  device 6.15e-08
  d64_t21_c1_l0 log_probs of the zero row        cpu fp32 4.35e-08  bound 4.77e-07  device 4.35e-08
  d128_t21_c32_l1 h                              cpu fp32 1.99e-07  bound 7.95e-07  device 1.79e-07
  d128_t21_c32_l1 lp                             cpu fp32 9.22e-08  bound 4.77e-07  device 6.56e-08
  d128_t21_c32_l1 log_probs of the zero row      cpu fp32 5.74e-08  bound 4.77e-07  device 5.74e-08
  d64_t97_c32_l3_b17 h                           cpu fp32 2.43e-07  bound 9.74e-07  device 2.34e-07
  d64_t97_c32_l3_b17 lp                          cpu fp32 9.17e-08  bound 4.77e-07  device 7.14e-08
  d64_t97_c32_l3_b17 log_probs of the zero row   cpu fp32 4.35e-08  bound 4.77e-07  device 4.35e-08
The device lands at 0.7 .. 1.2 of the float32 CPU run's own error.
"""
import re

import pytest
import torch

from tests import tfm_stream_cases as S
from tests.test_gpu_transformer_fp64 import hold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


# name -> (model, T, C, Lc, lens)
CASES = {
    "d64_t97_c5_l1": ("d64", 97, 5, 1, [97, 1, 0, 93]),
    "d128_t96_c8_l3": ("d128", 96, 8, 3, [96, 1, 0, 91]),
    "d64_t21_c1_l0": ("d64", 21, 1, 0, [21, 1, 0, 19]),
    "d128_t21_c32_l1": ("d128", 21, 32, 1, [21, 1, 0, 18]),
    "d64_t97_c32_l3_b17": ("d64", 97, 32, 3, [97, 1, 0, 95, 33, 64, 65, 31, 96, 2, 50, 77, 12, 88, 40, 5, 71]),
}
_memo = {}


def setup(name, dev):
  """(ref (fp32, CPU), enc (device), x (B, T, I), lens), made once"""
  if name not in _memo:
    from lipreading_amd.data import default_char2idx
    from lipreading_amd.transformer import TransformerVideoEncoder
    model, T, C, Lc, lens = CASES[name]
    dm, nh = S.MODELS[model]
    ref = S.make_ref(S.FRAME_DIM, dm, nh, S.LAYERS, S.FF, seed=5).eval()
    enc = TransformerVideoEncoder(S.FRAME_DIM, dm, nh, S.LAYERS, S.FF, enable_ctc=True, vocab_size=S.VOCAB,
                                  char2idx=default_char2idx(), attn_chunk=C, attn_left_chunks=Lc)
    assert not enc.load_state_dict(S.state_for_encoder(ref)).missing_keys
    x = torch.randn(len(lens), T, S.FRAME_DIM, generator=torch.Generator().manual_seed(T + C))
    _memo[name] = (ref, enc.to(dev).eval(), x, lens)
  return _memo[name]


def advances(name, plan):
  """the batch plan `plan` (a name of S.plans, or 'mixed': slot b takes plan b mod 6) of the case"""
  _, T, C, Lc, lens = CASES[name]
  names = sorted(S.plans(1, C))
  per = []
  for b, n in enumerate(lens):
    p = S.plans(n, C)[names[b % len(names)] if plan == "mixed" else plan]
    per.append(p or [0])   # (no frames at all: one empty flush)
  return S.batch_plan(per)


def run(name, dev, plan):
  key = (name, plan)
  if key not in _memo:
    ref, enc, x, lens = setup(name, dev)
    _memo[key] = S.Session(enc, len(lens), dev).run(x, advances(name, plan))
  return _memo[key]


def cpu_ref(name, dev, dtype):
  key = (name, dtype)
  if key not in _memo:
    ref, _, x, lens = setup(name, dev)
    _, _, C, Lc, _ = CASES[name]
    import copy
    r = copy.deepcopy(ref).to(dtype)
    _memo[key] = [S.stream_ref(r, x[b, :n].to(dtype), [n], C, Lc) for b, n in enumerate(lens)]
  return _memo[key]


def same_bits(a, b, what):
  for k in ("h", "lp", "state"):
    for slot, (u, v) in enumerate(zip(a[k], b[k])):
      assert torch.equal(u, v), (what, k, slot)
  assert a["frames"] == b["frames"] and a["status"] == b["status"] == [0] * len(a["status"])


# ---- 1: against float64, and against the one-shot forward -----------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_session_matches_float64(dev, name):
  ref, enc, x, lens = setup(name, dev)
  got = run(name, dev, "mixed")
  r64, r32 = cpu_ref(name, dev, torch.float64), cpu_ref(name, dev, torch.float32)
  assert got["frames"] == lens
  for k, i in (("h", 1), ("lp", 0)):
    hold("%s %s" % (name, k), torch.cat(got[k]), torch.cat([r[i] for r in r64]), torch.cat([r[i] for r in r32]))
  if got["zero_row"] is not None:
    z = torch.zeros(1, enc.d_model)
    heads = []
    for dt in (torch.float64, torch.float32):
      logits = torch.nn.functional.linear(z.to(dt), ref.output_proj.weight.detach().to(dt),
                                          ref.output_proj.bias.detach().to(dt))
      heads.append(S.O.masked_log_softmax(logits, ref.output_mask.to(dt).expand_as(logits)))
    hold(name + " log_probs of the zero row", got["zero_row"].view(1, -1), heads[0], heads[1])


@pytest.mark.parametrize("name", list(CASES))
def test_session_matches_the_one_shot_forward(dev, name):
  """encoder.forward of the same chunk-masked model in its 'f32' modes, rows < len."""
  ref, enc, x, lens = setup(name, dev)
  assert enc.input_projection == 'f32' and enc.attention == 'f32'
  got = run(name, dev, "one")
  with torch.no_grad():
    lp, h, _ = enc(x.to(dev), torch.tensor(lens), max_len=x.shape[1])
  for b, n in enumerate(lens):
    torch.testing.assert_close(got["h"][b], h[b, :n].cpu(), rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(got["lp"][b], lp[b, :n].cpu(), rtol=2e-4, atol=2e-5)


# ---- 2: bit for bit under chunking ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_every_chunking_gives_the_same_bits_and_state_bytes(dev, name):
  one = run(name, dev, "one")
  plans = ("ragged", "boundaries", "inside", "several", "mixed") + (("frames",) if "b17" not in name else ())
  for plan in plans:
    same_bits(run(name, dev, plan), one, plan)


def test_frame_by_frame_at_the_largest_case(dev):
  name = "d64_t97_c32_l3_b17"
  same_bits(run(name, dev, "frames"), run(name, dev, "one"), "frames")


# ---- 3: slots are independent ---------------------------------------------------------------------------------------

def test_a_permuted_batch_gives_the_permuted_bits(dev):
  name = "d128_t96_c8_l3"
  ref, enc, x, lens = setup(name, dev)
  base = run(name, dev, "ragged")
  perm = [2, 0, 3, 1]
  _, T, C, Lc, _ = CASES[name]
  per = [S.plans(lens[p], C)["several"] or [0] for p in perm]
  got = S.Session(enc, 4, dev).run(x[perm], S.batch_plan(per))
  for i, p in enumerate(perm):
    for k in ("h", "lp", "state"):
      assert torch.equal(got[k][i], base[k][p]), (k, i)


def test_alone_equals_slot_16_of_17(dev):
  name = "d64_t97_c32_l3_b17"
  ref, enc, x, lens = setup(name, dev)
  base = run(name, dev, "one")
  n = lens[16]
  got = S.Session(enc, 1, dev).run(x[16:17], S.batch_plan([S.plans(n, 32)["ragged"]]))
  for k in ("h", "lp", "state"):
    assert torch.equal(got[k][0], base[k][16]), k


def test_a_masked_reset_restarts_only_its_slots(dev):
  name = "d64_t97_c5_l1"
  ref, enc, x, lens = setup(name, dev)
  base = run(name, dev, "one")
  s = S.Session(enc, 4, dev)
  first = [min(n, 13) for n in lens]
  s.feed(x, first)
  before = [s.slot_bytes(b) for b in range(4)]
  mask = [1, 0, 0, 1]
  s.reset(mask)
  fresh = S.Session(enc, 4, dev)
  for b in range(4):
    assert torch.equal(s.slot_bytes(b), fresh.slot_bytes(b) if mask[b] else before[b])
  assert s.read()[0] == [0, first[1], first[2], 0]
  # the reset slots from their first frame, the others go on: everybody ends where a fresh session ends
  h, lp, cn = s.feed(x, [lens[b] - s.fed[b] for b in range(4)], [1, 1, 1, 1])
  for b in (0, 3):
    assert torch.equal(h[b], base["h"][b]) and torch.equal(lp[b], base["lp"][b])
  for b in range(4):
    assert torch.equal(s.slot_bytes(b), base["state"][b])


# ---- 4: counts, end, flush ------------------------------------------------------------------------------------------

def test_counts_end_and_flush(dev):
  name = "d64_t97_c5_l1"
  ref, enc, x, lens = setup(name, dev)
  base = run(name, dev, "one")
  s = S.Session(enc, 4, dev)
  assert s.feed(x, [7, 1, 0, 4])[2] == [5, 0, 0, 0]                    # E = (n // 5) * 5
  assert s.feed(x, [3, 0, 0, 0], T=6)[2] == [5, 0, 0, 0]               # sizes below chunk_T; idle slots
  assert s.feed(x, [13, 0, 0, 17])[2] == [10, 0, 0, 20]                # several chunks in one advance
  idle = s.slot_bytes(2)
  assert s.feed(x, [0, 0, 0, 0], [0, 1, 0, 0], T=0)[2] == [0, 1, 0, 0]   # t = 0 with end: a flush of the short chunk
  assert torch.equal(s.slot_bytes(2), idle)                            # idle: every bit stays
  assert s.feed(x, [0, 0, 0, 0], [0, 0, 1, 0], T=0)[2] == [0, 0, 0, 0]   # a flush of nothing ends the slot
  assert s.read()[2] == [0, 1, 1, 0] and s.read()[1] == [20, 1, 0, 20]
  h, lp, cn = s.feed(x, [lens[0] - 23, 0, 0, lens[3] - 21], [1, 0, 0, 1])
  assert cn == [lens[0] - 20, 0, 0, lens[3] - 20] and s.read()[2] == [1, 1, 1, 1]
  assert torch.equal(h[0], base["h"][0][20:]) and torch.equal(lp[3], base["lp"][3][20:])
  for b in range(4):
    assert torch.equal(s.slot_bytes(b), base["state"][b])


# ---- 5: traps -------------------------------------------------------------------------------------------------------

def _status_word(slot):
  return slot[:64].view(torch.int32)[11:12]


def _trap(s, x, dev, sizes, end=None, **kw):
  """one raw advance of 2 frames -> (status words after, counts); asserts that only the status words changed"""
  from lipreading_amd import _C
  B = s.B
  before = [s.slot_bytes(b) for b in range(B)]
  rows = 2 + s.C - 1
  h = torch.full((B, rows, s.Dm), float("nan"), device=dev)
  lp = torch.full((B, rows, s.Cv), float("nan"), device=dev)
  counts = torch.full((B,), -7, dtype=torch.int32, device=dev)
  _, ws = s.workspace(2)
  xd = x[:, :2].contiguous().to(dev)
  _C.check(s.advance_raw(xd, s._i32(sizes), s._i32(end), h, lp, counts, ws, **kw), "advance")
  torch.cuda.synchronize()
  words = []
  for b in range(B):
    after = s.slot_bytes(b)
    words.append(int(_status_word(after)))
    _status_word(after).copy_(_status_word(before[b]))
    assert torch.equal(after, before[b]), b
  return words, counts.cpu().tolist()


def test_the_status_bits_leave_the_slot_alone(dev):
  from lipreading_amd import _C
  name = "d64_t97_c5_l1"
  ref, enc, x, lens = setup(name, dev)
  s = S.Session(enc, 4, dev)
  s.feed(x, [7, 1, 3, 7], [0, 1, 0, 0])
  MIS, AFT, FULL = _C.LR_TFM_STREAM_MISMATCH, _C.LR_TFM_STREAM_AFTER_END, _C.LR_TFM_STREAM_FULL
  # frames after the end: slot 1 alone; slot 2 is idle and stays clean
  assert _trap(s, x, dev, [0, 2, 0, 0]) == ([0, AFT, 0, 0], [0, 0, 0, 0])
  # the positional table ends: slots 0 and 3 would pass 8 rows; slot 1 is idle now, its bit stays
  assert _trap(s, x, dev, [2, 0, 0, 2], pe_rows=8)[0] == [FULL, AFT, 0, FULL]
  assert s.read()[3] == [FULL, AFT, 0, FULL] and s.read()[0] == [7, 1, 3, 7]
  # another configuration (2 heads of 32: the same layout, other arithmetic): every slot that is not idle
  other = S.Session(enc, 4, dev)
  other.feed(x, [7, 1, 3, 4])
  assert _trap(other, x, dev, [2, 0, 2, 2], nhead=2)[0] == [MIS, 0, MIS, MIS]
  assert other.read()[3] == [MIS, 0, MIS, MIS]
  other.reset([1, 0, 0, 0])                          # the bit stays until a reset of the slot
  assert other.read()[3] == [0, 0, MIS, MIS]


def test_check_names_the_slot(dev):
  from lipreading_amd import _C
  ref, enc, x, lens = setup("d64_t97_c5_l1", dev)
  st = enc.stream(3, dev)
  xd = x[:3].to(dev)
  st.feed(xd[:, :4], end=torch.tensor([0, 1, 0], device=dev))
  st.check()
  st.feed(xd[:, 4:6], sizes=torch.tensor([2, 2, 0], device=dev))
  with pytest.raises(_C.LipReadingHipError, match=r"slot 1 has status 2 \(frames were fed after"):
    st.check()
  st.reset(torch.tensor([0, 1, 0], device=dev))
  assert st.check().frames().cpu().tolist() == [6, 0, 4]
  st.feed(xd[:, :2], sizes=torch.tensor([0, 0, 2], device=dev))
  big = torch.zeros(3, 600, S.FRAME_DIM, device=dev)
  st.feed(big, sizes=torch.tensor([0, 0, 600], device=dev))
  with pytest.raises(_C.LipReadingHipError, match=r"slot 2 has status 4 \(full"):
    st.check()


def test_short_buffers_and_nulls_write_nothing(dev):
  from lipreading_amd import _C
  ref, enc, x, lens = setup("d64_t97_c5_l1", dev)
  s = S.Session(enc, 4, dev)
  s.feed(x, [7, 1, 3, 4])
  before = s.state.clone()
  rows = 2 + s.C - 1
  h = torch.full((4, rows, s.Dm), float("nan"), device=dev)
  lp = torch.full((4, rows, s.Cv), float("nan"), device=dev)
  counts = torch.full((4,), -7, dtype=torch.int32, device=dev)
  _, ws = s.workspace(2)
  xd = x[:, :2].contiguous().to(dev)
  W, A, U = _C.LR_ERR_WORKSPACE, _C.LR_ERR_INVALID_ARG, _C.LR_ERR_UNSUPPORTED
  for want, kw in ((W, dict(state_bytes=s.nstate - 1)), (W, dict(ws_bytes=ws.numel() - 1)), (A, dict(state=None)),
                   (A, dict(ws=None)), (A, dict(counts=None)), (A, dict(x=None)), (A, dict(pe=None)), (A, dict(weights=None)),
                   (A, dict(hw=None)), (A, dict(lp=None)), (A, dict(state=s.state.data_ptr() + 4)),
                   (A, dict(ws=ws.data_ptr() + 8)), (A, dict(C=0)), (A, dict(Lc=-1)), (A, dict(B=0)), (A, dict(pe_rows=0)),
                   (U, dict(C=33)), (U, dict(C=32, Lc=4)), (U, dict(nhead=3))):
    assert s.advance_raw(xd, None, None, h, lp, counts, ws, **kw) == want, kw
  L = s.L
  assert L.lr_tfm_stream_state_bytes(4, s.I, s.Dm, s.nhead, s.F, s.layers, 33, 0) == 0
  assert L.lr_tfm_stream_state_bytes(4, s.I, s.Dm, s.nhead, s.F, s.layers, 32, 4) == 0
  assert L.lr_tfm_stream_state_bytes(4, s.I, 256, 2, s.F, s.layers, 8, 1) == 0           # head dimension 128 > 64
  assert L.lr_tfm_stream_state_bytes(4, s.I, 256, 4, s.F, s.layers, 8, 1) > 0
  assert L.lr_tfm_stream_workspace_bytes(4, 2, s.I, s.Dm, s.nhead, s.F, s.layers, s.Cv, 0, 0) == 0
  assert L.lr_tfm_stream_reset(s.state.data_ptr(), s.nstate - 1, None, 4, *s.cfg, _C.stream_handle()) == W
  assert L.lr_tfm_stream_reset(None, s.nstate, None, 4, *s.cfg, _C.stream_handle()) == A
  meta = torch.full((4,), -9, dtype=torch.int32, device=dev)
  assert L.lr_tfm_stream_read(s.state.data_ptr(), s.nstate - 1, meta.data_ptr(), None, None, None, 4, *s.cfg,
                              _C.stream_handle()) == W
  assert L.lr_tfm_stream_read(s.state.data_ptr(), s.nstate, None, None, None, None, 4, *s.cfg, _C.stream_handle()) == A
  torch.cuda.synchronize()
  s.check_guards()
  assert torch.equal(s.state, before) and torch.isnan(h).all() and torch.isnan(lp).all() and (ws == 0xFF).all()
  assert (counts == -7).all() and (meta == -9).all()


# ---- 6: the Python front doors --------------------------------------------------------------------------------------

def test_strided_views_go_in_without_a_copy(dev):
  ref, enc, x, lens = setup("d128_t96_c8_l3", dev)
  frames = x[:3].to(dev)
  a, b = enc.stream(3, dev), enc.stream(3, dev)
  for t0, t1 in ((0, 7), (7, 8), (8, 40), (40, 96)):
    view = frames[:, t0:t1]
    assert not view.is_contiguous() and a._frames_3d(view).data_ptr() == view.data_ptr()
    end = torch.full((3,), int(t1 == 96), device=dev)
    lp_v, h_v, c_v = a.feed(view, end=end, need_hidden=True)
    lp_c, h_c, c_c = b.feed(view.contiguous(), end=end, need_hidden=True)
    assert torch.equal(lp_v, lp_c) and torch.equal(h_v, h_c) and torch.equal(c_v, c_c)
  assert torch.equal(a.state_buf, b.state_buf) and a.frames().cpu().tolist() == [96, 96, 96]
  assert a.read()[1].cpu().tolist() == [96, 96, 96] and a.check() is a


def _char2idx():
  from lipreading_amd.data import BOS, EOS, PAD
  c2i = {PAD: 0, BOS: 1, EOS: 2}
  for ch in " abcdefgh":
    c2i[ch] = len(c2i)
  return c2i


def _encoder(dev, frame_dim=204, C=4, Lc=2):
  from lipreading_amd.transformer import TransformerVideoEncoder
  torch.manual_seed(11)
  c2i = _char2idx()
  return TransformerVideoEncoder(frame_dim, d_model=64, nhead=4, num_layers=2, dim_feedforward=128, enable_ctc=True,
                                 vocab_size=len(c2i), char2idx=c2i, attn_chunk=C, attn_left_chunks=Lc).to(dev).eval()


def test_chunked_encoder_has_the_forward_contract_and_goes_through_ctc_cer(dev):
  from lipreading_amd import train as T
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.transformer_stream import ChunkedTransformerEncoder
  enc = _encoder(dev)
  c2i = _char2idx()
  dec = BeamCTCDecoder(ctc_labels(c2i), beam_width=8, log_probs_input=True)
  g = torch.Generator().manual_seed(6)
  frames = torch.randn(3, 14, 68, 3, generator=g)
  frame_lens = torch.tensor([14, 9, 12])
  chars = torch.tensor([[1, 4, 5, 2], [1, 6, 2, 0], [1, 7, 8, 2]])
  char_lens = torch.tensor([4, 3, 4])
  loader = [(frames, frame_lens, chars, char_lens)]
  chunked = ChunkedTransformerEncoder(enc, 5)
  lp, hidden, state = chunked(frames.to(dev), frame_lens.to(dev), max_len=14)
  assert lp.shape == (3, 14, len(c2i) + 1) and hidden.shape == (3, 14, 64) and state is None
  lp1, hidden1, _ = ChunkedTransformerEncoder(enc, 14)(frames.to(dev), frame_lens.to(dev), max_len=14)
  assert torch.equal(lp, lp1) and torch.equal(hidden, hidden1)       # the pieces change no bit
  with torch.no_grad():
    want = enc(frames.to(dev), frame_lens.to(dev), max_len=14)
  for b, n in enumerate(frame_lens.tolist()):
    torch.testing.assert_close(lp[b, :n], want[0][b, :n], rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(hidden[b, :n], want[1][b, :n], rtol=2e-4, atol=2e-5)
    assert not hidden[b, n:].any()
  cer = T.ctc_cer(chunked, loader, dev, c2i, dec)
  assert 0.0 <= cer and cer == T.ctc_cer(ChunkedTransformerEncoder(enc, 14), loader, dev, c2i, dec)


def test_live_transcriber_equals_the_one_shot_search(dev):
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.transformer_stream import ChunkedTransformerEncoder, TransformerLiveTranscriber
  enc = _encoder(dev)
  dec = BeamCTCDecoder(ctc_labels(_char2idx()), beam_width=8, log_probs_input=True)
  g = torch.Generator().manual_seed(4)
  frames = torch.randn(3, 23, 204, generator=g).to(dev)
  lens = torch.tensor([23, 11, 17], dtype=torch.int32, device=dev)
  lp = ChunkedTransformerEncoder(enc, 23)(frames, lens, max_len=23)[0]
  want, want_off = dec.decode(lp, lens)
  live = TransformerLiveTranscriber(enc, dec, 3, 23, dev)
  for t0 in range(0, 23, 5):
    t1 = min(23, t0 + 5)
    live.feed(frames[:, t0:t1], (lens - t0).clamp(0, t1 - t0), ((lens > t0) & (lens <= t1)).int())
  got, got_off = live.check().result()
  assert got == want and [[o.tolist() for o in r] for r in got_off] == [[o.tolist() for o in r] for r in want_off]
  assert [p[0] for p in live.partial()] == [s[0] for s in want]
  live.reset(torch.tensor([0, 1, 0], device=dev))
  live.feed(frames[1:2].expand(3, -1, -1), torch.tensor([0, 11, 0], dtype=torch.int32, device=dev),
            torch.tensor([0, 1, 0], dtype=torch.int32, device=dev))
  assert live.result()[0] == want


def test_live_transcriber_behind_a_frontend_stream(dev):
  """pixels in, transcript out at H = W = 32: FrontendStream -> TransformerStream -> BeamStream against the one-shot
  search on ChunkedTransformerEncoder's log-probs of ChunkedFrontend's features, string for string."""
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.frontend import ConvFrontend3D, PixelLipReader, feature_dim
  from lipreading_amd.frontend_stream import ChunkedFrontend
  from lipreading_amd.transformer_stream import (ChunkedTransformerEncoder, ChunkedTransformerPixelLipReader,
                                                 TransformerLiveTranscriber)
  torch.manual_seed(12)
  model = PixelLipReader(_encoder(dev, frame_dim=feature_dim(32, 32)), ConvFrontend3D()).to(dev).eval()
  dec = BeamCTCDecoder(ctc_labels(_char2idx()), beam_width=8, log_probs_input=True)
  g = torch.Generator().manual_seed(8)
  clips = torch.randint(0, 256, (2, 19, 3, 32, 32), generator=g, dtype=torch.uint8).to(dev)
  lens = torch.tensor([19, 12], dtype=torch.int32, device=dev)
  feats = ChunkedFrontend(model.frontend, 19)(clips, lens, max_len=19)
  lp = ChunkedTransformerEncoder(model.encoder, 19)(feats, lens, max_len=19)[0]
  both = ChunkedTransformerPixelLipReader(model, 6)(clips, lens, max_len=19)
  assert torch.equal(both[0], lp)
  want = dec.decode(lp, lens)[0]
  live = TransformerLiveTranscriber(model, dec, 2, 19, dev, height=32, width=32)
  for t0 in range(0, 19, 4):
    t1 = min(19, t0 + 4)
    live.feed(clips[:, t0:t1], (lens - t0).clamp(0, t1 - t0), ((lens > t0) & (lens <= t1)).int())
  assert live.check().result()[0] == want
  assert live.encoder_stream.frames().cpu().tolist() == [19, 12]


def test_driver_streams_the_transformer(dev, tmp_path, capsys):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=6, captions_per_video=4, seed=7)
  common = ["--root=" + root, "--data=synth/micro", "--batch_size=8", "--encoder=transformer", "--hidden_size=64",
            "--num_layers=2", "--max_epochs=0", "--ctc_decoder=beam", "--beam_width=8", "--stream_chunk=5",
            "--tfm_chunk=4", "--tfm_left_chunks=2"]
  cers = []
  for extra in ([], ["--stream_tfm=True"]):
    capsys.readouterr()
    out = driver.run(**driver.parse_flags(common + extra))
    text = capsys.readouterr().out
    assert bool(re.search(r"Commit delay \(chunks of 5 frames\): .*\(encoder streamed: adds up to 3 frames", text)) == \
        bool(extra), text
    cers.append(float(re.search(r"\tCER:\s+(\S+)", text).group(1)))
    assert "commit_delay" in out
  assert 0.0 <= cers[1] and abs(cers[0] - cers[1]) <= 0.05   # (an untrained model: near-ties may fall either way)
