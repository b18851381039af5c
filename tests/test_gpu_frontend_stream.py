"""Conv frontend sessions on the MI355X (lr_conv_stream_*).

1  exact-integer cases: a session's features == the fp64 reference == ConvFrontend3D.forward on each slot's clip alone,
   under every chunking, with `==`
2  real-valued clips (uint8 and fp32) against the bf16-emulating CPU oracle, within the bound the one-shot forward holds
3  bit equality of features AND state bytes across chunkings, ragged feeds with idle calls, where `end` is given, runs,
   reads between feeds, slot permutations, batch sizes, strided views
4  masked reset; AFTER_END / MISMATCH leave the slot alone and raise through FrontendStream; the ABI's LR_ERR_* traps
5  a one-frame advance captured and replayed as a linear graph
6  compositions: ChunkedFrontend, PixelLiveTranscriber, ChunkedPixelLipReader, the driver's --stream_frontend

Figures of test 6 (max |log-prob error| against the CPU oracle: conv_frontend -> float64 GRU -> masked log-softmax;
uni GRU-32 on two unpadded 16 x 16 clips of 8 frames), measured on an MI355X:
  PixelLiveTranscriber 6.774e-06, PixelLipReader.forward 6.774e-06, PixelLipReader.forward on the second seed 7.931e-06
  (all three are the masked classes' constant, log(1e-45)); over the unmasked classes alone: session 4.2e-07, one-shot
  2.0e-06 (second seed: 4.4e-07, 6.1e-07).  ChunkedPixelLipReader, full look-ahead, BiGRU-32: 9.557e-06 against the
  one-shot model's 9.557e-06 (second seed 1.467e-05).  Real clips against the oracle: rel_err 0 to 1.1e-03 (bound 2e-2).
"""
import re

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests import frontend_stream_cases as C

pytestmark = pytest.mark.gpu

U8, F32, I32 = torch.uint8, torch.float32, torch.int32


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def rel_err(a, b):   # tests/test_gpu_frontend.py's
  return float(np.abs(a - b).max() / max(1e-6, np.abs(b).max()))


def frontend(dev, ws=None, bs=None, seed=3):
  from lipreading_amd.frontend import ConvFrontend3D
  torch.manual_seed(seed)
  fe = ConvFrontend3D()
  if ws is not None:
    with torch.no_grad():
      for p, v in zip(fe.parameters_in_order(), [t for pair in zip(ws, bs) for t in pair]):
        p.copy_(v.float())
  return fe.to(dev).eval()


def ivec(v, dev):
  return torch.tensor(list(v), dtype=I32, device=dev)


def run(st, clips, calls, read_between=False, contiguous=False):
  """Feeds `calls` (C.Call) from clips (B, T, 3, H, W) on the device; returns per slot the features it emitted and per
  call the counts.  Rows at and past counts[b] must be zero."""
  B = st.batch
  feats, counts = [[] for _ in range(B)], []
  for c in calls:
    x = clips[:, c.t0:c.t0 + c.chunk]
    if contiguous:
      x = x.contiguous()
    end = ivec(c.end, clips.device) if any(c.end) else None
    f, n = st.feed(x, ivec(c.sizes, clips.device), end)
    assert f.shape == (B, x.shape[1] + (3 if end is not None else 0), st.F) and f.dtype == F32
    n = n.cpu().tolist()
    for b in range(B):
      feats[b].append(f[b, :n[b]])
      assert not f[b, n[b]:].any(), (c, b)
    counts.append(n)
    if read_between:
      st.read()
  return [torch.cat(f) for f in feats], counts


def expected_counts(lens, calls):
  fed, ended, out = [0] * len(lens), [False] * len(lens), []
  for c in calls:
    row = []
    for b in range(len(lens)):
      before = C.emitted(fed[b], ended[b])
      fed[b] += c.sizes[b]
      ended[b] = ended[b] or bool(c.end[b])
      row.append(C.emitted(fed[b], ended[b]) - before)
    out.append(row)
  return out


_memo = {}


def exact(name, dev):
  """(problem, frontend on the device, clips on the device), made once"""
  if name not in _memo:
    p = C.problem(name)
    _memo[name] = (p, frontend(dev, p.ws, p.bs), p.clip.to(dev))
  return _memo[name]


# ---- 1: exact integers ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.BY_NAME))
def test_exact_cases_equal_fp64_the_one_shot_forward_and_every_chunking(dev, name):
  p, fe, clips = exact(name, dev)
  lens, T = p.case.lens, max(p.case.lens)
  B = len(lens)
  with torch.no_grad():
    one_shot = [fe(clips[b:b + 1, :n])[0] for b, n in enumerate(lens)]
  ref, ref_counts = C.stream_ref(p.x, lens, p.ws, p.bs, C.schedule(lens, [2] * ((T + 1) // 2), False))
  assert sum(ref_counts, []) and all(sum(r[b] for r in ref_counts) == lens[b] for b in range(B))
  for b in range(B):
    C.compare_exact(one_shot[b], p.features[b], "%s one-shot slot %d" % (name, b), axes=("frame", "feature"))
    C.compare_exact(ref[b], p.features[b], "%s stream_ref slot %d" % (name, b), axes=("frame", "feature"))
  st = fe.stream(B, p.case.H, p.case.W, dev)
  for chunking in C.chunkings(T):
    for end_with in (True, False):
      calls = C.schedule(lens, chunking, end_with)
      got, counts = run(st.reset(), clips, calls)
      assert counts == expected_counts(lens, calls), (chunking, end_with)
      for b in range(B):
        what = "%s slot %d, chunks %s, end %s" % (name, b, chunking, "with" if end_with else "after")
        C.compare_exact(got[b], p.features[b], what, axes=("frame", "feature"))
        assert torch.equal(got[b], one_shot[b]), what
      n, emitted, ended, status = (t.cpu().tolist() for t in st.read())
      assert n == list(lens) and emitted == list(lens) and all(ended) and not any(status)


def test_exact_fp32_clips_equal_the_uint8_ones(dev):
  p, fe, clips = exact("r16x32", dev)
  lens = p.case.lens
  st = fe.stream(len(lens), p.case.H, p.case.W, dev)
  got, _ = run(st, (clips // 255).float(), C.schedule(lens, [2, 2, 1], True))
  for b in range(len(lens)):
    C.compare_exact(got[b], p.features[b], "fp32 clip slot %d" % b, axes=("frame", "feature"))


# ---- 2: real values against the oracle --------------------------------------------------------------------------------

def real_problem(dev, B, T, H, W, dtype, seed=5):
  key = ("real", B, T, H, W, dtype, seed)
  if key not in _memo:
    fe = frontend(dev, seed=seed)
    g = torch.Generator().manual_seed(seed)
    clips = torch.randint(0, 256, (B, T, 3, H, W), generator=g, dtype=U8)
    if dtype == F32:
      clips = torch.rand((B, T, 3, H, W), generator=g)
    _memo[key] = (fe, clips, clips.to(dev))
  return _memo[key]


@pytest.mark.parametrize("dtype", [U8, F32])
def test_real_clips_match_the_oracle(dev, dtype):
  B, T, H = 2, 6, 32
  fe, clips, clips_d = real_problem(dev, B, T, H, H, dtype)
  lens = (6, 4)
  params = [p.detach().cpu() for p in fe.parameters_in_order()]
  st = fe.stream(B, H, H, dev)
  got, _ = run(st, clips_d, C.schedule(lens, [2, 3, 1], True))
  for b, n in enumerate(lens):
    want = O.conv_frontend(clips[b:b + 1, :n], params)[0].numpy()
    err = rel_err(got[b].cpu().numpy(), want)
    print("slot %d (%s): rel_err %.3e" % (b, dtype, err))
    assert want.any() and err < 2e-2, (b, err)


# ---- 3: the same bits, the same state bytes ------------------------------------------------------------------------------

LENS9 = (9, 5, 9, 7, 2)


def bits_problem(dev):
  return real_problem(dev, 5, 9, 16, 16, U8, seed=7)


def base_run(dev):
  if "base9" not in _memo:
    fe, _, clips = bits_problem(dev)
    st = fe.stream(5, 16, 16, dev)
    feats, _ = run(st, clips, C.schedule(LENS9, [9], True))
    _memo["base9"] = (feats, st.state_buf.clone())
  return _memo["base9"]


def test_every_chunking_gives_the_same_bits_and_the_same_state(dev):
  fe, _, clips = bits_problem(dev)
  base, base_state = base_run(dev)
  assert all(f.shape[0] == n and f.any() for f, n in zip(base, LENS9))
  st = fe.stream(5, 16, 16, dev)
  for chunking in ([9], [1] * 9, [2, 3, 4], [4, 1, 1, 3]):
    for end_with in (True, False):
      for kw in (dict(), dict(read_between=True), dict(contiguous=True)):
        got, _ = run(st.reset(), clips, C.schedule(LENS9, chunking, end_with), **kw)
        for b in range(5):
          assert torch.equal(got[b], base[b]), (chunking, end_with, kw, b)
        assert torch.equal(st.state_buf, base_state), (chunking, end_with, kw)
  again = fe.stream(5, 16, 16, dev)                     # a second session, a second run
  got, _ = run(again, clips, C.schedule(LENS9, [4, 1, 1, 3], False))
  assert all(torch.equal(a, b) for a, b in zip(got, base)) and torch.equal(again.state_buf, base_state)


def test_state_bytes_after_the_same_frames_do_not_depend_on_the_cut(dev):
  """... in the middle of the clips too: 6 frames of every slot, not ended."""
  fe, _, clips = bits_problem(dev)
  states, feats = [], []
  for chunking in ([6], [1] * 6, [2, 4], [5, 1]):
    st = fe.stream(5, 16, 16, dev)
    t0, out = 0, []
    for n in chunking:
      f, c = st.feed(clips[:, t0:t0 + n])
      out.append([f[b, :c[b]] for b in range(5)])
      t0 += n
    states.append(st.state_buf.clone())
    feats.append([torch.cat([o[b] for o in out]) for b in range(5)])
    assert st.read()[1].cpu().tolist() == [3] * 5
  for s, f in zip(states[1:], feats[1:]):
    assert torch.equal(s, states[0]) and all(torch.equal(a, b) for a, b in zip(f, feats[0]))


def test_ragged_feeds_with_idle_calls(dev):
  """Every slot at its own pace: a call hands slot b `size` frames from its own offset, staged at the front of a chunk
  filled with another byte; idle slots get size 0; ends come with the last frames or in an idle call."""
  fe, _, clips = bits_problem(dev)
  base, base_state = base_run(dev)
  plan = [  # per call: (size, end) per slot
      [(3, 0), (0, 0), (1, 0), (4, 0), (2, 0)],
      [(0, 0), (5, 1), (2, 0), (0, 0), (0, 1)],
      [(4, 0), (0, 0), (0, 0), (3, 1), (0, 0)],
      [(2, 1), (0, 0), (6, 0), (0, 0), (0, 0)],
      [(0, 0), (0, 0), (0, 1), (0, 0), (0, 0)]]
  st = fe.stream(5, 16, 16, dev)
  off, feats = [0] * 5, [[] for _ in range(5)]
  for call in plan:
    chunk = max(s for s, _ in call)
    x = torch.full((5, chunk, 3, 16, 16), 0xAB, dtype=U8, device=dev)
    for b, (s, _) in enumerate(call):
      x[b, :s] = clips[b, off[b]:off[b] + s]
      off[b] += s
    f, n = st.feed(x, ivec([s for s, _ in call], dev), ivec([e for _, e in call], dev))
    for b in range(5):
      feats[b].append(f[b, :n[b]])
      assert not f[b, n[b]:].any()
  assert off == list(LENS9)
  for b in range(5):
    assert torch.equal(torch.cat(feats[b]), base[b]), b
  assert torch.equal(st.state_buf, base_state)


def test_slots_are_independent(dev):
  fe, _, clips = bits_problem(dev)
  base, _ = base_run(dev)
  perm = [3, 0, 4, 2, 1]
  st = fe.stream(5, 16, 16, dev)
  got, _ = run(st, clips[perm], C.schedule([LENS9[p] for p in perm], [2, 3, 4], True))
  for i, p in enumerate(perm):
    assert torch.equal(got[i], base[p]), (i, p)
  alone = fe.stream(1, 16, 16, dev)                        # B = 1 against slot 3 of 5
  got, _ = run(alone, clips[3:4], C.schedule(LENS9[3:4], [4, 1, 1, 3], False))
  assert torch.equal(got[0], base[3])


def test_strided_views_go_in_without_a_copy(dev):
  fe, _, clips = bits_problem(dev)
  a, b = fe.stream(5, 16, 16, dev), fe.stream(5, 16, 16, dev)
  wide = torch.zeros((5, 9, 3, 16, 24), dtype=U8, device=dev)   # rows of another pitch: this one is copied
  wide[..., :16] = clips
  for t0, t1 in ((0, 4), (4, 5), (5, 9)):
    view = clips[:, t0:t1]
    assert not view.is_contiguous() and a._clips_5d(view).data_ptr() == view.data_ptr()
    assert a._clips_5d(wide[:, t0:t1, :, :, :16]).is_contiguous()
    fv, cv = a.feed(view)
    fc, cc = b.feed(wide[:, t0:t1, :, :, :16])
    assert torch.equal(fv, fc) and torch.equal(cv, cc)
  assert torch.equal(a.state_buf, b.state_buf) and a.frames().cpu().tolist() == [9] * 5


# ---- 4: reset, status bits, traps ---------------------------------------------------------------------------------------

def hdr_words(state, B):
  return state[:32 * B].view(I32).view(B, 8)


def test_a_masked_reset_restarts_only_its_slots(dev):
  fe, _, clips = bits_problem(dev)
  base, base_state = base_run(dev)
  st = fe.stream(5, 16, 16, dev)
  st.feed(clips[:, :5], ivec([min(n, 5) for n in LENS9], dev))
  before = st.state_buf.clone()
  mask = [1, 0, 0, 1, 1]
  st.reset(ivec(mask, dev))
  n, emitted, ended, status = (t.cpu().tolist() for t in st.read())
  assert n == [0, 5, 5, 0, 0] and emitted == [0, 2, 2, 0, 0] and not any(ended) and not any(status)
  fresh = fe.stream(5, 16, 16, dev).state_buf
  L = st.state_buf.numel() - 256
  per = L // 5
  for b in range(5):
    lo, hi = 256 + b * per, 256 + (b + 1) * per
    want = fresh if mask[b] else before
    assert torch.equal(st.state_buf[lo:hi], want[lo:hi]), b
    assert torch.equal(hdr_words(st.state_buf, 5)[b], hdr_words(want, 5)[b]), b
  # the reset slots from their first frame, the others go on: everybody ends where a fresh session ends
  x = torch.full((5, 9, 3, 16, 16), 0xAB, dtype=U8, device=dev)
  sizes = []
  for b, n in enumerate(LENS9):
    lo = 0 if mask[b] else min(n, 5)
    x[b, :n - lo] = clips[b, lo:n]
    sizes.append(n - lo)
  f, c = st.feed(x, ivec(sizes, dev), ivec([1] * 5, dev))
  for b in range(5):
    want = base[b] if mask[b] else base[b][C.emitted(min(LENS9[b], 5), False):]
    assert torch.equal(f[b, :c[b]], want), b
  assert torch.equal(st.state_buf, base_state)


def test_frames_after_the_end_and_another_size_leave_the_slot_alone_and_raise(dev):
  from lipreading_amd import _C
  fe, _, clips = bits_problem(dev)
  st = fe.stream(5, 16, 16, dev)
  st.feed(clips[:, :4], None, ivec([0, 1, 0, 0, 0], dev))       # slot 1 ends after 4 frames
  before = st.state_buf.clone()
  f, c = st.feed(clips[:, 4:6], ivec([0, 2, 0, 0, 0], dev))     # ... and is given two more
  assert c.cpu().tolist() == [0] * 5 and not f.any()
  after = st.state_buf.clone()
  assert hdr_words(after, 5)[:, 6].cpu().tolist() == [0, _C.LR_CONV_STREAM_AFTER_END, 0, 0, 0]
  hdr_words(after, 5)[:, 6].zero_()
  assert torch.equal(after, before)
  with pytest.raises(_C.LipReadingHipError, match="slot 1 has status 2"):
    st.check()
  st.feed(clips[:, 4:6], ivec([0, 0, 1, 0, 0], dev), ivec([0, 1, 0, 0, 0], dev))   # ending again, idle: nothing
  assert st.read()[3].cpu().tolist() == [0, 2, 0, 0, 0]                               # the bit stays until a reset
  st.reset(ivec([0, 1, 0, 0, 0], dev))
  assert st.check().read()[0].cpu().tolist() == [4, 0, 5, 4, 4]
  # a session of another size let loose on this state: 32 x 16 over slots that carry 16 x 16
  big = fe.stream(2, 32, 16, dev)
  small = fe.stream(2, 16, 16, dev)
  n = small.state_buf.numel()
  big.state_buf[:n] = small.state_buf
  before = big.state_buf.clone()
  f, c = big.feed(torch.zeros((2, 2, 3, 32, 16), dtype=U8, device=dev), ivec([2, 0], dev))
  assert c.cpu().tolist() == [0, 0] and not f.any()
  after = big.state_buf.clone()
  assert hdr_words(after, 2)[:, 6].cpu().tolist() == [_C.LR_CONV_STREAM_MISMATCH, 0]      # the idle slot keeps every bit
  hdr_words(after, 2)[:, 6].zero_()
  assert torch.equal(after, before)
  with pytest.raises(_C.LipReadingHipError, match="slot 0 has status"):
    big.check()
  assert big.read()[3].cpu().tolist() == [_C.LR_CONV_STREAM_MISMATCH] * 2                 # read: neither slot is 32 x 16
  big.reset(ivec([1, 1], dev))          # a masked reset needs the slot's own size as well
  assert big.read()[3].cpu().tolist() == [_C.LR_CONV_STREAM_MISMATCH] * 2
  big.reset()
  assert big.check().frames().cpu().tolist() == [0, 0]


def advance_raw(session, clip, sizes_t, end_t, feat_t, counts_t, ws_t, **kw):
  from lipreading_amd import _C
  s = session
  a = dict(x=clip.data_ptr(), flags=_C.LR_CONV_STREAM_F32 if clip.dtype == F32 else 0, sb=clip.stride(0),
           st=clip.stride(1), sizes=_C.ptr(sizes_t), end=_C.ptr(end_t), w1=s._w[0].data_ptr(), w2=s._w[1].data_ptr(),
           w3=s._w[2].data_ptr(), b1=s._bias[0].data_ptr(), b2=s._bias[1].data_ptr(), b3=s._bias[2].data_ptr(),
           feat=_C.ptr(feat_t), counts=_C.ptr(counts_t), state=s.state_buf.data_ptr(), nstate=s.state_buf.numel(),
           ws=ws_t.data_ptr(), nws=ws_t.numel(), B=s.batch, T=clip.shape[1], H=s.H, W=s.W)
  a.update(kw)
  return _C.lib().lr_conv_stream_advance(a["x"], a["flags"], a["sb"], a["st"], a["sizes"], a["end"], a["w1"], a["w2"],
                                         a["w3"], a["b1"], a["b2"], a["b3"], a["feat"], a["counts"], a["state"],
                                         a["nstate"], a["ws"], a["nws"], a["B"], a["T"], a["H"], a["W"],
                                         _C.stream_handle())


def test_every_trap_answers_before_any_launch(dev):
  from lipreading_amd import _C
  fe, _, clips = bits_problem(dev)
  L = _C.lib()
  st = fe.stream(5, 16, 16, dev)
  st.feed(clips[:, :3])
  before = st.state_buf.clone()
  x = clips[:, 3:5]
  nws = L.lr_conv_stream_workspace_bytes(5, 2, 16, 16)
  ws = torch.full((nws,), 0xFF, dtype=U8, device=dev)
  feat = torch.full((5, 2, st.F), float("nan"), device=dev)
  counts = torch.full((5,), -7, dtype=I32, device=dev)
  bad, short = _C.LR_ERR_INVALID_ARG, _C.LR_ERR_WORKSPACE
  for kw in (dict(x=None), dict(w1=None), dict(w2=None), dict(w3=None), dict(b1=None), dict(b2=None), dict(b3=None),
             dict(feat=None), dict(counts=None), dict(state=None), dict(ws=None), dict(B=0), dict(B=-5), dict(T=-1),
             dict(H=24), dict(W=8), dict(H=0), dict(sb=-1), dict(st=-1), dict(flags=2), dict(flags=-1),
             dict(state=st.state_buf.data_ptr() + 4), dict(ws=ws.data_ptr() + 8)):
    assert advance_raw(st, x, None, None, feat, counts, ws, **kw) == bad, kw
  for kw in (dict(nstate=st.state_buf.numel() - 1), dict(nws=nws - 1), dict(nws=0), dict(B=6)):
    assert advance_raw(st, x, None, None, feat, counts, ws, **kw) == short, kw
  assert advance_raw(st, x, None, None, feat, counts, ws, B=65535, nstate=1 << 40, nws=1 << 40) == _C.LR_ERR_UNSUPPORTED
  assert advance_raw(st, x, None, None, feat, counts, ws, H=2048, nstate=1 << 40, nws=1 << 40) == _C.LR_ERR_UNSUPPORTED
  assert advance_raw(st, x, None, None, feat, counts, ws, T=0) == _C.LR_OK          # no end, no frames: nothing
  sp, n = st.state_buf.data_ptr(), st.state_buf.numel()
  m = ivec([1] * 5, dev)
  assert L.lr_conv_stream_reset(None, n, None, 5, 16, 16, _C.stream_handle()) == bad
  assert L.lr_conv_stream_reset(sp, n, None, 5, 24, 16, _C.stream_handle()) == bad
  assert L.lr_conv_stream_reset(sp, n - 1, m.data_ptr(), 5, 16, 16, _C.stream_handle()) == short
  assert L.lr_conv_stream_reset(sp, n, None, 5, 2048, 16, _C.stream_handle()) == _C.LR_ERR_UNSUPPORTED
  assert L.lr_conv_stream_read(sp, n, None, None, None, None, 5, 16, 16, _C.stream_handle()) == bad
  assert L.lr_conv_stream_read(None, n, m.data_ptr(), None, None, None, 5, 16, 16, _C.stream_handle()) == bad
  assert L.lr_conv_stream_read(sp, n - 1, m.data_ptr(), None, None, None, 5, 16, 16, _C.stream_handle()) == short
  torch.cuda.synchronize()
  assert torch.equal(st.state_buf, before) and torch.isnan(feat).all() and (counts == -7).all() and (ws == 0xFF).all()
  assert m.cpu().tolist() == [1] * 5
  assert advance_raw(st, x, None, None, feat, counts, ws) == _C.LR_OK               # ... and the call itself is fine
  assert counts.cpu().tolist() == [2] * 5 and not torch.isnan(feat).any()


# ---- 5: capture -------------------------------------------------------------------------------------------------------

def test_a_one_frame_advance_replays_as_a_linear_graph(dev):
  from lipreading_amd import _C
  fe, _, clips = bits_problem(dev)
  eager = fe.stream(2, 16, 16, dev)
  want = [eager.feed(clips[:2, t:t + 1]) for t in range(5)]
  assert [w[1].cpu().tolist() for w in want] == [[0, 0]] * 3 + [[1, 1]] * 2
  s = fe.stream(2, 16, 16, dev)
  nws = _C.lib().lr_conv_stream_workspace_bytes(2, 1, 16, 16)
  ws = torch.full((nws,), 0xFF, dtype=U8, device=dev)
  xb = torch.zeros((2, 1, 3, 16, 16), dtype=U8, device=dev)
  feat = torch.full((2, 1, s.F), float("nan"), device=dev)
  counts = torch.full((2,), -1, dtype=I32, device=dev)
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):                     # a warm-up outside the capture, then back to the empty state
    _C.check(advance_raw(s, xb, None, None, feat, counts, ws), "warm-up")
  torch.cuda.current_stream().wait_stream(side)
  s.reset()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    _C.check(advance_raw(s, xb, None, None, feat, counts, ws), "captured advance")
  for t in range(5):
    xb.copy_(clips[:2, t:t + 1])
    graph.replay()
    assert torch.equal(feat, want[t][0]) and torch.equal(counts, want[t][1]), t
  assert torch.equal(s.state_buf, eager.state_buf)


# ---- 6: compositions --------------------------------------------------------------------------------------------------

def test_chunked_frontend_equals_the_one_shot_features(dev):
  from lipreading_amd.frontend_stream import ChunkedFrontend
  p, fe, clips = exact("sq16", dev)
  lens = p.case.lens
  lens_d = ivec(lens, dev)
  outs = [ChunkedFrontend(fe, chunk)(clips, lens_d) for chunk in (1, 4, 9)]
  chunked = ChunkedFrontend(fe, 2)
  outs += [chunked(clips, lens_d), chunked(clips, lens_d)]       # the second call re-uses the session
  for out in outs:
    assert out.shape == (len(lens), max(lens), 96) and out.dtype == F32
    for b, n in enumerate(lens):
      C.compare_exact(out[b, :n], p.features[b], "chunked slot %d" % b, axes=("frame", "feature"))
      assert not out[b, n:].any()
  fe2, cpu_clips, clips2 = real_problem(dev, 2, 6, 32, 32, U8)
  params = [q.detach().cpu() for q in fe2.parameters_in_order()]
  out = ChunkedFrontend(fe2, 4)(clips2, ivec((6, 4), dev))
  for b, n in enumerate((6, 4)):
    want = O.conv_frontend(cpu_clips[b:b + 1, :n], params)[0].numpy()
    assert rel_err(out[b, :n].cpu().numpy(), want) < 2e-2 and not out[b, n:].any()


def _char2idx():
  from lipreading_amd.data import BOS, EOS, PAD
  c2i = {PAD: 0, BOS: 1, EOS: 2}
  for ch in " abcdefgh":
    c2i[ch] = len(c2i)
  return c2i


def pixel_model(dev, seed, bidirectional=False):
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.frontend import PixelLipReader
  fe = frontend(dev, seed=seed)
  c2i = _char2idx()
  torch.manual_seed(seed + 100)
  enc = VideoEncoder(96, 32, rnn_type="GRU", num_layers=1, bidirectional=bidirectional, enable_ctc=True,
                     vocab_size=len(c2i), char2idx=c2i, device=dev)
  return PixelLipReader(enc, fe).to(dev).eval()


def oracle_log_probs(model, clips, lens, bidirectional=False):
  """conv_frontend (bf16-emulating) -> float64 torch GRU -> masked log-softmax, on the CPU"""
  c2i = _char2idx()
  params = [q.detach().cpu() for q in model.frontend.parameters_in_order()]
  feats = O.conv_frontend(clips, params).double()
  twin = O.OracleVideoEncoder(96, 32, rnn_type="GRU", bidirectional=bidirectional, enable_ctc=True, vocab_size=len(c2i),
                              char2idx=c2i)
  twin.load_state_dict({k: v.detach().cpu() for k, v in model.encoder.state_dict().items()}, strict=False)
  twin = twin.double().eval()
  with torch.no_grad():
    return twin(feats, torch.tensor(lens))[0]


def pixel_errors(dev, seed, T=8):
  """(session's, one-shot path's) max |log-prob error| against the oracle on two unpadded clips; the session's
  log-probs, transcripts and the model"""
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.frontend_stream import PixelLiveTranscriber
  model = pixel_model(dev, seed)
  g = torch.Generator().manual_seed(seed)
  clips = torch.randint(0, 256, (2, T, 3, 16, 16), generator=g, dtype=U8)
  lens = [T, T]
  want = oracle_log_probs(model, clips, lens)
  with torch.no_grad():
    one = model(clips.to(dev), ivec(lens, dev))[0]
  dec = BeamCTCDecoder(ctc_labels(_char2idx()), beam_width=8, log_probs_input=True)
  live = PixelLiveTranscriber(model, dec, 2, T, 16, 16, dev)
  seen, encoder_feed = [], live.encoder_stream.feed      # the session's own log-probs, as the encoder session hands them on

  def recording_feed(feat, counts):
    seen.append((encoder_feed(feat, counts), counts))
    return seen[-1][0]
  live.encoder_stream.feed = recording_feed
  d = clips.to(dev)
  for t0 in range(0, T, 3):
    t1 = min(T, t0 + 3)
    live.feed(d[:, t0:t1], None, ivec([int(t1 == T)] * 2, dev) if t1 == T else None)
  lp = torch.stack([torch.cat([l[b, :int(c[b])] for l, c in seen]) for b in range(2)])
  assert lp.shape == want.shape == one.shape
  err_s = float((lp.cpu().double() - want).abs().max())
  err_o = float((one.cpu().double() - want).abs().max())
  live_classes = model.encoder.output_mask.cpu() > 0      # (the masked classes sit at log(1e-45): a constant's error)
  print("seed %d, unmasked classes only: session %.3e, one-shot %.3e" %
        (seed, float((lp.cpu().double() - want)[..., live_classes].abs().max()),
         float((one.cpu().double() - want)[..., live_classes].abs().max())))
  return err_s, err_o, lp, live, dec


def test_pixel_live_transcriber_tracks_the_oracle_as_the_one_shot_model_does(dev):
  # measured on an MI355X (max |log-prob error| against the oracle): session 6.774e-06, one-shot 6.774e-06, one-shot
  # on the second seed 7.931e-06 (the module docstring has the unmasked-class figures); the test prints them again
  err_s, err_o, lp, live, dec = pixel_errors(dev, 21)
  floor = pixel_errors(dev, 22)[1]
  print("session %.3e, one-shot %.3e, one-shot on a second seed %.3e" % (err_s, err_o, floor))
  # one bf16 rounding flip upstream is a discrete event that either path may take alone: 3 x, floored at the one-shot
  # path's error on a second seed
  assert err_s <= 3 * max(err_o, floor), (err_s, err_o, floor)
  lens = ivec([lp.shape[1]] * 2, dev)
  want, want_off = dec.decode(lp, lens)
  got, got_off = live.result()
  assert got == want and [[o.tolist() for o in r] for r in got_off] == [[o.tolist() for o in r] for r in want_off]
  assert live.frontend_stream.check().read()[1].cpu().tolist() == [lp.shape[1]] * 2
  assert live.encoder_stream.frames().cpu().tolist() == [lp.shape[1]] * 2


def test_chunked_pixel_lip_reader_with_a_full_look_ahead_tracks_the_one_shot_model(dev):
  from lipreading_amd.frontend_stream import ChunkedPixelLipReader
  T = 8
  model = pixel_model(dev, 23, bidirectional=True)
  g = torch.Generator().manual_seed(23)
  clips = torch.randint(0, 256, (2, T, 3, 16, 16), generator=g, dtype=U8)
  lens = [T, T]
  want = oracle_log_probs(model, clips, lens, bidirectional=True)
  with torch.no_grad():
    one = model(clips.to(dev), ivec(lens, dev))[0]
  chunked = ChunkedPixelLipReader(model, 3, lookahead=T)
  got = chunked(clips.to(dev), ivec(lens, dev), max_len=T, need_final_state=False)
  assert got[0].shape == one.shape and got[2] is None
  err_c = float((got[0].cpu().double() - want).abs().max())
  err_o = float((one.cpu().double() - want).abs().max())
  m2 = pixel_model(dev, 24, bidirectional=True)
  clips2 = torch.randint(0, 256, (2, T, 3, 16, 16), generator=g, dtype=U8)
  with torch.no_grad():
    floor = float((m2(clips2.to(dev), ivec(lens, dev))[0].cpu().double() -
                   oracle_log_probs(m2, clips2, lens, bidirectional=True)).abs().max())
  print("chunked %.3e, one-shot %.3e, one-shot on a second seed %.3e" % (err_c, err_o, floor))
  assert err_c <= 3 * max(err_o, floor), (err_c, err_o, floor)
  uni = ChunkedPixelLipReader(pixel_model(dev, 25), 3)            # ... and the causal composition runs, final state and all
  lp, hidden, state = uni(clips.to(dev), ivec([T, 5], dev))
  assert lp.shape[:2] == (2, T) and hidden.shape == (2, T, 32) and state.shape == (1, 2, 32) and torch.isfinite(lp).all()


def test_driver_streams_the_frontend(dev, tmp_path, capsys):
  from lipreading_amd import driver
  from lipreading_amd.dataset import write_synthetic_dataview
  root = str(tmp_path)
  write_synthetic_dataview(root, "synth/micro6", n_videos=6, captions_per_video=3, seed=11, frames=True, frame_hw=64,
                           min_seconds=0.7, max_seconds=1.3)
  common = dict(root=root, data="synth/micro6", frontend="conv3d", encoder="rnn", rnn_type="GRU", hidden_size=32,
                num_layers=1, batch_size=4, max_epochs=0, train_split=0.7, crop_size=32, cuda=True, ctc_decoder="beam",
                beam_width=8, stream_chunk=5, stream_frontend=True)
  capsys.readouterr()
  out = driver.run(bidirectional=False, stream_encoder=True, **common)
  text = capsys.readouterr().out
  assert re.search(r"Commit delay \(chunks of 5 frames\): .*\(encoder streamed; frontend streamed: adds 3 frames of "
                   r"latency\)", text), text
  assert "commit_delay" in out and 0.0 <= float(re.search(r"\tCER:\s+(\S+)", text).group(1))
  out = driver.run(bidirectional=True, stream_lookahead=4, **common)
  text = capsys.readouterr().out
  assert re.search(r"adds 4 frames of look-ahead latency; frontend streamed: adds 3 frames of latency\)", text), text
