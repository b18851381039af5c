"""Look-ahead sessions on the MI355X (lr_rnn_bistream_*, lipreading_amd/encoder_lookahead.py).

Every case runs with NaN-filled outputs, a 0xFF-filled workspace, guard words either side of y and log_probs, ragged
sizes and look-ahead per slot, NaN in the rows of a window past a slot's own end, and a head mask with two zeros (tests/
lookahead_cases.py).  The reference of every number is torch.nn on the CPU, one module per (layer, direction), with the
rules of an advance written out (lc_ref).

Against float64 (hold's rule of tests/test_gpu_transformer_fp64.py as it stands: element-wise, relative to the float64
tensor's largest entry, 4 x the error torch.nn's float32 CPU run makes on the same case, never less than 4 ulp): the
figures of the table are printed by the tests; the figures below are what an MI355X gave.

MEASURED (an MI355X; float32 CPU error, the bound = 4 x max(that, 1 ulp = 1.19e-7), the device's error):
  bigru20_i7 blocks_5_3 y                          cpu fp32 1.08e-07  bound 4.77e-07  device 8.51e-08
  bigru20_i7 blocks_5_3 log_probs                  cpu fp32 6.41e-08  bound 4.77e-07  device 8.17e-08
  bigru20_i7 blocks_5_3 h                          cpu fp32 9.48e-08  bound 4.77e-07  device 7.81e-08
  bigru20_i7 ragged y                              cpu fp32 1.17e-07  bound 4.77e-07  device 1.08e-07
  bigru20_i7 ragged log_probs                      cpu fp32 6.41e-08  bound 4.77e-07  device 8.17e-08
  bigru20_i7 ragged h                              cpu fp32 7.91e-08  bound 4.77e-07  device 7.81e-08
  bigru20_i7 ragged log_probs of the zero row      cpu fp32 5.00e-08  bound 4.77e-07  device 6.26e-08
  bilstm36_b17 blocks_5_3 y                        cpu fp32 1.89e-07  bound 7.55e-07  device 1.76e-07
  bilstm36_b17 blocks_5_3 log_probs                cpu fp32 1.05e-07  bound 4.77e-07  device 1.02e-07
  bilstm36_b17 blocks_5_3 h                        cpu fp32 1.21e-07  bound 4.85e-07  device 1.07e-07
  bilstm36_b17 blocks_5_3 c                        cpu fp32 1.07e-07  bound 4.77e-07  device 1.17e-07
  bilstm36_b17 blocks_5_3 log_probs of the zero row cpu fp32 4.11e-08  bound 4.77e-07  device 4.11e-08
  bilstm36_b17 ragged y                            cpu fp32 1.80e-07  bound 7.18e-07  device 1.97e-07
  bilstm36_b17 ragged log_probs                    cpu fp32 9.69e-08  bound 4.77e-07  device 1.07e-07
  bilstm36_b17 ragged h                            cpu fp32 1.21e-07  bound 4.85e-07  device 1.07e-07
  bilstm36_b17 ragged c                            cpu fp32 1.07e-07  bound 4.77e-07  device 1.17e-07
  bilstm36_b17 ragged log_probs of the zero row    cpu fp32 4.11e-08  bound 4.77e-07  device 4.11e-08
  birnn16 blocks_5_3 y                             cpu fp32 1.22e-07  bound 4.90e-07  device 1.26e-07
  birnn16 blocks_5_3 log_probs                     cpu fp32 9.30e-08  bound 4.77e-07  device 6.51e-08
  birnn16 blocks_5_3 h                             cpu fp32 1.34e-07  bound 5.34e-07  device 1.42e-07
  birnn16 blocks_5_3 log_probs of the zero row     cpu fp32 3.16e-08  bound 4.77e-07  device 3.16e-08
  birnn16 ragged y                                 cpu fp32 9.10e-08  bound 4.77e-07  device 1.26e-07
  birnn16 ragged log_probs                         cpu fp32 9.30e-08  bound 4.77e-07  device 6.51e-08
  birnn16 ragged h                                 cpu fp32 8.66e-08  bound 4.77e-07  device 1.42e-07
  birnn16 ragged log_probs of the zero row         cpu fp32 3.16e-08  bound 4.77e-07  device 3.16e-08
  bigru256 blocks_5_3 y                            cpu fp32 3.18e-07  bound 1.27e-06  device 2.66e-07
  bigru256 blocks_5_3 log_probs                    cpu fp32 8.35e-08  bound 4.77e-07  device 9.56e-08
  bigru256 blocks_5_3 h                            cpu fp32 2.35e-07  bound 9.39e-07  device 1.67e-07
  bigru256 blocks_5_3 log_probs of the zero row    cpu fp32 3.55e-08  bound 4.77e-07  device 3.55e-08
  bigru256 ragged y                                cpu fp32 4.19e-07  bound 1.68e-06  device 2.62e-07
  bigru256 ragged log_probs                        cpu fp32 9.38e-08  bound 4.77e-07  device 9.92e-08
  bigru256 ragged h                                cpu fp32 2.46e-07  bound 9.85e-07  device 1.67e-07
  bigru256 ragged log_probs of the zero row        cpu fp32 3.55e-08  bound 4.77e-07  device 3.55e-08
  bilstm700 blocks_5_3 y                           cpu fp32 4.17e-07  bound 1.67e-06  device 4.54e-07
  bilstm700 blocks_5_3 log_probs                   cpu fp32 6.83e-08  bound 4.77e-07  device 5.54e-08
  bilstm700 blocks_5_3 h                           cpu fp32 3.26e-07  bound 1.31e-06  device 3.32e-07
  bilstm700 blocks_5_3 c                           cpu fp32 2.72e-07  bound 1.09e-06  device 2.82e-07
  bilstm700 blocks_5_3 log_probs of the zero row   cpu fp32 7.00e-08  bound 4.77e-07  device 2.11e-08
  bilstm700 ragged y                               cpu fp32 4.17e-07  bound 1.67e-06  device 4.54e-07
  bilstm700 ragged log_probs                       cpu fp32 6.83e-08  bound 4.77e-07  device 5.54e-08
  bilstm700 ragged h                               cpu fp32 3.26e-07  bound 1.31e-06  device 3.32e-07
  bilstm700 ragged c                               cpu fp32 2.72e-07  bound 1.09e-06  device 2.82e-07
  bilstm700 ragged log_probs of the zero row       cpu fp32 7.00e-08  bound 4.77e-07  device 2.11e-08
  sat_bilstm blocks_5_3 y                          cpu fp32 5.95e-08  bound 4.77e-07  device 5.30e-08
  sat_bilstm blocks_5_3 log_probs                  cpu fp32 9.07e-08  bound 4.77e-07  device 6.29e-08
  sat_bilstm blocks_5_3 h                          cpu fp32 5.95e-08  bound 4.77e-07  device 3.26e-08
  sat_bilstm blocks_5_3 c                          cpu fp32 1.59e-08  bound 4.77e-07  device 1.22e-08
  sat_bilstm blocks_5_3 log_probs of the zero row  cpu fp32 5.12e-08  bound 4.77e-07  device 4.44e-08
  sat_bilstm ragged y                              cpu fp32 5.95e-08  bound 4.77e-07  device 5.30e-08
  sat_bilstm ragged log_probs                      cpu fp32 9.07e-08  bound 4.77e-07  device 6.29e-08
  sat_bilstm ragged h                              cpu fp32 5.95e-08  bound 4.77e-07  device 3.26e-08
  sat_bilstm ragged c                              cpu fp32 1.59e-08  bound 4.77e-07  device 1.22e-08
  sat_bilstm ragged log_probs of the zero row      cpu fp32 5.12e-08  bound 4.77e-07  device 4.44e-08
  bigru20_i7 one_shot y                            cpu fp32 1.17e-07  bound 4.77e-07  device 1.08e-07
  bigru20_i7 one_shot log_probs                    cpu fp32 6.41e-08  bound 4.77e-07  device 8.17e-08
  bigru20_i7 one_shot h                            cpu fp32 6.71e-08  bound 4.77e-07  device 7.81e-08
  bilstm36_b17 one_shot y                          cpu fp32 1.95e-07  bound 7.79e-07  device 1.68e-07
  bilstm36_b17 one_shot log_probs                  cpu fp32 1.02e-07  bound 4.77e-07  device 1.05e-07
  bilstm36_b17 one_shot h                          cpu fp32 1.07e-07  bound 4.77e-07  device 1.07e-07
  bilstm36_b17 one_shot c                          cpu fp32 1.02e-07  bound 4.77e-07  device 1.17e-07
  bilstm36_b17 one_shot log_probs of the zero row  cpu fp32 4.11e-08  bound 4.77e-07  device 4.11e-08
  birnn16 one_shot y                               cpu fp32 1.91e-07  bound 7.64e-07  device 1.26e-07
  birnn16 one_shot log_probs                       cpu fp32 9.30e-08  bound 4.77e-07  device 6.51e-08
  birnn16 one_shot h                               cpu fp32 2.09e-07  bound 8.35e-07  device 1.42e-07
  birnn16 one_shot log_probs of the zero row       cpu fp32 3.16e-08  bound 4.77e-07  device 3.16e-08
  bigru256 one_shot y                              cpu fp32 3.46e-07  bound 1.39e-06  device 2.64e-07
  bigru256 one_shot log_probs                      cpu fp32 7.22e-08  bound 4.77e-07  device 8.42e-08
  bigru256 one_shot h                              cpu fp32 2.67e-07  bound 1.07e-06  device 1.67e-07
  bigru256 one_shot log_probs of the zero row      cpu fp32 3.55e-08  bound 4.77e-07  device 3.55e-08
  bilstm700 one_shot y                             cpu fp32 2.58e-07  bound 1.03e-06  device 4.54e-07
  bilstm700 one_shot log_probs                     cpu fp32 6.83e-08  bound 4.77e-07  device 5.54e-08
  bilstm700 one_shot h                             cpu fp32 2.57e-07  bound 1.03e-06  device 3.32e-07
  bilstm700 one_shot c                             cpu fp32 2.43e-07  bound 9.71e-07  device 2.82e-07
  bilstm700 one_shot log_probs of the zero row     cpu fp32 7.00e-08  bound 4.77e-07  device 2.11e-08
  sat_bilstm one_shot y                            cpu fp32 5.46e-08  bound 4.77e-07  device 5.30e-08
  sat_bilstm one_shot log_probs                    cpu fp32 9.07e-08  bound 4.77e-07  device 6.29e-08
  sat_bilstm one_shot h                            cpu fp32 4.06e-08  bound 4.77e-07  device 3.26e-08
  sat_bilstm one_shot c                            cpu fp32 1.22e-08  bound 4.77e-07  device 1.22e-08
  sat_bilstm one_shot log_probs of the zero row    cpu fp32 5.12e-08  bound 4.77e-07  device 4.44e-08
  chunked(4, 14) log_probs                         cpu fp32 9.14e-08  bound 4.77e-07  device 8.06e-08
  chunked(4, 14) hidden                            cpu fp32 2.86e-07  bound 1.14e-06  device 2.09e-07
The device lands at 0.03 .. 0.44 of its bound; no bound was tuned to it.
"""
import re

import pytest
import torch

from tests import encoder_stream_cases as U
from tests import lookahead_cases as C
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
    _memo[key] = C.lc_ref(case, w, x, C.PLANS[plan_name](case, lens), dtype)
  return _memo[key]


def session_run(name, dev, plan_name, **kw):
  key = (name, plan_name, "gpu", tuple(sorted(kw.items())))
  if key not in _memo:
    case, w, x, lens = setup(name)
    _memo[key] = C.Session(case, w, dev).run(x, C.PLANS[plan_name](case, lens), **kw)
  return _memo[key]


def same_bits(a, b, what):
  for k in ("y", "lp", "h", "c", "frames", "state", "zero_row"):
    if a[k] is None or b[k] is None:
      assert k == "zero_row" or (a[k] is None and b[k] is None), (what, k)   # (a plan may meet no row past a slot's frames)
      continue
    u, v = (C.fed_rows(a[k], a["fed"]), C.fed_rows(b[k], b["fed"])) if k == "lp" else (a[k], b[k])
    assert torch.equal(u, v), (what, k)


def hold_all(tag, case, w, lens, got, r64, r32):
  assert got["fed"] == lens and got["frames"].cpu().tolist() == lens
  hold(tag + " y", got["y"], r64["y"], r32["y"])
  hold(tag + " log_probs", C.fed_rows(got["lp"], lens), C.fed_rows(r64["lp"], lens), C.fed_rows(r32["lp"], lens))
  hold(tag + " h", got["h"], r64["h"], r32["h"])
  if case.cell == "LSTM":
    hold(tag + " c", got["c"], r64["c"], r32["c"])
  if got["zero_row"] is not None:   # rows past a slot's frames: the head of the zero row
    z = torch.zeros(1, 2 * case.H)
    hold(tag + " log_probs of the zero row", got["zero_row"].view(1, -1), C.head(case, w, z, torch.float64),
         C.head(case, w, z, torch.float32))
  lp = C.fed_rows(got["lp"], lens)
  assert (lp[:, 1] < -90).all() and (lp[:, case.C - 1] < -90).all() and torch.isfinite(lp).all()   # masked: finite, ~-103


# ---- 1: against float64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plan", ["blocks_5_3", "ragged"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_session_matches_float64(dev, name, plan):
  case, w, x, lens = setup(name)
  hold_all("%s %s" % (name, plan), case, w, lens, session_run(name, dev, plan), ref(name, plan, torch.float64),
           ref(name, plan, torch.float32))


# ---- 2: one advance is the one-shot model ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.CASES))
def test_one_advance_is_the_one_shot_model(dev, name):
  case, w, x, lens = setup(name)
  hold_all(name + " one_shot", case, w, lens, session_run(name, dev, "one_chunk"),
           C.one_shot_ref(case, w, x, lens, torch.float64), C.one_shot_ref(case, w, x, lens, torch.float32))


# ---- 3: bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.BIT_CASES)
def test_full_lookahead_gives_the_single_advances_bits(dev, name):
  one = session_run(name, dev, "one_chunk")
  for plan in ("blocks_4_full", "frame_by_frame_full"):
    same_bits(session_run(name, dev, plan), one, plan)
  case, w, x, lens = setup(name)
  again = C.Session(case, w, dev).run(x, C.blocks_4_full(case, lens), read_between=True)   # reads between feeds
  same_bits(again, one, "second run")


@pytest.mark.parametrize("name", C.BIT_CASES)
def test_layer_0s_forward_state_is_the_same_bits_under_every_plan(dev, name):
  case = C.CASES[name]
  one = session_run(name, dev, "one_chunk")
  for plan in C.PLANS:
    got = session_run(name, dev, plan)
    assert torch.equal(got["h"][0], one["h"][0]), plan
    if case.cell == "LSTM":
      assert torch.equal(got["c"][0], one["c"][0]), plan
    assert got["frames"].cpu().tolist() == one["frames"].cpu().tolist(), plan


def test_a_permuted_batch_gives_the_permuted_bits(dev):
  case, w, x, lens = setup("bigru256")
  perm = [2, 0, 3, 1]
  base = session_run("bigru256", dev, "blocks_5_3")
  plens = [lens[p] for p in perm]
  got = C.Session(case, w, dev).run(x[perm], C.blocks_5_3(case, plens))
  assert torch.equal(got["y"], base["y"][perm]) and torch.equal(got["h"], base["h"][:, perm])
  for i, p in enumerate(perm):
    assert torch.equal(got["lp"][i, :lens[p]], base["lp"][p, :lens[p]])


def test_alone_equals_slot_16_of_17(dev):
  case, w, x, lens = setup("bilstm36_b17")
  base = session_run("bilstm36_b17", dev, "blocks_5_3")
  got = C.Session(case, w, dev, B=1).run(x[16:17], C.blocks_5_3(case, [lens[16]]))
  n = lens[16]
  assert torch.equal(got["y"][0], base["y"][16]) and torch.equal(got["lp"][0, :n], base["lp"][16, :n])
  assert torch.equal(got["h"][:, 0], base["h"][:, 16]) and torch.equal(got["c"][:, 0], base["c"][:, 16])


# ---- 4: slot rules --------------------------------------------------------------------------------------------------

def test_idle_and_look_only_slots_keep_every_byte(dev):
  case, w, x, lens = setup("bilstm36_b17")
  s = C.Session(case, w, dev)
  first = [min(n, 3) for n in lens]
  s.feed(x[:, :5].to(dev), 3, first, [min(n - f, 2) for n, f in zip(lens, first)])
  before = s.state.clone()
  h0, c0, f0, _ = s.read()
  # slot 0 consumes, the odd slots look only (some past what they have: clamped), the others idle
  sizes = [2] + [0] * (case.B - 1)
  ahead = [1] + [(9 if b % 2 else 0) for b in range(1, case.B)]
  s.feed(x[:, 3:8].to(dev), 2, sizes, ahead)
  h1, c1, f1, st1 = s.read()
  for b in range(1, case.B):
    assert torch.equal(s.slot_bytes(s.state, b), s.slot_bytes(before, b)), b
  assert torch.equal(h1[:, 1:], h0[:, 1:]) and torch.equal(c1[:, 1:], c0[:, 1:]) and torch.equal(f1[1:], f0[1:])
  assert int(f1[0]) == int(f0[0]) + 2 and not torch.equal(h1[:, 0], h0[:, 0]) and not st1.any()


def test_sizes_and_ahead_are_clamped(dev):
  case, w, x, lens = setup("bigru256")
  xd = x[:, :7].to(dev)
  a, b = C.Session(case, w, dev), C.Session(case, w, dev)
  ya, la = a.feed(xd, 4, [4, 4, 0, 0], [3, 3, 0, 7])
  yb, lb = b.feed(xd, 4, [99, 1 << 30, -5, 0], [99, 1 << 30, -1, 1 << 30])
  assert torch.equal(ya, yb) and torch.equal(la, lb) and torch.equal(a.state, b.state)
  assert a.read()[2].cpu().tolist() == [4, 4, 0, 0]
  yn, ln = C.Session(case, w, dev).feed(xd, 4, None, None)            # NULL sizes: chunk_T, NULL ahead: 0
  y0, l0 = C.Session(case, w, dev).feed(xd[:, :4], 4, [4] * 4, [0] * 4)
  assert torch.equal(yn, y0) and torch.equal(ln, l0)


def test_a_masked_reset_restarts_only_its_slots(dev):
  case, w, x, lens = setup("bilstm36_b17")
  base = session_run("bilstm36_b17", dev, "one_chunk")
  s = C.Session(case, w, dev)
  first = [min(n, 3) for n in lens]
  mask = [b % 2 for b in range(case.B)]
  keep = [b for b in range(case.B) if not mask[b]]
  gone = [b for b in range(case.B) if mask[b]]
  xa = torch.full((case.B, case.T, case.I), float("nan"))
  for b, n in enumerate(lens):
    xa[b, :n] = x[b, :n]
  s.feed(xa.to(dev), 3, first, [n - f for n, f in zip(lens, first)])   # (the whole rest seen: the single advance's bits)
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
  y, lp = s.feed(xc.to(dev), case.T, sizes, None)
  for b in gone:
    assert torch.equal(y[b], base["y"][b]) and torch.equal(lp[b, :lens[b]], base["lp"][b, :lens[b]])
  for b in keep:
    assert torch.equal(y[b, :sizes[b]], base["y"][b, first[b]:lens[b]])
  assert torch.equal(s.state, base["state"])


def _status_words(state, B):
  return state[:32 * B].view(torch.int32).view(B, 8)[:, 6]


def test_the_two_kinds_of_session_refuse_each_others_state(dev):
  from lipreading_amd import _C
  case, w, x, lens = setup("bilstm36_b17")
  ucase = U.CASES["lstm36_b17"]
  assert (ucase.cell, ucase.I, ucase.H, ucase.layers, ucase.B) == (case.cell, case.I, case.H, case.layers, case.B)
  bi, uni = C.Session(case, w, dev), U.Session(ucase, U.weights(ucase), dev)
  first = [min(n, 3) for n in lens]
  bi.feed(x[:, :3].to(dev), 3, first, None)
  uni.feed(x[:, :3].to(dev), first)
  assert bi.state.numel() == uni.state.numel()
  ws = torch.full((1 << 22,), 0xFF, dtype=torch.uint8, device=dev)
  xd = x[:, 3:6].to(dev)
  # a causal session's state handed to the look-ahead advance
  before = uni.state.clone()
  y = torch.full((case.B, 2, 2 * case.H), float("nan"), device=dev)
  _C.check(bi.advance_raw(xd, None, None, y, None, ws, 2, state=uni.state), "advance")
  assert not y.any()                                 # nothing ran: every row is the zero row
  after = uni.state.clone()
  assert (_status_words(after, case.B) == _C.LR_RNN_STREAM_MISMATCH).all()
  _status_words(after, case.B).zero_()
  assert torch.equal(after, before)
  assert (uni.read()[3] == _C.LR_RNN_STREAM_MISMATCH).all()
  # ... and a look-ahead session's state handed to the causal advance
  before = bi.state.clone()
  mine, uni.state = uni.state, bi.state
  yu = torch.full((case.B, 2, case.H), float("nan"), device=dev)
  _C.check(uni.advance_raw(xd[:, :2], None, yu, None, ws), "advance")
  uni.state = mine
  after = bi.state.clone()
  assert (_status_words(after, case.B) == _C.LR_RNN_STREAM_MISMATCH).all()
  _status_words(after, case.B).zero_()
  assert torch.equal(after, before)
  h, c, frames, status = bi.read()
  assert (status == _C.LR_RNN_STREAM_MISMATCH).all() and frames.cpu().tolist() == first
  bi.reset([1] * case.B)   # the bit stays until a reset of the slot
  assert not bi.read()[3].any()


@pytest.mark.parametrize("how", ["H", "layers", "cell"])
def test_an_advance_of_another_configuration_leaves_the_state_alone(dev, how):
  from lipreading_amd import _C
  case, w, x, lens = setup("bilstm36_b17")
  s = C.Session(case, w, dev)
  s.feed(x[:, :3].to(dev), 3, [min(n, 3) for n in lens], None)
  before = s.state.clone()
  kw = dict(H=20) if how == "H" else dict(layers=1) if how == "layers" else dict(mode=0)
  ws = torch.full((1 << 22,), 0xFF, dtype=torch.uint8, device=dev)
  y = torch.full((case.B, 2, 2 * 64), float("nan"), device=dev)
  _C.check(s.advance_raw(x[:, 3:6].to(dev), None, None, y, None, ws, 2, **kw), "advance")
  after = s.state.clone()
  assert (_status_words(after, case.B) == _C.LR_RNN_STREAM_MISMATCH).all()
  _status_words(after, case.B).zero_()
  assert torch.equal(after, before)


def test_short_buffers_write_nothing(dev):
  from lipreading_amd import _C
  case, w, x, lens = setup("bigru20_i7")
  s = C.Session(case, w, dev)
  before = s.state.clone()
  nws = s.L.lr_rnn_bistream_workspace_bytes(s.mode, 1, 5, case.T, case.I, case.H, 1, case.C)
  ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=dev)
  y = torch.full((1, 5, 2 * case.H), float("nan"), device=dev)
  lp = torch.full((1, 5, case.C), float("nan"), device=dev)
  xd = x.to(dev)
  for kw in (dict(state_bytes=s.state.numel() - 1), dict(pack_bytes=s.pack.numel() - 1), dict(ws_bytes=nws - 1)):
    assert s.advance_raw(xd, None, None, y, lp, ws, 5, **kw) == _C.LR_ERR_WORKSPACE
  assert s.advance_raw(xd, None, None, y, lp, ws, 5, window_T=4) == _C.LR_ERR_INVALID_ARG
  torch.cuda.synchronize()
  assert torch.equal(s.state, before) and torch.isnan(y).all() and torch.isnan(lp).all() and (ws == 0xFF).all()


# ---- 5: strided views, capture --------------------------------------------------------------------------------------

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
  return VideoEncoder(204, H, rnn_type=rnn_type, num_layers=layers, bidirectional=True, enable_ctc=ctc,
                      vocab_size=len(c2i), char2idx=c2i, device=dev).to(dev).eval()


def test_strided_views_go_in_without_a_copy(dev):
  enc = _encoder(dev)
  g = torch.Generator().manual_seed(3)
  frames = torch.randn(3, 20, 68, 3, generator=g).to(dev)
  a, b = enc.stream_lookahead(3, dev), enc.stream_lookahead(3, dev)
  for t0, t1, w1 in ((0, 7, 12), (7, 8, 20), (8, 20, 20)):
    view = frames[:, t0:w1]
    ahead = torch.full((3,), w1 - t1, dtype=torch.int32, device=dev)
    assert not view.is_contiguous() and a._frames_3d(view).data_ptr() == view.data_ptr()
    lp_v, y_v = a.feed(view, None, ahead, need_hidden=True, chunk=t1 - t0)
    lp_c, y_c = b.feed(view.contiguous().view(3, w1 - t0, 204), None, ahead, need_hidden=True, chunk=t1 - t0)
    assert lp_v.shape == (3, t1 - t0, enc.adj_vocab_size) and y_v.shape == (3, t1 - t0, 64)
    assert torch.equal(lp_v, lp_c) and torch.equal(y_v, y_c)
  assert torch.equal(a.state_buf, b.state_buf) and a.frames().cpu().tolist() == [20, 20, 20]
  h, c, frames_, status = a.read()
  assert h.shape == (2, 3, 32) and c is None and not status.any()


def test_a_fixed_shape_advance_replays_as_a_linear_graph(dev):
  from lipreading_amd import _C
  case, w, x, lens = setup("bigru20_i7")
  eager = C.Session(case, w, dev)
  want = [eager.feed(x[:, t:t + 3].to(dev), 1, None, [2]) for t in range(5)]
  s = C.Session(case, w, dev)
  nws = s.L.lr_rnn_bistream_workspace_bytes(s.mode, 1, 1, 3, case.I, case.H, 1, case.C)
  ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=dev)
  xb = torch.zeros(1, 3, case.I, device=dev)
  ahead = torch.tensor([2], dtype=torch.int32, device=dev)
  y = torch.full((1, 1, 2 * case.H), float("nan"), device=dev)
  lp = torch.full((1, 1, case.C), float("nan"), device=dev)
  side = torch.cuda.Stream(device=dev)
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):                     # a warm-up outside the capture, then back to the empty state
    _C.check(s.advance_raw(xb, None, ahead, y, lp, ws, 1), "warm-up")
  torch.cuda.current_stream().wait_stream(side)
  s.reset()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    _C.check(s.advance_raw(xb, None, ahead, y, lp, ws, 1), "captured advance")
  for t in range(5):
    xb.copy_(x[:, t:t + 3])
    graph.replay()
    assert torch.equal(y, want[t][0]) and torch.equal(lp, want[t][1]), t
  assert torch.equal(s.state, eager.state)


# ---- 6: front doors -------------------------------------------------------------------------------------------------

def _door_case(enc, frames, lens):
  """the encoder's own weights as a case of lookahead_cases, for the float64 reference"""
  B, T = frames.shape[:2]
  case = C.Case("door", enc.rnn_type, 204, enc.hidden_size, enc.num_layers, B, T, enc.adj_vocab_size, False)
  w = dict(w_ih=[], w_hh=[], b_ih=[], b_hh=[])
  for l in range(enc.num_layers):
    lw = [p.detach().cpu() for p in enc.rnn.layer_weights(l, 2)]
    for d in range(2):
      for i, k in enumerate(("w_ih", "w_hh", "b_ih", "b_hh")):
        w[k].append(lw[4 * d + i])
  w["head_w"], w["head_b"] = enc.output_proj.weight.detach().cpu(), enc.output_proj.bias.detach().cpu()
  w["head_mask"] = enc.output_mask.detach().cpu()
  return case, w


def test_chunked_lookahead_encoder_with_full_lookahead_is_the_encoder(dev):
  from lipreading_amd import train as T
  from lipreading_amd.decoder import BeamCTCDecoder, GreedyDecoder, ctc_labels
  from lipreading_amd.encoder_lookahead import ChunkedLookaheadEncoder
  enc = _encoder(dev)
  c2i = _char2idx()
  g = torch.Generator().manual_seed(6)
  frames = torch.randn(3, 14, 68, 3, generator=g)
  frame_lens = torch.tensor([14, 9, 12])
  lens = frame_lens.tolist()
  chunked = ChunkedLookaheadEncoder(enc, 4, 14)
  lp, hidden, state = chunked(frames.to(dev), frame_lens.to(dev), max_len=14)
  assert lp.shape == (3, 14, enc.adj_vocab_size) and hidden.shape == (3, 14, 64) and state is None
  one = ChunkedLookaheadEncoder(enc, 14, 0)(frames.to(dev), frame_lens.to(dev), max_len=14)
  assert torch.equal(lp, one[0]) and torch.equal(hidden, one[1])          # full look-ahead: the single advance's bits
  with torch.no_grad():
    want = enc(frames.to(dev), frame_lens.to(dev), max_len=14, need_final_state=False)
  case, w = _door_case(enc, frames, lens)
  x = frames.view(3, 14, 204)
  r64, r32 = C.one_shot_ref(case, w, x, lens, torch.float64), C.one_shot_ref(case, w, x, lens, torch.float32)
  hold("chunked(4, 14) log_probs", C.fed_rows(lp, lens), C.fed_rows(r64["lp"], lens), C.fed_rows(r32["lp"], lens))
  hold("chunked(4, 14) hidden", hidden, r64["y"], r32["y"])
  greedy = GreedyDecoder(ctc_labels(c2i))
  assert greedy.decode(lp, frame_lens.to(dev))[0] == greedy.decode(want[0], frame_lens.to(dev))[0]
  # bounded look-ahead goes through the evaluation loop
  dec = BeamCTCDecoder(ctc_labels(c2i), beam_width=8, log_probs_input=True)
  chars = torch.tensor([[1, 4, 5, 2], [1, 6, 2, 0], [1, 7, 8, 2]])
  loader = [(frames, frame_lens, chars, torch.tensor([4, 3, 4]))]
  cer = T.ctc_cer(ChunkedLookaheadEncoder(enc, 4, 2), loader, dev, c2i, dec)
  assert 0.0 <= cer
  assert T.ctc_cer(chunked, loader, dev, c2i, dec) == T.ctc_cer(ChunkedLookaheadEncoder(enc, 14, 0), loader, dev, c2i, dec)


def test_lookahead_transcriber_equals_the_search_on_the_sessions_log_probs(dev):
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.encoder_lookahead import LookaheadTranscriber
  enc = _encoder(dev)
  dec = BeamCTCDecoder(ctc_labels(_char2idx()), beam_width=8, log_probs_input=True)
  g = torch.Generator().manual_seed(4)
  frames = torch.randn(3, 23, 204, generator=g).to(dev)
  lens = torch.tensor([23, 11, 17], dtype=torch.int32, device=dev)
  live = LookaheadTranscriber(enc, dec, 3, 23, dev)
  plain = enc.stream_lookahead(3, dev)
  lps = []
  for t0 in range(0, 23, 5):
    n, t1 = min(5, 23 - t0), min(23, t0 + 8)
    sizes, ahead = (lens - t0).clamp(0, n), (lens - t0 - n).clamp(0, 3)
    live.feed(frames[:, t0:t1], sizes, ahead, chunk=n)
    lps.append(plain.feed(frames[:, t0:t1], sizes, ahead, chunk=n))
  want, want_off = dec.decode(torch.cat(lps, dim=1), lens)
  got, got_off = live.result()
  assert got == want and [[o.tolist() for o in r] for r in got_off] == [[o.tolist() for o in r] for r in want_off]
  assert [p[0] for p in live.partial()] == [s[0] for s in want]
  assert torch.equal(live.encoder_stream.state_buf, plain.state_buf)
  assert live.encoder_stream.frames().cpu().tolist() == [23, 11, 17]
  live.reset(torch.tensor([0, 1, 0], device=dev))
  assert live.encoder_stream.frames().cpu().tolist() == [23, 0, 17]


def test_driver_streams_a_bidirectional_encoder(dev, tmp_path, capsys):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=6, captions_per_video=4, seed=7)
  flags = ["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True", "--ctc_only=True",
           "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=0", "--ctc_decoder=beam", "--beam_width=8",
           "--bidirectional=True", "--stream_chunk=5", "--stream_lookahead=2"]
  capsys.readouterr()
  out = driver.run(**driver.parse_flags(flags))
  text = capsys.readouterr().out
  assert re.search(r"Commit delay \(chunks of 5 frames\): .*adds 2 frames of look-ahead latency", text), text
  assert 0.0 <= float(re.search(r"\tCER:\s+(\S+)", text).group(1)) and "commit_delay" in out
