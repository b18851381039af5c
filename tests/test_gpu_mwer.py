"""GPU: lr_ctc_nbest_risk / lr_ctc_nbest_risk_grad through lipreading_amd.mwer against the float64 restatement of
tests/mwer_cases.py, the contract's edge cases, MWERLoss end to end, train.mwer_step and the driver's --mwer.

Measured on the MI355X over parity_cases() (the tolerances are 8 x the float32 restatement's own errors, see
tests/mwer_cases.py): the figures are in DESIGN.md §25."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lipreading_amd import _C
from lipreading_amd import mwer as M
from tests import mwer_cases as K
from tests.test_gpu_ctc import LOSS_TOL

pytestmark = pytest.mark.gpu

PARITY = dict(K.parity_cases())


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(name):
  """The float64 restatement of a parity case: computed once, shared, never modified."""
  return K.run(PARITY[name])


def device_run(case, dev, reduction='mean', scale=None, lp_of=None, ids_of=None, blank=None):
  """The front door on a case: fp32 log_softmax of the logits on the device, the loss, autograd back to the
  log-probabilities — the kernel's own output, bit for bit.  (Its rows sum to zero, so it is also the gradient at the
  logits, which the restatement returns.)"""
  lp = F.log_softmax(torch.tensor(case["logits"], dtype=torch.float32, device=dev), dim=-1)
  if lp_of is not None:
    lp = lp_of(lp)
  x = lp = lp.detach().requires_grad_(True)
  ids = torch.tensor(case["hyp_ids"], device=dev)
  lens = torch.tensor(case["hyp_lens"], device=dev)
  if ids_of is not None:
    ids, lens = ids_of(ids, lens)
  sizes = None if case["sizes"] is None else torch.tensor(case["sizes"], device=dev)
  loss, status, info = M.nbest_risk_loss(lp, sizes, ids, lens, torch.tensor(case["risk"], device=dev),
                                         blank_index=case["blank"] if blank is None else blank, reduction=reduction)
  (loss if scale is None else loss * scale).backward()
  return dict(loss=float(loss.detach()), loss_t=loss.detach(), grad=x.grad.double().cpu().numpy(), grad_t=x.grad,
              hyp_ll=info["hyp_ll"].double().cpu().numpy(), hyp_ll_t=info["hyp_ll"],
              posterior=info["posterior"].double().cpu().numpy(), status=info["hyp_status"].cpu().numpy(),
              utt_risk=info["utt_risk"].double().cpu().numpy(), batch_status=int(status.item()))


def check_parity(got, want, what):
  assert (got["status"] == want["status"]).all(), (what, got["status"], want["status"])
  assert got["batch_status"] == want["batch_status"]
  g, l, ll = K.rel_errors(got, want)
  p = np.abs(got["posterior"] - want["posterior"]).max()
  print("%s: device against float64: grad %.3e (tol %.3e) loss %.3e (tol %.3e) hyp_ll %.3e (tol %.3e) posterior %.3e"
        % (what, g, K.TOL_GRAD, l, K.TOL_LOSS, ll, K.TOL_LL, p))
  assert np.isneginf(got["hyp_ll"][want["status"] != K.USED]).all()
  assert (got["posterior"][want["status"] != K.USED] == 0).all()
  assert g <= K.TOL_GRAD and l <= K.TOL_LOSS and ll <= K.TOL_LL and p <= K.TOL_POST_ABS
  np.testing.assert_allclose(got["utt_risk"], want["utt_risk"], rtol=K.TOL_LOSS, atol=1e-6)


# ---- parity with the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_with_the_float64_restatement(dev, name):
  case, want = PARITY[name], reference(name)
  K.assert_spread(want, case["N"])                    # a condition on the oracle alone
  assert 1 in case["sizes"].tolist() and len(set(case["sizes"].tolist())) > 1 or case["T"] == 1   # ragged, down to 1
  check_parity(device_run(case, dev), want, name)


def test_parity_at_the_longest_hypotheses(dev):
  """513 states: two per thread of the lattice kernel.  Held to the tolerances of the 76-frame cases."""
  case = K.wide_case()
  want = K.run(case)
  assert (want["status"] == K.USED).all() and case["hyp_lens"].max() == 256
  check_parity(device_run(case, dev), want, "wide")


def test_sum_reduction(dev):
  case = PARITY["T17_N3_C65"]
  check_parity(device_run(case, dev, reduction='sum'), K.run(case, reduction='sum'), "sum")


# ---- edge and contract cases ------------------------------------------------------------------------------------------
def test_blank_at_the_last_class_equals_blank_zero_on_permuted_classes(dev):
  case = PARITY["T17_N3_C3"]
  C = case["C"]
  first = device_run(case, dev)
  moved = dict(case, hyp_ids=case["hyp_ids"] - 1)                      # class c -> c - 1, the blank 0 -> C - 1
  perm = list(range(1, C)) + [0]
  last = device_run(moved, dev, lp_of=lambda lp: lp[..., perm], blank=C - 1)
  assert (first["status"] == last["status"]).all() and (first["status"] == K.USED).any()
  assert torch.equal(first["hyp_ll_t"], last["hyp_ll_t"]) and torch.equal(first["loss_t"], last["loss_t"])
  want = K.oracle(case["logits"][..., perm], case["sizes"], moved["hyp_ids"], case["hyp_lens"], case["risk"],
                  blank=C - 1)
  check_parity(last, want, "blank last")


def _slot_case():
  """One batch with every slot status.  T = 8, C = 6, N = 6, ids 5 wide."""
  rng = np.random.RandomState(3)
  junk = [77, -5, 6, 0, 9]
  ids = np.array([
      [[1, 2, 3, 77, -5], [1, 2, 4, 0, 0], [1, 6, 3, 0, 0], [1, 0, 3, 0, 0], [1, 2, 3, 4, 5], [2, 3, 0, 0, 0]],
      [[1, 1, 1, 1, 1], [3, 4, 0, 0, 0], junk, [5, 0, 0, 0, 0], junk, junk],
      [junk, [0, 1, 0, 0, 0], [-1, 2, 0, 0, 0], junk, [1, 2, 3, 0, 0], junk],
      [[1, 2, 0, 0, 0], junk, [3, 0, 0, 0, 0], junk, junk, junk]], dtype=np.int32)
  lens = np.array([[3, -1, 3, 3, 6, 2],       # used, empty, an id == C, an id == blank, over-long, NaN risk
                   [5, 2, 0, 1, -1, -7],      # infeasible (5 ids + 4 repeats > 8 frames), used, len 0, used, empty, empty
                   [-1, 2, 2, -1, 3, -1],     # no usable slot: empty, blank id, negative id, empty, inf risk, empty
                   [2, 0, 1, -1, -1, -1]],    # sizes == 0: infeasible whatever the length
                  dtype=np.int32)
  risk = rng.randint(0, 5, size=(4, 6)).astype(np.float32)
  risk[0, 5], risk[2, 4] = np.nan, np.inf
  want_status = [[0, 1, 2, 2, 2, 2], [3, 0, 0, 0, 1, 1], [1, 2, 2, 1, 2, 1], [3, 3, 3, 1, 1, 1]]
  case = dict(logits=rng.randn(4, 8, 6).astype(np.float32), sizes=np.array([8, 8, 6, 0], dtype=np.int32), hyp_ids=ids,
              hyp_lens=lens, risk=risk, blank=0, T=8, C=6, N=6, B=4)
  return case, want_status


def test_every_slot_status_in_one_batch(dev):
  case, want_status = _slot_case()
  want = K.run(case)
  assert want["status"].tolist() == want_status       # the restatement reads the specification the same way
  got = device_run(case, dev)
  assert got["status"].tolist() == want_status
  check_parity(got, want, "slots")
  # utterance 0 has ONE used slot, utterances 2 and 3 none: no gradient there; U = 2
  assert (got["grad"][0] == 0).all() and (got["grad"][2:] == 0).all() and np.abs(got["grad"][1]).max() > 0
  assert got["utt_risk"][2] == 0 and got["utt_risk"][3] == 0
  assert abs(got["loss"] - (want["utt_risk"][0] + want["utt_risk"][1]) / 2) <= K.TOL_LOSS * want["loss"]


def test_a_batch_without_a_usable_slot_is_skipped(dev):
  case, _ = _slot_case()
  none = {k: (v[2:] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
  got = device_run(none, dev)
  assert got["batch_status"] == 1 and got["loss"] == 0.0 and (got["grad"] == 0).all()
  assert (got["status"] != K.USED).all() and np.isneginf(got["hyp_ll"]).all()


@pytest.mark.parametrize("B", [1, 4])
def test_one_slot_gives_the_risk_itself_and_no_gradient(dev, B):
  case = K.make_case(11, 17, 65, 1, [8, 3, 0, 12][:B])
  got = device_run(case, dev, reduction='sum')
  assert (got["status"] == K.USED).all()
  assert got["loss"] == float(case["risk"].sum())      # small integers: their sum is exact
  assert (got["grad"] == 0).all()
  if B == 1:
    assert device_run(case, dev, reduction='mean')["loss"] == float(case["risk"][0, 0])


def _raw_grad(case, dev, fill):
  """The two entries called directly, the gradient buffer pre-filled with `fill` (the front door hands the kernel
  torch.empty)."""
  L = _C.lib()
  lp = F.log_softmax(torch.tensor(case["logits"], device=dev), dim=-1)
  B, T, C = lp.shape
  ids = torch.tensor(case["hyp_ids"], device=dev)
  lens = torch.tensor(case["hyp_lens"], device=dev)
  risk = torch.tensor(case["risk"], device=dev)
  sizes = torch.tensor(case["sizes"], device=dev)
  N, W = ids.shape[1], ids.shape[2]
  nbytes = L.lr_ctc_nbest_workspace_bytes(B, T, C, N, W)
  ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
  f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
  hyp_ll, post, utt, loss, gw = f32(B, N), f32(B, N), f32(B), f32(1), f32(B)
  hs = torch.empty((B, N), dtype=torch.int32, device=dev)
  st = torch.empty(1, dtype=torch.int32, device=dev)
  head = (lp.data_ptr(), lp.stride(0), lp.stride(1), sizes.data_ptr(), ids.data_ptr(), ids.stride(0), ids.stride(1),
          lens.data_ptr(), lens.stride(0), risk.data_ptr(), case["blank"], 1)
  tail = (ws.data_ptr(), nbytes, B, T, C, N, W, _C.stream_handle())
  _C.check(L.lr_ctc_nbest_risk(*head, hyp_ll.data_ptr(), post.data_ptr(), hs.data_ptr(), utt.data_ptr(),
                               loss.data_ptr(), st.data_ptr(), gw.data_ptr(), *tail), "lr_ctc_nbest_risk")
  grad = torch.full((B, T, C), fill, dtype=torch.float32, device=dev)
  _C.check(L.lr_ctc_nbest_risk_grad(*head, hyp_ll.data_ptr(), post.data_ptr(), hs.data_ptr(), utt.data_ptr(),
                                    gw.data_ptr(), None, grad.data_ptr(), *tail), "lr_ctc_nbest_risk_grad")
  return grad


def test_every_gradient_element_is_written_and_rows_past_the_sizes_are_zero(dev):
  case = PARITY["T17_N3_C65"]
  grad = _raw_grad(case, dev, float("nan"))
  assert bool(torch.isfinite(grad).all())
  for b, n in enumerate(case["sizes"]):
    assert bool((grad[b, n:] == 0).all())
  assert torch.equal(grad, device_run(case, dev)["grad_t"])      # NULL grad_scale = 1: the front door's gradient
  slots, _ = _slot_case()
  assert bool(torch.isfinite(_raw_grad(slots, dev, float("nan"))).all())


def test_strided_inputs_give_the_same_bits(dev):
  case = PARITY["T75_N3_C65"]
  plain = device_run(case, dev)

  def transposed(lp):                                   # the (B, T, C) view of a (T, B, C) tensor
    return lp.transpose(0, 1).contiguous().transpose(0, 1)

  def sliced(ids, lens):                                # ids[:, :N] / lens[:, :N] of a wider (B, W, T) block
    B, N, W = ids.shape
    wide = torch.full((B, N + 5, W + 3), 1, dtype=ids.dtype, device=ids.device)
    wide[:, :N, :W] = ids
    wide_lens = torch.full((B, N + 5), 2, dtype=lens.dtype, device=lens.device)
    wide_lens[:, :N] = lens
    return wide[:, :N], wide_lens[:, :N]

  got = device_run(case, dev, lp_of=transposed, ids_of=sliced)
  for k in ("loss_t", "hyp_ll_t", "grad_t"):
    assert torch.equal(plain[k], got[k]), k
  assert (plain["status"] == got["status"]).all()


def test_two_launches_are_bit_identical(dev):
  case = PARITY["T76_N16_C65"]
  a, b = device_run(case, dev), device_run(case, dev)
  for k in ("loss_t", "hyp_ll_t", "grad_t"):
    assert torch.equal(a[k], b[k]), k


def test_an_incoming_gradient_of_two_doubles_the_gradient_exactly(dev):
  case = PARITY["T17_N16_C65"]
  one, two = device_run(case, dev), device_run(case, dev, scale=2.0)
  assert float(one["grad_t"].abs().max()) > 0 and torch.equal(two["grad_t"], 2.0 * one["grad_t"])


def test_hyp_ll_against_the_ctc_loss_kernels(dev):
  """-nll of lr_ctc_nll on the same strings, blank 0."""
  from lipreading_amd.ctc import ctc_loss_with_status
  case = K.make_case(21, 17, 65, 1, [1, 1, 2, 7, 8, 15], sizes=[17, 1, 9, 17, 12, 17])
  got = device_run(case, dev)
  lp = F.log_softmax(torch.tensor(case["logits"], device=dev), dim=-1)
  labels = torch.tensor(case["hyp_ids"][:, 0].clip(1, 64) - 1, dtype=torch.int64, device=dev)   # the loss shifts them up again
  _, _, nll = ctc_loss_with_status(lp, labels, torch.tensor(case["sizes"], device=dev),
                                   torch.tensor(case["hyp_lens"][:, 0], device=dev), 'sum')
  err = (got["hyp_ll_t"][:, 0] + nll).abs().max().item()
  print("hyp_ll + nll: %.3e" % err)
  assert (got["status"] == K.USED).all() and err <= LOSS_TOL


# ---- MWERLoss end to end ----------------------------------------------------------------------------------------------
LABELS = ['_'] + list("abcd ")


def _planted(dev):
  """One-hot-ish frames spelling known strings plus noise.  Utterance 0 and 2 decode to their references; utterance
  1's frames spell another string than its reference."""
  spelled = ["ab cd", "ba dc", "a bb"]
  refs = ["ab cd", "bd bc", "a bb"]
  T = 14
  rng = np.random.RandomState(4)
  logits = rng.randn(len(spelled), T, len(LABELS)).astype(np.float32)
  for b, s in enumerate(spelled):
    t = 0
    for i, ch in enumerate(s):
      if i and s[i - 1] == ch:
        logits[b, t, 0] += 5.0
        t += 1
      logits[b, t, LABELS.index(ch)] += 5.0
      t += 1
    logits[b, t:, 0] += 5.0
  width = max(len(r) for r in refs)
  ref_ids = np.zeros((len(refs), width), dtype=np.int32)
  for b, r in enumerate(refs):
    ref_ids[b, :len(r)] = [LABELS.index(c) for c in r]
  ref_lens = np.array([len(r) for r in refs], dtype=np.int32)
  sizes = np.array([T, T - 2, T], dtype=np.int32)
  lp = F.log_softmax(torch.tensor(logits, device=dev), dim=-1)
  return lp, torch.tensor(sizes, device=dev), torch.tensor(ref_ids, device=dev), torch.tensor(ref_lens, device=dev), refs


@pytest.mark.parametrize("unit", ["char", "word"])
def test_mwer_loss_on_planted_log_probs(dev, unit):
  from lipreading_amd.decoder import BeamCTCDecoder
  lp, sizes, ref_ids, ref_lens, refs = _planted(dev)
  dec = BeamCTCDecoder(LABELS, beam_width=8, cutoff_top_n=6, log_probs_input=True)
  N = 4
  x = lp.clone().requires_grad_(True)
  loss, status, info = M.MWERLoss(dec, nbest=N, unit=unit)(x, sizes, ref_ids, ref_lens)
  loss.backward()
  assert int(status.item()) == 0
  # the slots are the decoder's own N best
  ids, _, lens, scores = dec.decode_ids(lp, sizes)
  assert torch.equal(info["hyp_ids"], ids[:, :N])
  found = ~((lens[:, :N] == 0) & torch.isinf(scores[:, :N]))
  assert torch.equal(info["hyp_lens"], torch.where(found, lens[:, :N], torch.full_like(lens[:, :N], -1)))
  # the risks are host Levenshtein distances of the decoded strings
  h_ids, h_lens = info["hyp_ids"].cpu().numpy(), info["hyp_lens"].cpu().numpy()
  risk = np.zeros(h_lens.shape, dtype=np.float32)
  for b in range(h_lens.shape[0]):
    for n in range(N):
      s = ''.join(LABELS[i] for i in h_ids[b, n, :max(h_lens[b, n], 0)])
      risk[b, n] = dec.cer(s, refs[b]) if unit == 'char' else dec.wer(s, refs[b])
  assert np.array_equal(info["risk"].cpu().numpy(), risk)
  assert risk[0, 0] == 0 and risk[2, 0] == 0 and risk[1, 0] > 0      # as planted
  # the loss and the gradient are the restatement's on those slots (log-probabilities are their own log_softmax)
  want = K.oracle(lp.double().cpu().numpy(), sizes.cpu().numpy(), h_ids, h_lens, risk)
  got = dict(loss=float(loss), grad=x.grad.double().cpu().numpy(), hyp_ll=info["hyp_ll"].double().cpu().numpy(),
             status=info["hyp_status"].cpu().numpy())
  assert (got["status"] == want["status"]).all()
  g, l, ll = K.rel_errors(got, want)
  print("planted %s: grad %.3e loss %.3e hyp_ll %.3e" % (unit, g, l, ll))
  assert g <= K.TOL_GRAD and l <= K.TOL_LOSS and ll <= K.TOL_LL


def test_mwer_loss_adds_the_reference_only_where_no_beam_is_exact(dev):
  from lipreading_amd.decoder import BeamCTCDecoder
  lp, sizes, ref_ids, ref_lens, refs = _planted(dev)
  dec = BeamCTCDecoder(LABELS, beam_width=8, cutoff_top_n=6, log_probs_input=True)
  N = 3
  plain = M.MWERLoss(dec, nbest=N)(lp, sizes, ref_ids, ref_lens)[2]
  loss, status, info = M.MWERLoss(dec, nbest=N, with_reference=True)(lp, sizes, ref_ids, ref_lens)
  assert tuple(info["hyp_lens"].shape) == (3, N + 1)
  assert torch.equal(info["hyp_lens"][:, :N], plain["hyp_lens"]) and torch.equal(info["risk"][:, :N], plain["risk"])
  exact = ((plain["risk"] == 0) & (plain["hyp_lens"] >= 0)).any(dim=1).cpu().tolist()
  assert exact == [True, False, True]
  assert info["hyp_lens"][:, N].cpu().tolist() == [-1, len(refs[1]), -1]
  assert info["hyp_status"][:, N].cpu().tolist() == [K.EMPTY, K.USED, K.EMPTY]
  assert info["risk"][:, N].cpu().tolist() == [0.0, 0.0, 0.0]
  assert info["hyp_ids"][1, N, :len(refs[1])].cpu().tolist() == [LABELS.index(c) for c in refs[1]]
  # the reference pulls utterance 1's expected risk down, the others are untouched
  assert float(info["utt_risk"][1]) < float(plain["utt_risk"][1])
  assert torch.equal(info["utt_risk"][[0, 2]], plain["utt_risk"][[0, 2]])


# ---- the step and the driver ------------------------------------------------------------------------------------------
def _small_setup(dev, frames_per_clip=None):
  from lipreading_amd.data import default_char2idx, make_collate_fn
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  c2i = default_char2idx()
  rng = np.random.RandomState(0)
  items = []
  for n in sorted(rng.randint(20, 40, 4)) if frames_per_clip is None else [frames_per_clip] * 4:
    items.append((rng.randn(n, 68, 3).astype(np.float32), np.r_[1, rng.randint(4, 64, 6), 2]))
  batch = make_collate_fn(dev)(items)
  torch.manual_seed(0)
  enc = VideoEncoder(204, 32, rnn_type='GRU', bidirectional=True, enable_ctc=True, vocab_size=64, char2idx=c2i).to(dev)
  opt = FusedAdam(FlatParameters(enc), lr=3e-3)
  dec = BeamCTCDecoder(ctc_labels(c2i), beam_width=8, log_probs_input=True)
  return enc.train(), opt, M.MWERLoss(dec, nbest=4), batch


def test_mwer_step_trains_without_a_host_read(dev):
  from lipreading_amd import train as T
  enc, opt, mwer, (frames, frame_lens, chars, char_lens) = _small_setup(dev)
  before = {k: v.detach().clone() for k, v in enc.named_parameters()}
  for _ in range(3):
    risk, ctc, status, info = T.mwer_step(enc, opt, mwer, frames, frame_lens, chars, char_lens, grad_norm=50)
    assert int(status.item()) == 0 and np.isfinite(float(risk)) and np.isfinite(float(ctc))
  for k, v in enc.named_parameters():
    assert not torch.equal(before[k], v.detach()), k
  # the risk the step returned is nbest_risk_loss on the step's own log-probabilities and slots
  again, st, _ = M.nbest_risk_loss(info["log_probs"], frame_lens.to(dev).to(torch.int32), info["hyp_ids"],
                                   info["hyp_lens"], info["risk"])
  assert int(st.item()) == 0 and torch.equal(again.detach(), risk)


def test_mwer_step_skips_a_batch_whose_references_do_not_fit(dev):
  from lipreading_amd import train as T
  enc, opt, mwer, (frames, frame_lens, chars, char_lens) = _small_setup(dev, frames_per_clip=3)   # 7 labels, 3 frames
  before = {k: v.detach().clone() for k, v in enc.named_parameters()}
  _, _, status, _ = T.mwer_step(enc, opt, mwer, frames, frame_lens, chars, char_lens, grad_norm=50)
  assert int(status.item()) == 1 and opt.skipped_steps() == 1
  for k, v in enc.named_parameters():
    assert torch.equal(before[k], v.detach()), k


def test_driver_trains_with_mwer(dev, tmp_path, capsys):
  from lipreading_amd import driver
  from lipreading_amd.dataset import write_synthetic_dataview
  root = str(tmp_path)
  write_synthetic_dataview(root, "StephenColbert/micro", n_videos=6, captions_per_video=5, seed=11)
  flags = driver.parse_flags(["--data=StephenColbert/micro", "--batch_size=5", "--enable_ctc=True", "--ctc_only=True",
                              "--rnn_type=GRU", "--bidirectional=True", "--hidden_size=32", "--learning_rate=3e-4",
                              "--grad_norm=400", "--cuda=True", "--ctc_decoder=beam", "--beam_width=8", "--mwer=4",
                              "--root=" + root, "--max_epochs=1"])
  out = driver.run(**flags)
  text = capsys.readouterr().out
  h = out["history"]
  assert len(h) == 1 and np.isfinite(h[0]["expected_risk"]) and h[0]["expected_risk"] > 0
  assert np.isfinite(h[0]["ctc_loss"]) and 0.0 <= h[0]["val_cer"] <= 2.0
  assert "Training expected risk: " in text and "AVG Expected Risk: " in text
