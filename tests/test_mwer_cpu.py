"""CPU: the restatement of the N-best minimum error rate objective (tests/mwer_cases.py) against finite differences and
its own invariants; what the front door, the driver and the workspace query refuse.  No device call."""
import numpy as np
import pytest
import torch

from lipreading_amd import _C, driver
from lipreading_amd import mwer as M
from tests import mwer_cases as K


def _mixed_case():
  """Three utterances: ragged sizes, an empty slot, a len = 0 hypothesis, an infeasible hypothesis."""
  rng = np.random.RandomState(5)
  B, T, C, N, W = 3, 7, 5, 3, 5
  logits = rng.randn(B, T, C)
  ids = np.array([[[1, 2, 2, 0, 0], [1, 3, 0, 0, 0], [9, 9, 9, 9, 9]],
                  [[4, 0, 0, 0, 0], [7, 7, 7, 7, 7], [4, 1, 0, 0, 0]],
                  [[2, 2, 2, 1, 0], [2, 1, 0, 0, 0], [2, 3, 1, 0, 0]]], dtype=np.int32)
  lens = np.array([[3, 2, -1], [1, 0, 2], [4, 2, 3]], dtype=np.int32)    # (2,0): 4 ids + 2 repeats > 5 frames
  risk = np.array([[2.0, 1.0, 5.0], [0.0, 1.0, 3.0], [4.0, 1.0, 2.0]])
  return dict(logits=logits, sizes=np.array([7, 4, 5]), hyp_ids=ids, hyp_lens=lens, risk=risk, blank=0)


def test_restatement_agrees_with_central_finite_differences():
  c = _mixed_case()
  res = K.run(c)
  assert res["status"].tolist() == [[0, 0, 1], [0, 0, 0], [3, 0, 0]]
  assert np.isneginf(res["hyp_ll"][0, 2]) and np.isneginf(res["hyp_ll"][2, 0])
  rng = np.random.RandomState(0)
  h = 1e-6
  for _ in range(12):
    b, t, k = rng.randint(3), rng.randint(7), rng.randint(5)
    if t >= c["sizes"][b]:
      assert res["grad"][b, t, k] == 0.0
      continue
    up, down = dict(c), dict(c)
    up["logits"], down["logits"] = c["logits"].copy(), c["logits"].copy()
    up["logits"][b, t, k] += h
    down["logits"][b, t, k] -= h
    numeric = (K.run(up)["loss"] - K.run(down)["loss"]) / (2 * h)
    assert abs(numeric - res["grad"][b, t, k]) <= 1e-6 * max(abs(numeric), np.abs(res["grad"]).max()), (b, t, k)


def test_restatement_invariants():
  c = _mixed_case()
  res = K.run(c)
  assert np.abs(res["grad"].sum(axis=2)).max() < 1e-12                      # every row sums to zero over the classes
  for b, n in enumerate(c["sizes"]):
    assert (res["grad"][b, n:] == 0).all()                                  # nothing past the utterance's frames
  np.testing.assert_allclose(res["posterior"].sum(axis=1), 1.0, rtol=1e-12)
  flat = dict(c, risk=np.full((3, 3), 2.5))
  res = K.run(flat)                                                          # a constant risk: nothing to learn
  assert abs(res["loss"] - 2.5) < 1e-12 and np.abs(res["grad"]).max() < 1e-12
  one = dict(c, hyp_ids=c["hyp_ids"][:, 1:2], hyp_lens=c["hyp_lens"][:, 1:2], risk=c["risk"][:, 1:2])
  res = K.oracle(one["logits"], one["sizes"], one["hyp_ids"], one["hyp_lens"], one["risk"], reduction='sum')
  assert res["loss"] == 3.0 and (res["grad"] == 0).all()                    # one slot: the risk itself, no gradient
  none = dict(c, hyp_lens=np.full((3, 3), -1))
  res = K.run(none)
  assert res["batch_status"] == 1 and res["loss"] == 0.0 and (res["grad"] == 0).all()


def test_float32_restatement_stays_within_the_recorded_e32():
  """The constants behind the GPU tolerances are this evaluation's errors (a sample: the case that set the maximum and
  a small one)."""
  cases = dict(K.parity_cases())
  for name in ("T76_N16_C65", "T17_N3_C3"):
    r64, r32 = K.run(cases[name]), K.run(cases[name], dtype=torch.float32)
    K.assert_spread(r64, cases[name]["N"])
    g, l, ll = K.rel_errors(r32, r64)
    assert g <= 1.5 * K.E32_GRAD and l <= 1.5 * K.E32_LOSS and ll <= 1.5 * K.E32_LL, (name, g, l, ll)


def test_front_door_refuses_cpu_tensors_and_bad_shapes():
  lp = torch.zeros(2, 5, 7)
  ids = torch.zeros(2, 3, 4, dtype=torch.int32)
  lens = torch.zeros(2, 3, dtype=torch.int32)
  risk = torch.zeros(2, 3)
  with pytest.raises(_C.LipReadingHipError):
    M.nbest_risk_loss(lp, None, ids, lens, risk)


@pytest.mark.parametrize("change, match", [
    (dict(reduction="none"), "reduction"),
    (dict(ids=(2, 17, 4), lens=(2, 17), risk=(2, 17)), "at most 16"),
    (dict(lens=(2, 4)), "hyp_lens and risk"),
    (dict(risk=(3, 3)), "hyp_lens and risk"),
    (dict(ids=(3, 3, 4)), "hyp_ids"),
    (dict(lp=(2, 5)), "log_probs"),
    (dict(ids=(2, 3, 300)), "at most 256"),
    (dict(blank=7), "blank_index"),
])
def test_front_door_shape_checks(monkeypatch, change, match):
  monkeypatch.setattr(_C, "require_cuda", lambda *t: None)    # the checks under test come before any device call
  lp = torch.zeros(change.get("lp", (2, 5, 7)))
  ids = torch.zeros(change.get("ids", (2, 3, 4)), dtype=torch.int32)
  lens = torch.zeros(change.get("lens", (2, 3)), dtype=torch.int32)
  risk = torch.zeros(change.get("risk", (2, 3)))
  with pytest.raises(ValueError, match=match):
    M.nbest_risk_loss(lp, None, ids, lens, risk, blank_index=change.get("blank", 0),
                      reduction=change.get("reduction", "mean"))


def test_mwer_loss_checks_its_decoder():
  from lipreading_amd.decoder import BeamCTCDecoder
  labels = ['_'] + list("abc ")
  with pytest.raises(ValueError, match="log_probs_input"):
    M.MWERLoss(BeamCTCDecoder(labels, beam_width=8), nbest=4)
  dec = BeamCTCDecoder(labels, beam_width=8, log_probs_input=True)
  with pytest.raises(ValueError, match="beam_width"):
    M.MWERLoss(dec, nbest=9)
  with pytest.raises(ValueError, match="unit"):
    M.MWERLoss(dec, nbest=4, unit="phone")
  with pytest.raises(ValueError, match="slots"):
    M.MWERLoss(BeamCTCDecoder(labels, beam_width=32, log_probs_input=True), nbest=16, with_reference=True)
  loss = M.MWERLoss(dec, nbest=4, unit="word", with_reference=True)
  assert loss.scorer is not dec.scorer() and loss.nbest == 4
  with pytest.raises(_C.LipReadingHipError):
    loss(torch.zeros(1, 4, 5), None, torch.zeros(1, 2, dtype=torch.int32), torch.tensor([2], dtype=torch.int32))


def test_driver_flags():
  f = driver.parse_flags(["--mwer=4", "--ctc_decoder=beam", "--ctc_only=True", "--enable_ctc=True",
                          "--mwer_ctc_weight=0.05", "--mwer_unit=word", "--mwer_reference=True", "--beam_width=8"])
  assert (f["mwer"], f["mwer_ctc_weight"], f["mwer_unit"], f["mwer_reference"]) == (4, 0.05, "word", True)
  d = driver.parse_flags([])
  assert (d["mwer"], d["mwer_ctc_weight"], d["mwer_unit"], d["mwer_reference"]) == (0, 0.01, "char", False)
  with pytest.raises(ValueError, match="ctc_decoder=beam"):
    driver.parse_flags(["--mwer=4", "--ctc_only=True", "--enable_ctc=True"])
  with pytest.raises(ValueError, match="CTC-only"):
    driver.parse_flags(["--mwer=4", "--ctc_decoder=beam", "--enable_ctc=True"])
  with pytest.raises(ValueError, match="beam_width"):
    driver.parse_flags(["--mwer=4", "--ctc_decoder=beam", "--ctc_only=True", "--enable_ctc=True", "--beam_width=3"])
  with pytest.raises(ValueError, match="between 1 and 15"):
    driver.parse_flags(["--mwer=16", "--mwer_reference=True", "--ctc_decoder=beam", "--ctc_only=True",
                        "--enable_ctc=True"])
  with pytest.raises(ValueError, match="mwer_unit"):
    driver.parse_flags(["--mwer_unit=phone"])
  # a pixel / transformer regime is encoder + CTC by itself
  assert driver.parse_flags(["--mwer=2", "--ctc_decoder=beam", "--encoder=transformer"])["mwer"] == 2


def test_train_step_refuses_data_parallel():
  from lipreading_amd import train as T
  with pytest.raises(NotImplementedError, match="data-parallel MWER is not built"):
    T.mwer_step(None, None, None, None, None, None, None, grad_sync=object())


def test_workspace_query_returns_zero_past_each_limit():
  L = _C.lib()
  ok = L.lr_ctc_nbest_workspace_bytes(32, 75, 65, 16, 75)
  S = 152                                                  # 2 * 75 + 1 states, rounded up to 8
  assert ok == 2 * 32 * 16 * 75 * S * 8 + 2 * 32 * 16 * 8
  assert L.lr_ctc_nbest_workspace_bytes(1, 1, 1, 1, 0) > 0
  assert L.lr_ctc_nbest_workspace_bytes(2, 300, 256, 16, 256) > 0
  for bad in ((0, 75, 65, 4, 75), (32, 0, 65, 4, 75), (32, 75, 0, 4, 75), (32, 75, 257, 4, 75), (32, 75, 65, 0, 75),
              (32, 75, 65, 17, 75), (32, 75, 65, 4, 257), (32, 75, 65, 4, -1)):
    assert L.lr_ctc_nbest_workspace_bytes(*bad) == 0, bad


def test_null_and_invalid_arguments_are_rejected_without_a_device():
  L = _C.lib()
  one = 4096                                               # any non-NULL value: the checks return before a pointer is used
  # log_probs, strides, sizes | hyps, strides | lens, stride | risk | blank, reduction | 7 outputs | ws, bytes | shape
  def fwd(lp=one, hyps=one, lens=one, risk=one, blank=0, reduction=1, outs=(one,) * 7, ws=one, ws_bytes=1 << 40,
          shape=(2, 5, 7, 3, 4), stride_t=7):
    return L.lr_ctc_nbest_risk(lp, 35, stride_t, None, hyps, 12, 4, lens, 3, risk, blank, reduction, *outs, ws,
                               ws_bytes, *shape, None)
  assert fwd(lp=None) == _C.LR_ERR_INVALID_ARG
  assert fwd(hyps=None) == _C.LR_ERR_INVALID_ARG and fwd(lens=None) == _C.LR_ERR_INVALID_ARG
  assert fwd(risk=None) == _C.LR_ERR_INVALID_ARG and fwd(ws=None) == _C.LR_ERR_INVALID_ARG
  for i in range(7):
    outs = [one] * 7
    outs[i] = None
    assert fwd(outs=outs) == _C.LR_ERR_INVALID_ARG, i
  assert fwd(blank=7) == _C.LR_ERR_INVALID_ARG and fwd(blank=-1) == _C.LR_ERR_INVALID_ARG
  assert fwd(reduction=2) == _C.LR_ERR_INVALID_ARG
  assert fwd(stride_t=-1) == _C.LR_ERR_INVALID_ARG
  assert fwd(ws_bytes=16) == _C.LR_ERR_WORKSPACE
  assert fwd(shape=(2, 5, 7, 17, 4)) == _C.LR_ERR_UNSUPPORTED
  # the gradient entry: the forward's five outputs, grad_weight, grad_scale (may be NULL), grad
  def bwd(grad=one, gw=one, lp=one):
    return L.lr_ctc_nbest_risk_grad(lp, 35, 7, None, one, 12, 4, one, 3, one, 0, 1, one, one, one, one, gw, None, grad,
                                    one, 1 << 40, 2, 5, 7, 3, 4, None)
  assert bwd(grad=None) == _C.LR_ERR_INVALID_ARG and bwd(gw=None) == _C.LR_ERR_INVALID_ARG
  assert bwd(lp=None) == _C.LR_ERR_INVALID_ARG
