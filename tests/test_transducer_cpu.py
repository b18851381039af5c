"""No GPU: the float64 restatement of the transducer (tests/transducer_cases.py) against brute force and against
itself, the conditions the GPU tests put on their cases, and the driver's --transducer flag checks."""
import pytest
import torch

from tests import transducer_cases as K


def _tiny(T, U, V1=4, J=3, seed=0, mask_class=None):
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  mask = torch.ones(V1, dtype=torch.float64)
  if mask_class is not None:
    mask[mask_class] = 0
  allowed = [c for c in range(1, V1) if mask[c] != 0]
  labels = torch.tensor([[allowed[int(i)] for i in torch.randint(0, len(allowed), (max(U, 1),), generator=g)]][0][:U],
                        dtype=torch.int32)[None]
  return dict(e=r(1, T, J), p=r(1, U + 1, J), W=r(V1, J), b=r(V1), mask=mask, labels=labels)


@pytest.mark.parametrize("T,U", [(3, 2), (4, 1)])
def test_the_recursion_equals_the_sum_over_all_alignments(T, U):
  c = _tiny(T, U)
  lp = K.joint_log_probs(c["e"], c["p"], c["W"], c["b"], c["mask"])[0]
  want = K.brute_force_nll(lp, c["labels"][0], T, U)
  got = K.lattice_nll(lp, c["labels"][0], T, U)
  assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))


def test_without_labels_the_loss_is_the_blank_path():
  c = _tiny(5, 0)
  lp = K.joint_log_probs(c["e"], c["p"], c["W"], c["b"], c["mask"])[0]
  got = K.lattice_nll(lp, c["labels"][0], 5, 0)
  assert abs(float(got) + float(lp[:, 0, 0].sum())) <= 1e-12


def test_masked_classes_carry_no_probability_and_no_gradient():
  c = _tiny(4, 2, V1=5, mask_class=2)
  W, b = c["W"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
  lp = K.joint_log_probs(c["e"], c["p"], W, b, c["mask"])
  assert bool((lp[..., 2] == float("-inf")).all())
  assert abs(float(lp.detach().exp().sum(-1).max()) - 1.0) <= 1e-12
  loss, status, _, stats = K.rnnt_loss(c["e"], c["p"], W, b, c["mask"], c["labels"], [4], [2])
  loss.backward()
  assert status == 0 and stats == [0]
  assert not W.grad[2].any() and float(b.grad[2]) == 0.0 and bool(W.grad[0].any())


def test_autograd_equals_the_occupancy_formula():
  c = _tiny(4, 3, V1=5, J=4, seed=2)
  z = torch.tanh(c["e"][:, :, None, :] + c["p"][:, None, :, :])
  logits = (z @ c["W"].t() + c["b"]).detach().requires_grad_(True)
  lp = torch.log_softmax(logits, -1)[0]
  K.lattice_nll(lp, c["labels"][0], 4, 3).backward()
  want = K.occupancy_grad(lp.detach(), c["labels"][0], 4, 3)
  assert float((logits.grad[0] - want).abs().max()) <= 1e-12
  # a ragged sample inside a larger tensor: nodes outside (T_b, U_b) get nothing
  logits.grad = None
  lp = torch.log_softmax(logits, -1)[0]
  K.lattice_nll(lp, c["labels"][0], 3, 2).backward()
  want = K.occupancy_grad(lp.detach(), c["labels"][0], 3, 2)
  assert float((logits.grad[0] - want).abs().max()) <= 1e-12
  assert not logits.grad[0, 3:].any() and not logits.grad[0, :, 3:].any()


def test_status_rules():
  mask = torch.ones(6)
  mask[4] = 0
  lab = torch.tensor([1, 2, 3])
  assert K.sample_status(5, 3, lab, 5, 3, 6, mask) == 0
  assert K.sample_status(1, 0, lab, 5, 3, 6, mask) == 0
  for Tb, Ub in ((0, 1), (6, 1), (3, -1), (3, 4)):
    assert K.sample_status(Tb, Ub, lab, 5, 3, 6, mask) == K.BAD_LENGTH
  for bad in (0, 6, 4, -1):
    assert K.sample_status(5, 3, torch.tensor([1, bad, 3]), 5, 3, 6, mask) == K.BAD_ID
    assert K.sample_status(5, 1, torch.tensor([1, bad, 3]), 5, 3, 6, mask) == 0      # past the length: never read
  c = _tiny(3, 2)
  e, p = c["e"].repeat(2, 1, 1).requires_grad_(True), c["p"].repeat(2, 1, 1)
  labels = c["labels"].repeat(2, 1)
  labels[1, 0] = 0
  loss, status, nll, stats = K.rnnt_loss(e, p, c["W"], c["b"], c["mask"], labels, [3, 3], [2, 2])
  loss.backward()
  assert stats == [0, K.BAD_ID] and status == 0 and float(nll[1].detach()) == 0.0 and float(loss.detach()) == float(nll[0].detach())
  assert not e.grad[1].any() and bool(e.grad[0].any())
  _, status, _, _ = K.rnnt_loss(e, p, c["W"], c["b"], c["mask"], labels, [0, 3], [2, 2])
  assert status == 1


def _greedy_case(T=9, seed=4):
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  mask = torch.ones(7, dtype=torch.float64)
  mask[3] = 0
  b = r(7)
  b[0] += 1.5
  return dict(e=r(2, T, 6), tables=r(2, 7, 6), W=r(7, 6) * 2, b=b, mask=mask)


def _run(c, sizes, **kw):
  return K.greedy(c["e"], sizes, c["tables"], c["W"], c["b"], c["mask"], **kw)


def test_chunked_greedy_equals_one_shot_for_every_cut():
  c = _greedy_case()
  sizes = torch.tensor([9, 6])
  whole = _run(c, sizes)
  assert sum(whole["lens"]) > 0 and 3 not in [k for row in whole["ids"] for k in row]
  for cut in range(0, 10):
    st = None
    for t0, t1 in ((0, cut), (cut, 9)):
      part = dict(c, e=c["e"][:, t0:t1])
      if t1 > t0:
        st = _run(part, (sizes - t0).clamp(0, t1 - t0), state=st, max_out=45)
    assert st == dict(whole, max_out=45), cut


def test_greedy_cap_and_forced_count():
  c = _greedy_case()
  c["b"][0] = -50.0
  out = _run(c, torch.tensor([9, 4]), max_symbols=2)
  assert out["lens"] == [18, 8] and out["forced"] == [9, 4]
  assert out["frames"][1] == [0, 0, 1, 1, 2, 2, 3, 3]
  out = _run(c, torch.tensor([9, 4]), max_symbols=2, max_out=5)
  assert out["lens"] == [18, 8] and [len(r) for r in out["ids"]] == [5, 5]
  c["b"][0] = 50.0
  out = _run(c, torch.tensor([9, 4]))
  assert out["lens"] == [0, 0] and out["forced"] == [0, 0]


def test_a_tie_goes_to_the_lowest_class():
  c = _greedy_case()
  c["W"] = torch.zeros_like(c["W"])
  c["b"] = torch.tensor([0.0, 1.0, -1.0, 9.0, 1.0, 0.5, 1.0], dtype=torch.float64)   # class 3 is masked; 1, 4, 6 tie
  out = _run(c, torch.tensor([2, 1]), max_symbols=2)
  assert out["ids"] == [[1, 1, 1, 1], [1, 1]]
  c["b"][0] = 1.0                                                                      # the blank ties too, and is lowest
  assert _run(c, torch.tensor([2, 1]))["lens"] == [0, 0]


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_named_case_meets_the_margin_condition(name):
  _, margin, err = K.greedy_reference(name)
  assert margin >= K.MARGIN_FACTOR * max(err, K.FP32_ERROR[name][6]), (name, margin, err)
  assert set(K.FP32_ERROR) == set(K.CASES)


def test_driver_flag_checks():
  from lipreading_amd import driver
  base = ["--enable_ctc=True", "--ctc_only=True", "--transducer=True"]
  f = driver.parse_flags(base)
  assert f["transducer"] and f["transducer_joint"] == 256 and f["transducer_embed"] == 64
  assert f["transducer_context"] == 2 and f["transducer_ctc_weight"] == 0.3 and f["transducer_max_symbols"] == 5
  assert driver.parse_flags(["--transducer=True", "--encoder=transformer"])["transducer"]
  assert driver.parse_flags(["--transducer=True", "--frontend=conv3d"])["transducer"]
  assert not driver.parse_flags([])["transducer"]
  for extra in (["--ctc_only=False"], ["--ctc_decoder=beam", "--mwer=4"], ["--ctc_decoder=beam", "--stream_chunk=5"],
                ["--attn_decode=beam"], ["--transducer_context=3"], ["--transducer_joint=513"],
                ["--transducer_max_symbols=0"], ["--transducer_ctc_weight=-1"], ["--score=device"],
                ["--encoder=transformer", "--tfm_chunk=4", "--ctc_decoder=beam", "--stream_chunk=4", "--stream_tfm=True"]):
    with pytest.raises(ValueError, match="transducer"):
      driver.parse_flags(base + extra)
  with pytest.raises(ValueError, match="transducer"):
    driver.parse_flags(["--transducer=True"])             # the landmark RNN regime without the CTC loop
