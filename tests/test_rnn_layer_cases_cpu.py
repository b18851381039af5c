"""tests/rnn_layer_cases.py is what tests/test_gpu_rnn_fp64.py takes it for (no GPU): both references are finite, the
float32 yardstick is good enough for 4 x its error to mean something, the lengths are ragged, the saturated cases
saturate, every case sits on the dispatch branch it names — and a reference that is deliberately wrong is caught by the
bounds the GPU test applies.

The float32 CPU layer's worst error against float64 per case, relative to the tensor's largest entry, measured over the
table on an Intel host (MKL's AVX-512 kernels): 4.9e-8 (the single frame) .. 6.0e-7, the saturated cases 1.5e-7 .. 2.0e-7;
the 2e-6 asked of it below leaves a factor of three.  The figure belongs to the host's BLAS, not to the layer: on an AMD
EPYC host MKL sums the 4624 terms of the two grid cases' dx = dG . W_ih (I = 8) in another order and that one tensor comes
out at 2.17e-6 (grid_lstm1156) and 1.60e-6 (grid_lstm1400_uni), at any thread count, with or without oneDNN; every other
tensor of the table stays below 6.1e-7 there too.  So on such a host test_references_..._is_tight[grid_lstm1156] misses its
2e-6 by a tenth; the GPU test takes the yardstick of the host it runs on, and dx of those cases is held by the one-launch
path's 1e-4 there, of which the device uses 7.5e-7."""
import pytest
import torch

from tests import rnn_layer_cases as C


@pytest.mark.parametrize("name", list(C.CASES))
def test_references_are_finite_and_the_yardstick_is_tight(name):
  case = C.CASES[name]
  want64, cpu32 = C.reference(name)
  assert sorted(want64) == sorted(cpu32) == sorted(C.tensor_names(case))
  worst = 0.0
  for k in C.tensor_names(case):
    assert want64[k].dtype == torch.float64 and cpu32[k].dtype == torch.float32
    assert torch.isfinite(want64[k]).all() and torch.isfinite(cpu32[k]).all(), k
    err, _ = C.figures(cpu32[k], want64[k])
    worst = max(worst, err)
    # what keeps 4 x the figure a bound that a wrong element cannot hide under
    assert err <= 2e-6, (k, err)
    elem, norm = C.bounds(case, k, err)
    if C.exact(case):
      assert elem == 4 * max(err, C.ULP) and norm is None      # hold()'s rule, nothing added
  print("%-24s float32 CPU against float64: worst %.2e" % (name, worst))


@pytest.mark.parametrize("name", list(C.CASES))
def test_lengths_are_ragged(name):
  case, lens = C.CASES[name], C.inputs(name).lens.tolist()
  assert len(lens) == case.B and all(1 <= n <= case.T for n in lens)
  assert case.T in lens
  assert lens[case.B - 1] == case.T      # the last tile of 16 / group of 8 samples holds a full-length one
  if case.B >= 3:
    assert 1 in lens
  if case.B >= 2 and case.T >= 2:
    assert len(set(lens)) > 1
  # the padded frames of x hold real values (the layer must not read them), and the garbage for them is large
  if case.B >= 2 and case.T >= 2:
    pad = ~C.valid_mask(name).expand_as(C.inputs(name).x)
    assert pad.any() and float(C.inputs(name).x[pad].abs().max()) > 0
    assert float(C.x_with_garbage(name)[pad].abs().min()) >= 1e3
    assert torch.equal(C.x_with_garbage(name)[~pad], C.inputs(name).x[~pad])


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if c.saturated])
def test_saturated_cases_saturate(name):
  """|pre-activation| > 44 in float64, both signs, in every gate block: past where exp2(2.885 x) overflows."""
  case, inp = C.CASES[name], C.inputs(name)
  G, H = C.GATES[case.cell], case.H
  for d in range(case.D):
    t0 = 0 if d == 0 else int(inp.lens[0]) - 1       # the direction's first step of sample 0: h = 0
    pre = inp.w_ih[d].double() @ inp.x[0, t0].double() + inp.b_ih[d].double() + inp.b_hh[d].double()
    for g in range(G):
      blk = pre[g * H:(g + 1) * H]
      assert float(blk.max()) > 44 and float(blk.min()) < -44, (d, g)


def _expected_branches(case):
  """lr_rnn_layer_forward / rnn_layer_backward_impl / resolve_shape, restated."""
  G, H, I, D = C.GATES[case.cell], case.H, case.I, case.D
  GH = G * H
  x3, split, exact_in = C.X3 in case.flags, C.SPLIT in case.flags, C.EXACT in case.flags
  recur = "step"
  if split:
    assert case.cell != "RNN" and H % 4 == 0
    c32, c16 = (H + 31) // 32, (H + 15) // 16
    c16 += c16 & 1
    if G == 4 and 1152 < H <= 1536:
      recur = "grid"
    elif c32 <= (27 if G == 3 else 24):
      recur = "cluster32:%d" % c32
    else:
      assert (56 if G == 3 else 50) <= c16 <= 72
      recur = "cluster16:%d" % c16
  if x3:
    proj = "xproj" if exact_in else "fgemm_x3"
    assert I <= 1024
  elif I % 4 == 0:
    proj = "fgemm_x3" if split and GH >= 1536 else "fgemm_f32"
  elif D == 2 and case.offset % 4 == 0:
    proj = "sgemm_batched"
  else:
    proj = "sgemm_each"
  wgrad = "fgemm" if x3 else ("fgemm_splitk" if split else "grouped")
  return proj, wgrad, recur


@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_sit_on_the_branches_they_name(name):
  case = C.CASES[name]
  assert case.H % 4 == 0 and case.D in (1, 2) and case.offset in (0, 1)
  assert (case.proj, case.wgrad, case.recur) == _expected_branches(case)


def _wgrad_k_splits(case):
  """wgrad_fgemm_plan (lr_rnn.hip), restated: into how many ranges a RECUR_SPLIT layer's weight half cuts K = B * T."""
  G, H, I, D, R = C.GATES[case.cell], case.H, case.I, case.D, case.B * case.T
  jobs = [(G * H, I), (2 * H, H), (H, H)] if G == 3 else [(G * H, I), (G * H, H)]
  tiles = D * sum(((m + 127) // 128) * ((n + 127) // 128) for m, n in jobs)
  return max(1, min(384 // tiles, ((R + 31) // 32) // 8, 16))


def test_every_branch_has_a_case():
  splits = {n: _wgrad_k_splits(c) for n, c in C.CASES.items() if c.wgrad == "fgemm_splitk"}
  assert splits["split_gru40_k_split"] == 2 and C.CASES["split_gru40_k_split"].I % 4 != 0
  assert all(v == 1 for n, v in splits.items() if n != "split_gru40_k_split")
  have = {(c.proj, c.I % 4 != 0) for c in C.CASES.values()}
  assert {("sgemm_batched", True), ("sgemm_each", True), ("fgemm_f32", False), ("fgemm_x3", False), ("xproj", False)} <= have
  assert any(c.proj == "sgemm_each" and c.D == 2 and c.offset == 1 for c in C.CASES.values())
  assert any(c.proj == "sgemm_each" and c.D == 1 for c in C.CASES.values())
  # odd I through each of the two weight-gradient forms and both dx products
  assert {c.wgrad for c in C.CASES.values() if c.I % 4} == {"grouped", "fgemm_splitk"}
  recur = {c.recur.split(":")[0] for c in C.CASES.values()}
  assert recur == {"step", "cluster32", "cluster16", "grid"}
  for name in C.PROPERTY_CASES + [C.GRID_CASE, C.LSTM_STEP_CASE]:
    assert name in C.CASES
  assert C.CASES[C.GRID_CASE].recur == "grid" and C.CASES[C.LSTM_STEP_CASE].recur == "step"


@pytest.mark.parametrize("name,wrong", [(n, w) for n, c in C.CASES.items() for w in C.WRONG if C.applies(w, c)])
def test_a_wrong_reference_is_caught(name, wrong):
  """The GPU test's bounds against a reference that is NOT the layer: the float32 CPU result (a stand-in for a correct
  device) must fall outside them — in y, and so in test_layer_matches_float64."""
  case = C.CASES[name]
  want64, cpu32 = C.reference(name)
  bad64 = C.evaluate(name, torch.float64, wrong=wrong)
  caught = []
  for k in C.tensor_names(case):
    cpu_err, _ = C.figures(cpu32[k], want64[k])
    elem, norm = C.bounds(case, k, cpu_err)
    err, nerr = C.figures(cpu32[k], bad64[k])
    if err > elem or (norm is not None and nerr > norm):
      caught.append(k)
  assert "y" in caught and len(caught) >= 3, caught
