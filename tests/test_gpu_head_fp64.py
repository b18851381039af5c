"""The output head and the token loss against float64, path by path (lr_proj.hip through lr_proj_logsoftmax_forward /
_backward, the three products it hands to lr_sgemm, encoder._ProjLogSoftmaxFunction through autograd, and the lr_nll_*
entry points of lr_misc.hip; the cases, the float64 formulas and the ABI helpers are tests/head_cases.py, held to what they
claim by tests/test_head_cases_cpu.py).

Part 1: every element of log_probs of every forward case, the fused kernel and the fallback chain, with a NaN guard band
behind the output and a 0xFF workspace; the two refusals.  Part 2: dlogits, dhidden, dW and dbias of every backward case,
with dhidden given and NULL, accumulate = 0 into NaN and accumulate = 1 on top of seeded values.  Part 3: the head's three
products through lr_sgemm with padded leading dimensions, misaligned bases and two workspace sizes.  Part 4: the autograd
wrapper on contiguous, sliced and transposed `hidden`, and two backward passes into a FlatParameters buffer.  Part 5: the
token loss, its two backward kernels, the all-PAD batch, and train.decoder_nll / decoder_nll_sum on a strided label view.

No bound here was tuned to a device result.  Everything is held by hold()'s rule: element-wise, relative to the float64
tensor's largest entry, 4 x the error the same formula makes in float32 torch on the CPU on the same case, never less than
4 ulp of fp32.  log_probs is held on the unmasked and on the masked columns separately: the masked entries sit near -103
and would otherwise set the scale for the others.

Measured on the MI355X: the range over the path's tensors of the float32 CPU figure and of the device's, then the path's
worst tensor by the share of its bound it uses, as (CPU fp32 figure, bound, device figure).  No kernel bug came out of
these cases: every tensor of every kernel sits inside its bound, at 0.58 of it at the most.  That most is the all-masked
rows, where the kernels round bias + (-103.28) and then add the product, two roundings at 103 where the formula has one.
                                  CPU fp32           device
  forward fused, unmasked         0 .. 1.6e-7        0 .. 1.7e-7       k512_r33_c128       (1.34e-7, 5.35e-7, 1.66e-7)
  forward fused, masked           6.5e-8 .. 8.8e-8   5.7e-8 .. 1.0e-7  k48_r15_c15         (6.47e-8, 4.77e-7, 1.04e-7)
  forward fused, all masked       4.3e-7 .. 5.7e-7   1.0e-6 .. 1.2e-6  k80_r33_c256        (4.32e-7, 1.73e-6, 9.96e-7)
  forward fused, saturated        2.4e-7 .. 3.1e-7   1.4e-7 .. 1.5e-7  k64_r17_c65_sat     (2.41e-7, 9.64e-7, 1.42e-7)
  forward fallback, unmasked      0 .. 1.5e-7        0 .. 1.4e-7       k72_r16_c129        (1.03e-7, 4.77e-7, 1.28e-7)
  forward fallback, masked        5.7e-8 .. 8.8e-8   6.4e-8 .. 1.0e-7  k520_r50_c256       (7.57e-8, 4.77e-7, 1.02e-7)
  forward fallback, all masked    5.3e-7             8.7e-7            k40_r5_c17_all      (5.31e-7, 2.12e-6, 8.70e-7)
  fused against fallback, same data: 9.2e-8 apart on the unmasked columns, the same bits on the masked ones
  backward fused                  0 .. 4.3e-7        0 .. 4.5e-7       r17_k64_c8 dW       (1.34e-7, 5.36e-7, 1.68e-7)
  backward fused, saturated       9.1e-8 .. 4.2e-7   1.5e-8 .. 4.3e-7  r17_k64_c65_sat dW  (1.20e-7, 4.79e-7, 1.30e-7)
  backward chain                  4.8e-8 .. 3.6e-7   4.3e-8 .. 2.9e-7  r50_k520_c256 dbias (8.98e-8, 4.77e-7, 1.60e-7)
  ... accumulate = 1, fused       0 .. 4.0e-7        0 .. 2.0e-7       r16_k65_c128 dbias  (1.13e-7, 4.77e-7, 1.62e-7)
  ... accumulate = 1, chain       9.3e-8 .. 3.0e-7   1.1e-7 .. 3.0e-7  r50_k520_c256 dbias (9.32e-8, 4.77e-7, 1.59e-7)
  lr_sgemm NT + bias              2.4e-8 .. 2.7e-7   2.4e-8 .. 2.6e-7  16x129x72           (2.62e-7, 1.05e-6, 2.62e-7)
  lr_sgemm NN                     2.8e-7 .. 3.8e-7   1.9e-7 .. 2.5e-7  50x520x256          (2.79e-7, 1.12e-6, 2.25e-7)
  lr_sgemm TN, beta = 1           1.1e-7 .. 2.1e-7   1.1e-7 .. 2.1e-7  256x63x33           (1.68e-7, 6.70e-7, 1.68e-7)
  autograd wrapper (after its fix) 7.3e-8 .. 3.4e-7  6.4e-8 .. 3.0e-7  k144_r33_c65 transposed dhidden (2.26e-7, 9.02e-7, 3.03e-7)
  token loss: loss, sum           0 .. 1.2e-7        0 .. 1.2e-7       n3000_v68 sum       (1.17e-7, 4.77e-7, 1.17e-7)
  token loss: d_log_probs         0 .. 4.0e-8        0 .. 4.0e-8       n1023_v3            (4.02e-8, 4.77e-7, 4.02e-8)
  (vector and scalar backward kernels: the same bits on every case)

One bug came out, in the wrapper, not in a kernel: encoder._ProjLogSoftmaxFunction handed hidden.data_ptr() and
mask.data_ptr() to the kernels without looking at the strides, saved the strided view for the backward, and allocated
dhidden with empty_like(hidden), which keeps a transposed view's strides.  test_autograd_wrapper_on_strided_hidden and
test_autograd_wrapper_takes_a_strided_mask measured it on the MI355X before the fix: a slice wide[..., :K] read the wider
tensor's rows as if they were K long — log_probs off by 150 .. 209 times their largest entry; a transposed view read
(T, B, K) memory as (B, T, K) — off by 0.45 .. 0.55; a mask taken as every other element of a longer vector — off by 10.
No error was raised and nothing was read out of bounds; the shipped models pass contiguous tensors, which is why no
other test saw it.  The wrapper now takes .contiguous() of its four operands before data_ptr(), saves the contiguous
hidden for the backward, and allocates dhidden dense."""
import pytest
import torch

from tests import head_cases as C
from tests.test_gpu_transformer_fp64 import hold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _C():
  from lipreading_amd import _C
  return _C


def all_nan(t):
  return bool(torch.isnan(t).all())


def hold_log_probs(case, got, want64, cpu32, tag=""):
  """Every element, the unmasked and the masked columns each against their own largest entry."""
  assert got.shape == want64.shape
  masked = C.masked_columns(case)
  for what, cols in (("unmasked", ~masked), ("masked", masked)):
    if cols.any():
      hold("%s %slp %s" % (case.name, tag, what), got[:, cols], want64[:, cols], cpu32[:, cols])


# ---- part 1: the forward head ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def forward(dev):
  """lr_proj_logsoftmax_forward on a case: once per case, shared."""
  runs = {}

  def get(name):
    if name not in runs:
      runs[name] = C.run_forward(C.FWD_CASES[name], dev)
    return runs[name]
  return get


@pytest.mark.parametrize("name", list(C.FWD_CASES))
def test_forward_matches_float64(forward, name):
  """The saturated case at the same bound: every exp but one underflows, and the row's logsumexp is its largest logit."""
  case = C.FWD_CASES[name]
  want64, cpu32 = C.fwd_reference(name)
  status, lp, guard = forward(name)
  assert status == 0
  assert all_nan(guard)
  hold_log_probs(case, lp, want64, cpu32)
  masked = C.masked_columns(case)
  # masked classes: finite and ~103.28 below the others, not -inf (the subnormal 1e-45f is kept).  Where EVERY class is
  # masked the -103.28 is common to the row and leaves with the logsumexp: those rows are held by hold() alone.
  assert torch.isfinite(lp).all()
  if case.mask == "two":
    assert float(lp[:, masked].max()) < -90


@pytest.mark.parametrize("fused,fallback", C.TWINS)
def test_fused_and_fallback_agree_on_the_same_data(forward, fused, fallback):
  """One float of misalignment of hidden or of W sends the same numbers down the chain: each result is inside its bound
  (test_forward_matches_float64), so the two are within the sum of the bounds of each other; they need not be bit-equal."""
  assert C.plan(C.FWD_CASES[fused]) == "fused" and C.plan(C.FWD_CASES[fallback]) == "fallback"
  want64, cpu32 = C.fwd_reference(fused)
  assert C.fwd_reference(fallback)[0].equal(want64)
  a, b = forward(fused)[1], forward(fallback)[1]
  masked = C.masked_columns(C.FWD_CASES[fused])
  for what, cols in (("unmasked", ~masked), ("masked", masked)):
    each = C.bound(C.figures(cpu32[:, cols], want64[:, cols]))
    gap = float((a[:, cols].double() - b[:, cols].double()).abs().max()) / float(want64[:, cols].abs().max())
    print("%-28s %-9s fused against fallback %.2e  (each within %.2e of float64)" % (fallback, what, gap, each))
    assert gap <= 2 * each


def test_forward_refuses_more_than_256_classes(dev):
  status, lp, guard = C.run_forward(C.REFUSED, dev)
  assert status == _C().LR_ERR_UNSUPPORTED
  assert all_nan(lp) and all_nan(guard)


@pytest.mark.parametrize("name", ["k64_r17_c65", "k40_r33_c65", "k520_r50_c256"])
def test_forward_refuses_a_short_workspace(dev, name):
  status, lp, guard = C.run_forward(C.FWD_CASES[name], dev, short=1)
  assert status == _C().LR_ERR_WORKSPACE
  assert all_nan(lp) and all_nan(guard)


# ---- part 2: the backward head --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def backward(dev):
  """The plain run of a case (dhidden given, accumulate = 0 into NaN): once per case, shared."""
  runs = {}

  def get(name):
    if name not in runs:
      runs[name] = C.run_backward(C.BWD_CASES[name], dev)
    return runs[name]
  return get


def guards_hold(run):
  for key, guard in run["guards"].items():
    assert all_nan(guard), key


@pytest.mark.parametrize("name", list(C.BWD_CASES))
def test_backward_matches_float64(backward, name):
  want64, cpu32 = C.bwd_reference(name)
  got = backward(name)
  guards_hold(got)
  for key in C.BWD_KEYS:
    assert got[key].shape == want64[key].shape
    hold("%s %s" % (name, key), got[key], want64[key], cpu32[key])


@pytest.mark.parametrize("name", list(C.BWD_CASES))
def test_backward_without_dhidden_gives_the_same_bits(dev, backward, name):
  got = C.run_backward(C.BWD_CASES[name], dev, null_dhidden=True)
  guards_hold(got)
  assert "dhidden" not in got
  for key in ("dlogits", "dW", "dbias"):
    assert not torch.isnan(got[key]).any(), key
    assert torch.equal(got[key], backward(name)[key]), key


@pytest.mark.parametrize("name", list(C.BWD_CASES))
@pytest.mark.parametrize("null_dhidden", [False, True])
def test_backward_accumulates_onto_the_priors(dev, backward, name, null_dhidden):
  """accumulate = 1: prior + gradient, within the bound of that sum; dlogits and dhidden as without."""
  case = C.BWD_CASES[name]
  inp, _ = C.bwd_inputs(case)
  want64, cpu32 = C.bwd_reference(name)
  got = C.run_backward(case, dev, null_dhidden=null_dhidden, accumulate=True)
  guards_hold(got)
  for key in ("dlogits",) + (() if null_dhidden else ("dhidden",)):
    assert torch.equal(got[key], backward(name)[key]), key
  for key, prior in (("dW", inp.prior_dW), ("dbias", inp.prior_db)):
    hold("%s %s+=" % (name, key), got[key], prior.double() + want64[key], prior + cpu32[key])


# ---- part 3: the products the head hands to lr_sgemm ------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in C.gemm_shapes()])
def test_the_heads_products(dev, name):
  """NT with the folded bias (the fallback forward), NN (dhidden) and TN with beta = 1 (dW) at the fallback and chain
  shapes: padded lda / ldb / ldc with NaN in the padding, bases on and one float off a 16-byte boundary, C NaN-filled
  under beta = 0, a 0xFF workspace of the size lr_sgemm_workspace_bytes returns and of twice that (plan_gemm sizes its K
  split by what it is given)."""
  want64, cpu32 = C.gemm_formula(name, torch.float64), C.gemm_formula(name, torch.float32)
  for pad, offset in C.GEMM_LAYOUTS:
    for factor in (1, 2):
      got, padding, behind, wbytes = C.run_gemm(name, dev, pad, offset, factor)
      assert all_nan(padding) and all_nan(behind)
      hold("%s ld+%d off %d ws %dx%d" % (name, pad, offset, factor, wbytes), got, want64, cpu32)


# ---- part 4: the autograd wrapper -----------------------------------------------------------------------------------------

VARIANTS = ("contiguous", "slice", "transposed")


def make_hidden(values, variant, dev):
  """(B, T, K) values on the device as a leaf's view: contiguous; wide[..., :K] of a (B, T, K + 8) tensor; the transpose
  of a (T, B, K) tensor.  Returns (leaf, hidden)."""
  B, T, K = values.shape
  if variant == "contiguous":
    leaf = values.to(dev).requires_grad_(True)
    return leaf, leaf
  if variant == "slice":
    wide = torch.full((B, T, K + 8), 1e3, device=dev)
    wide[..., :K] = values.to(dev)
    leaf = wide.requires_grad_(True)
    hidden = leaf[..., :K]
  else:
    leaf = values.to(dev).transpose(0, 1).contiguous().requires_grad_(True)
    hidden = leaf.transpose(0, 1)
  assert hidden.shape == (B, T, K) and not hidden.is_contiguous()
  return leaf, hidden


def leaf_grad(leaf, variant, K):
  if variant == "slice":
    assert not leaf.grad[..., K:].any()      # nothing reaches the columns outside the slice
    return leaf.grad[..., :K]
  return leaf.grad.transpose(0, 1) if variant == "transposed" else leaf.grad


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["k144_r33_c65", "k40_r33_c65", "k72_r16_c129"])
def test_autograd_wrapper_on_strided_hidden(dev, name, variant):
  """_ProjLogSoftmaxFunction on a (B, T, K) hidden that is contiguous, a slice of a wider tensor, or a transposed view:
  lp and the gradients of hidden, weight and bias against float64 (fused forward and backward; fallback forward with the
  fused backward; fallback forward with the chain)."""
  from lipreading_amd.encoder import _ProjLogSoftmaxFunction
  case = C.FWD_CASES[name]
  inp = C.fwd_inputs(case)
  R, K, Cn = case.R, case.K, case.C
  B = 3 if R % 3 == 0 else 2      # 33 = 3 x 11, 16 = 2 x 8
  assert R % B == 0
  T = R // B
  want64, cpu32 = C.autograd_formula(inp, torch.float64), C.autograd_formula(inp, torch.float32)

  leaf, hidden = make_hidden(inp.hidden.view(B, T, K), variant, dev)
  weight = inp.W.to(dev).requires_grad_(True)
  bias = inp.bias.to(dev).requires_grad_(True)
  lp = _ProjLogSoftmaxFunction.apply(hidden, weight, bias, inp.mask.to(dev))
  assert lp.shape == (B, T, Cn) and lp.is_contiguous()
  lp.backward(inp.g.view(B, T, Cn).to(dev))
  what = "%s %s " % (name, variant)
  hold_log_probs(case, lp.detach().reshape(R, Cn).cpu(), want64["lp"], cpu32["lp"], tag=variant + " ")
  hold(what + "dhidden", leaf_grad(leaf, variant, K).reshape(R, K).cpu(), want64["dhidden"], cpu32["dhidden"])
  hold(what + "dW", weight.grad.cpu(), want64["dW"], cpu32["dW"])
  hold(what + "dbias", bias.grad.cpu(), want64["dbias"], cpu32["dbias"])


def test_autograd_wrapper_takes_a_strided_mask(dev):
  """... and a mask that is every other element of a longer vector."""
  from lipreading_amd.encoder import _ProjLogSoftmaxFunction
  case = C.FWD_CASES["k64_r17_c65"]
  inp = C.fwd_inputs(case)
  want64, cpu32 = C.fwd_reference(case.name)
  wide = torch.full((2 * case.C,), 0.5, device=dev)
  wide[::2] = inp.mask.to(dev)
  with torch.no_grad():
    lp = _ProjLogSoftmaxFunction.apply(inp.hidden.view(1, case.R, case.K).to(dev), inp.W.to(dev), inp.bias.to(dev), wide[::2])
  hold_log_probs(case, lp.reshape(case.R, case.C).cpu(), want64, cpu32, tag="strided mask ")


@pytest.mark.parametrize("name", ["k64_r17_c65", "k72_r16_c129"])
def test_second_backward_doubles_the_flat_gradients(dev, name):
  """The parameters in an optim.FlatParameters buffer: the backward adds straight into .grad (accumulate = 1), so a second
  backward through the retained graph leaves twice the gradient there — fused backward and chain."""
  from lipreading_amd.encoder import _ProjLogSoftmaxFunction
  from lipreading_amd.optim import FlatParameters
  case = C.FWD_CASES[name]
  inp = C.fwd_inputs(case)
  R, K, Cn = case.R, case.K, case.C
  want64, cpu32 = C.autograd_formula(inp, torch.float64), C.autograd_formula(inp, torch.float32)
  proj = torch.nn.Linear(K, Cn).to(dev)
  with torch.no_grad():
    proj.weight.copy_(inp.W)
    proj.bias.copy_(inp.bias)
  flat = FlatParameters(proj)
  assert proj.weight.grad is not None and not flat.grad.any()
  hidden = inp.hidden.view(1, R, K).to(dev).requires_grad_(True)
  lp = _ProjLogSoftmaxFunction.apply(hidden, proj.weight, proj.bias, inp.mask.to(dev))
  g = inp.g.view(1, R, Cn).to(dev)
  for n in (1, 2):
    lp.backward(g, retain_graph=True)
    assert proj.weight.grad.data_ptr() == flat.grad[flat.offsets[0]:].data_ptr()      # still the flat buffer's slice
    for key, p in (("dW", proj.weight), ("dbias", proj.bias)):
      hold("%s %s after %d backward" % (name, key, n), p.grad.cpu(), n * want64[key], n * cpu32[key])
  hold("%s dhidden after 2 backward" % name, hidden.grad.reshape(R, K).cpu(), 2 * want64["dhidden"], 2 * cpu32["dhidden"])


# ---- part 5: the token loss -------------------------------------------------------------------------------------------------

LIVE = [n for n, c in C.NLL_CASES.items() if c.pattern != "all"]
ALL_PAD = [n for n, c in C.NLL_CASES.items() if c.pattern == "all"]


def scalar64(x):
  return torch.as_tensor(float(x), dtype=torch.float64).reshape(1)


@pytest.mark.parametrize("name", LIVE)
def test_token_loss_forward_matches_float64(dev, name):
  want64, cpu32 = C.nll_reference(name)
  out2, guard2 = C.run_nll_forward(name, dev, three=False)
  out3, guard3 = C.run_nll_forward(name, dev, three=True)
  assert all_nan(guard2) and all_nan(guard3)
  assert float(out2[1]) == float(out3[1]) == want64["count"]
  hold(name + " loss", out2[0:1], scalar64(want64["loss"]), cpu32["loss"].reshape(1))
  hold(name + " loss (forward3)", out3[0:1], scalar64(want64["loss"]), cpu32["loss"].reshape(1))
  hold(name + " sum", out3[2:3], scalar64(want64["sum"]), cpu32["sum"].reshape(1))
  assert torch.equal(out3[0], out3[2] / out3[1])      # one float32 division
  assert torch.equal(out2[0], out3[0])


@pytest.mark.parametrize("name", LIVE)
def test_token_loss_backward_matches_float64(dev, name):
  """Every element of d_log_probs; then the same call one float past a 16-byte boundary, which takes the scalar kernel
  whatever V is: the same bits."""
  case = C.NLL_CASES[name]
  want64, cpu32 = C.nll_reference(name)
  assert C.plan(case, offset=0) == case.path and C.plan(case, offset=1) == "scalar"
  d_lp, guard = C.run_nll_backward(name, dev, offset=0)
  assert all_nan(guard)
  hold(name + " d_lp " + case.path, d_lp, want64["d_lp"], cpu32["d_lp"])
  assert torch.equal(d_lp != 0, want64["d_lp"] != 0)      # zero everywhere but at the labels, bit for bit
  off, guard = C.run_nll_backward(name, dev, offset=1)
  assert all_nan(guard)
  assert torch.equal(off, d_lp)


@pytest.mark.parametrize("name", ALL_PAD)
def test_token_loss_of_an_all_pad_batch(dev, name):
  """No label counts: count 0, sum 0, and the loss is the reference's 0 / 0.  The gradient is not pinned."""
  want64, _ = C.nll_reference(name)
  assert want64["count"] == 0 and torch.isnan(want64["loss"])
  out2, guard2 = C.run_nll_forward(name, dev, three=False)
  out3, guard3 = C.run_nll_forward(name, dev, three=True)
  assert all_nan(guard2) and all_nan(guard3)
  assert float(out2[1]) == 0 and float(out3[1]) == 0 and float(out3[2]) == 0
  assert torch.isnan(out2[0]) and torch.isnan(out3[0])
  for offset in (0, 1):      # the backward kernels still stay inside d_log_probs
    _, guard = C.run_nll_backward(name, dev, offset=offset)
    assert all_nan(guard)


@pytest.mark.parametrize("name", ["n1025_v65", "n3000_v68", "n1023_v3"])
def test_decoder_nll_on_a_strided_label_view(dev, name):
  """train.decoder_nll and decoder_nll_sum as the training loop calls them: labels = chars[:, 1:], a view whose rows are
  longer than the loop's L steps."""
  from lipreading_amd.train import decoder_nll, decoder_nll_sum
  case, inp = C.NLL_CASES[name], C.nll_inputs(name)
  want64, cpu32 = C.nll_reference(name)
  chars = inp.wide.to(dev)
  labels = chars[:, 1:]
  assert labels.stride(0) == case.stride > case.L and labels.shape[1] >= case.L
  lp = inp.lp.to(dev).requires_grad_(True)
  loss = decoder_nll(lp, labels, case.pad)
  (loss * C.NLL_G).backward()
  hold(name + " decoder_nll", loss.detach().reshape(1), scalar64(want64["loss"]), cpu32["loss"].reshape(1))
  hold(name + " decoder_nll d_lp", lp.grad.cpu(), want64["d_lp"], cpu32["d_lp"])
  total, count = decoder_nll_sum(lp.detach(), labels, case.pad)
  assert float(count) == want64["count"]
  hold(name + " decoder_nll_sum", total.reshape(1), scalar64(want64["sum"]), cpu32["sum"].reshape(1))
