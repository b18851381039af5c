"""CPU checks of the float64 reference the transformer kernels are held to (tests/test_gpu_transformer_fp64.py):
oracle.torch_oracle's layer formulas equal torch's own nn.TransformerEncoderLayer in float64, and every seeded case of
tests/tfm_layer_cases.py keeps enough rows graded once the rows with a feed-forward pre-activation near zero are
taken out of the gradient comparison."""
import pytest
import torch

from oracle import torch_oracle as O
from tests import tfm_layer_cases as C


@pytest.mark.parametrize("name", ["d256_f512_r33", "d64_f128", "d320_f388"])
def test_layer_formulas_equal_torch_in_float64(name):
  """Outputs, the input gradient and the 14 parameter gradients of input projection + positions + one layer, ragged
  lengths included, to rounding: the device is held to torch's definition, not to this repository's reading of it."""
  x, lens, W, pe, dh = C.case_tensors(name)
  B, T, _, I, Dm, nhead, F, _ = C.CASES[name]
  proj = torch.nn.Linear(I, Dm).double()
  layer = torch.nn.TransformerEncoderLayer(Dm, nhead, F, dropout=0.0, activation='relu', batch_first=True,
                                           norm_first=False).double().train()
  at = layer.self_attn
  params = [proj.weight, proj.bias, at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias,
            layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm1.weight,
            layer.norm1.bias, layer.norm2.weight, layer.norm2.bias]
  with torch.no_grad():
    for p, w in zip(params, W):
      p.copy_(w.double())
  xr = x.double().requires_grad_(True)
  h = layer(proj(xr) + pe.double(), src_key_padding_mask=torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1))
  h.backward(dh.double())
  W64 = [w.double() for w in W]
  c = O.tfm_layer_forward(x.double(), lens, W64, pe.double(), nhead)
  dx, grads = O.tfm_layer_backward(c, W64, dh.double().reshape(B * T, Dm))
  want = [h.detach().reshape(B * T, Dm), xr.grad.reshape(B * T, I)] + [p.grad for p in params]
  for k, a, b in zip(C.OUTPUTS, [c["h2"], dx] + grads, want):
    assert C.rel_err(a, b) < 1e-12, (k, C.rel_err(a, b))


def test_split_bf16_product_is_three_products_of_the_halves():
  """hi = bf16(x), lo = bf16(x - hi): hi + lo carries 16 bits of x, the product misses only lo x lo (2^-16 of a term)."""
  g = torch.Generator().manual_seed(0)
  a, b = torch.randn(37, 300, generator=g), torch.randn(300, 29, generator=g)
  want = a.double() @ b.double()
  err = C.rel_err(O.split_bf16_matmul(a, b), want)
  assert 1e-7 < err < 2e-5, err               # worse than fp32 (it is not a plain product), far better than bf16
  ah = a.bfloat16().float()
  assert float((a - ah - (a - ah).bfloat16().float()).abs().max()) <= 2.0 ** -16 * float(a.abs().max())


@pytest.mark.parametrize("mode", [C.X3, C.F32])
@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_keep_enough_rows_graded(name, mode):
  """The exclusion conditions, from the float64 reference alone, and the figures the device's bounds are derived from."""
  if mode == C.F32 and name in C.ROWBLOCK_CASES:
    return   # (the d_model 256 cases run in X3 mode only: row blocks and the five-launch path)
  r = C.reference(name, mode)
  C.assert_exclusion_is_harmless(r["marginal"])
  recorded = C.Z_ERR[(name, mode, False, None)]
  assert r["m"] == 8 * recorded and recorded / 1.5 <= r["z_err"] <= recorded * 1.5, (r["z_err"], recorded)
  assert float(r["dh"].reshape(r["marginal"].numel(), -1)[r["marginal"]].abs().sum()) == 0


# (name, bf16 input, lengths): the variants tests/test_gpu_transformer_fp64.py runs beside the plain cases
VARIANTS = [("d256_f512_r63", True, None), ("d256_f1024_r2400", True, None), ("d256_f256_r64", False, (16, 1, 0, 16)),
            ("d128_t96", False, (96, 0))]


@pytest.mark.parametrize("name,bf16_input,lens", VARIANTS)
def test_variants_keep_enough_rows_graded(name, bf16_input, lens):
  r = C.reference(name, C.X3, bf16_input, lens)
  C.assert_exclusion_is_harmless(r["marginal"])
  recorded = C.Z_ERR[(name, C.X3, bf16_input, lens)]
  assert r["m"] == 8 * recorded and recorded / 1.5 <= r["z_err"] <= recorded * 1.5, (r["z_err"], recorded)
  for k, v in r["cpu_err"].items():
    assert v <= 1.5 * C.cpu_figure(C.X3, k), (k, v)


def test_rowblock_predicate_stops_where_32_bit_offsets_end():
  """lr_tfm_rowblock_supported (a host function; nothing is allocated): the row-block kernels reach their [R][width]
  tensors, width up to max(F, 768), through 32-bit byte offsets whose top bit means "out of range", so the largest
  tensor has to end below 2^31 bytes.  The last supported and the first unsupported row count per width."""
  from lipreading_amd import _C
  L = _C.lib()
  for F in (256, 512, 1024, 2048):
    last = (2 ** 31 - 1) // (max(F, 768) * 4)
    assert last * max(F, 768) * 4 < 2 ** 31 <= (last + 1) * max(F, 768) * 4
    assert last == {256: 699050, 512: 699050, 1024: 524287, 2048: 262143}[F]
    assert L.lr_tfm_rowblock_supported(1, last, 256, F, 4) == 1
    assert L.lr_tfm_rowblock_supported(1, last + 1, 256, F, 4) == 0
    for B, T in ((last // 75, 75), ((last + 75) // 75, 75), (65536, 65536), (2 ** 31 - 1, 1), (46341, 46341)):
      assert L.lr_tfm_rowblock_supported(B, T, 256, F, 4) == int(B * T <= last), (B, T, F)   # (B * T itself past 2^31 too)
  assert L.lr_tfm_rowblock_supported(32, 75, 256, 1024, 4) == 1 and L.lr_tfm_rowblock_supported(32, 75, 256, 384, 4) == 0
  assert L.lr_tfm_rowblock_supported(32, 75, 256, 1024, 9) == 0 and L.lr_tfm_rowblock_supported(0, 75, 256, 1024, 4) == 0


@pytest.mark.parametrize("mode", [C.X3, C.F32])
def test_recorded_cpu_figures_are_the_measured_ones(mode):
  """CPU_FIGURE (a device bound is 4 x its entry) is the restatement's largest error over the cases, neither more nor
  less.  Within a factor 1.5: the restatement's own products change their summation order with the BLAS build and its
  thread count."""
  worst = [0.0] * 4
  for name in (C.CASES if mode == C.X3 else C.GENERAL_CASES):
    for k, v in C.reference(name, mode)["cpu_err"].items():
      worst[C.kind(k)] = max(worst[C.kind(k)], v)
  for got, recorded in zip(worst, C.CPU_FIGURE[mode]):
    assert recorded / 1.5 <= got <= recorded * 1.5, (worst, C.CPU_FIGURE[mode])
