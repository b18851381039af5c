"""The transformer encoder's kernels against float64, piece by piece (lr_transformer.hip, lr_tfm_rowblock.hip,
lr_attention.hip; the formulas are oracle.torch_oracle's, pinned to torch by tests/test_tfm_layer_reference.py).

Part 1: LayerNorm, the key-masked softmax and the batched product through the C ABI.  Part 2: one whole layer, every
element of the output, the input gradient and the 14 parameter gradients, with the rows whose ReLU could fall either way
taken out of the gradient comparison (tests/tfm_layer_cases.py).  Part 3: the borders of the stack.

No bound here was tuned to a device result.  The exact-fp32 pieces are allowed 4 x the error that the SAME formula makes
in float32 on the CPU against float64 (another summation order), measured in the test, and never less than 4 ulp of fp32
at the tensor's largest entry (4 x 2^-23: a case of a handful of elements can come out exact on the CPU).  One layer is
allowed 4 x tfm_layer_cases.CPU_FIGURE, the CPU restatement's error over all cases."""
import math

import pytest
import torch

from oracle import torch_oracle as O
from tests import tfm_layer_cases as C

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
LR_ERR_UNSUPPORTED = -4


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _lib():
  from lipreading_amd import _C
  return _C.lib()


def _st():
  from lipreading_amd import _C
  return _C.stream_handle()


def _check(status, what):
  from lipreading_amd import _C
  _C.check(status, what)


def hold(what, got, want64, cpu32):
  """got (device) within 4 x the float32 CPU formula's own error of the float64 result, element-wise, relative to the
  float64 tensor's largest entry.  Prints the figures first."""
  scale = max(float(want64.abs().max()), 1e-30)
  cpu = float((cpu32.double() - want64).abs().max()) / scale
  err = float((got.double().cpu() - want64).abs().max()) / scale
  bound = 4 * max(cpu, ULP)
  print("%-40s cpu fp32 %.2e  bound %.2e  device %.2e" % (what, cpu, bound, err))
  assert torch.isfinite(got).all(), what
  assert err <= bound, (what, err, bound, cpu)


# ---- part 1: LayerNorm ------------------------------------------------------------------------------------------------
# measured on the CPU (float32 formula against float64, relative to the largest entry; the bound is 4 x the case's own
# figure, at least 4.8e-7): unit-variance rows: y, mean, rstd 3e-8 .. 8.5e-7, dx 4e-8 .. 3.4e-7, dgamma / dbeta up to
# 2.9e-7; at a common offset of 100: y 1.3e-6 .. 5.8e-6 (the mean's rounding, 100 x 2^-24, against a spread of 1), dx and
# dgamma up to 2.9e-6.  The device came out at 0.1 .. 0.8 of its bound.

def ln_inputs(R, D, kind, g):
  x = torch.randn(R, D, generator=g)
  res = 0.5 * torch.randn(R, D, generator=g)
  if kind == "offset":       # mean ~ 100, spread ~ 1: a one-pass variance E[x^2] - E[x]^2 loses every digit here
    x = x + 100.0
  if kind == "constant":     # row 0 is constant (0.5 + 0.25 sums exactly in any order): variance 0
    x[0], res[0] = 0.5, 0.25
  gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
  beta = 0.2 * torch.randn(D, generator=g)
  dy = torch.randn(R, D, generator=g)
  return x, res, gamma, beta, dy


def run_layernorm(dev, R, D, kind, eps=1e-5):
  L = _lib()
  g = torch.Generator().manual_seed(R * 31 + D)
  x, res, gamma, beta, dy = ln_inputs(R, D, kind, g)
  for residual in (None, res):
    s32 = x if residual is None else x + residual
    s64 = x.double() if residual is None else x.double() + residual.double()
    y64, mean64, rstd64 = O.layernorm_forward(s64, gamma.double(), beta.double(), eps)
    y32, mean32, rstd32 = O.layernorm_forward(s32, gamma, beta, eps)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    rd = None if residual is None else residual.to(dev)
    y = torch.full((R, D), float("nan"), device=dev)
    stats = torch.full((R, 2), float("nan"), device=dev)
    _check(L.lr_layernorm_forward(xd.data_ptr(), None if rd is None else rd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                  y.data_ptr(), stats.data_ptr(), R, D, eps, _st()), "lr_layernorm_forward")
    tag = "ln %dx%d %s%s " % (R, D, kind, "" if residual is None else "+res")
    hold(tag + "y", y, y64, y32)
    hold(tag + "mean", stats[:, 0:1], mean64, mean32)
    hold(tag + "rstd", stats[:, 1:2], rstd64, rstd32)
    if kind == "constant":
      assert float(stats[0, 1]) == pytest.approx(1.0 / math.sqrt(eps), rel=4 * ULP)   # variance 0: rstd = 1 / sqrt(eps)
      assert torch.equal(y[0].cpu(), beta)                                             # 0 x rstd x gamma + beta
    # the backward on its own: the float64 statistics, rounded to fp32, for the device and the CPU formula alike
    st32 = torch.cat([mean64, rstd64], dim=1).float()
    ds64, dg64, db64 = O.layernorm_backward(s64, gamma.double(), mean64, rstd64, dy.double())
    ds32, dg32, db32 = O.layernorm_backward(s32, gamma, st32[:, 0:1], st32[:, 1:2], dy)
    wsb = L.lr_layernorm_workspace_bytes(D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    std, dyd = st32.to(dev), dy.to(dev)
    for accumulate in (0, 1):
      dg0, db0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
      dx = torch.full((R, D), float("nan"), device=dev)
      dgam, dbet = dg0.to(dev), db0.to(dev)
      _check(L.lr_layernorm_backward(xd.data_ptr(), None if rd is None else rd.data_ptr(), gd.data_ptr(),
                                     std.data_ptr(), dyd.data_ptr(), dx.data_ptr(), dgam.data_ptr(),
                                     dbet.data_ptr(), ws.data_ptr(), wsb, accumulate, R, D, _st()), "lr_layernorm_backward")
      hold(tag + "dx", dx, ds64, ds32)
      if accumulate:
        hold(tag + "dgamma+=", dgam, dg0.double() + dg64, dg0 + dg32)
        hold(tag + "dbeta+=", dbet, db0.double() + db64, db0 + db32)
      else:
        hold(tag + "dgamma", dgam, dg64, dg32)
        hold(tag + "dbeta", dbet, db64, db32)


@pytest.mark.parametrize("D", [4, 5, 64, 256, 260, 1920])
@pytest.mark.parametrize("R", [1, 3, 4, 5, 1023, 1025, 2400])
def test_layernorm_matches_float64(dev, R, D):
  """lr_layernorm_forward / _backward, with and without residual, dgamma / dbeta overwritten and added to.  The
  backward walks rows in rounds of 4 x 256 = 1024 (R = 1023, 1025, 2400) and a lane owns columns lane, lane + 64, ..."""
  run_layernorm(dev, R, D, "plain")


@pytest.mark.parametrize("kind", ["offset", "constant"])
@pytest.mark.parametrize("R,D", [(5, 256), (1025, 260), (3, 1920), (4, 5)])
def test_layernorm_offset_and_constant_rows(dev, R, D, kind):
  run_layernorm(dev, R, D, kind)


def test_layernorm_backward_says_where_it_ends(dev):
  """The forward takes any D; the backward keeps 4 x 2 x D floats in LDS: D = 1924 is LR_ERR_UNSUPPORTED, nothing written."""
  L = _lib()
  R, D = 3, 1924
  g = torch.Generator().manual_seed(5)
  x, _, gamma, beta, dy = ln_inputs(R, D, "plain", g)
  y64, mean64, rstd64 = O.layernorm_forward(x.double(), gamma.double(), beta.double(), 1e-5)
  y32 = O.layernorm_forward(x, gamma, beta, 1e-5)[0]
  xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
  y, stats = torch.empty(R, D, device=dev), torch.empty(R, 2, device=dev)
  _check(L.lr_layernorm_forward(xd.data_ptr(), None, gd.data_ptr(), bd.data_ptr(), y.data_ptr(), stats.data_ptr(), R, D,
                                1e-5, _st()), "lr_layernorm_forward")
  hold("ln 3x1924 y", y, y64, y32)
  wsb = L.lr_layernorm_workspace_bytes(D)
  ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
  dx, dgam, dbet = torch.full((R, D), 7.0, device=dev), torch.full((D,), 7.0, device=dev), torch.full((D,), 7.0, device=dev)
  dyd = dy.to(dev)
  status = L.lr_layernorm_backward(xd.data_ptr(), None, gd.data_ptr(), stats.data_ptr(), dyd.data_ptr(), dx.data_ptr(),
                                   dgam.data_ptr(), dbet.data_ptr(), ws.data_ptr(), wsb, 0, R, D, _st())
  assert status == LR_ERR_UNSUPPORTED
  torch.cuda.synchronize()
  assert bool((dx == 7.0).all()) and bool((dgam == 7.0).all()) and bool((dbet == 7.0).all())


# ---- part 1: the key-masked softmax -----------------------------------------------------------------------------------
# measured on the CPU: probabilities within 5e-8 with and without a common offset of 1000, the backward within 9.4e-8, row
# sums within 1.6e-7 of 1: every bound here is the floor, 4 ulp = 4.8e-7.  The device: at most 0.25 of it.

def softmax_lens(T, with_zero=False):
  return torch.tensor([1, T, max(1, T // 2), 0 if with_zero else max(1, T - 1)], dtype=torch.int32)


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 75, 96, 97, 130])
def test_attn_softmax_matches_float64(dev, T, offset):
  """lr_attn_softmax_forward / _backward: masked probabilities exactly 0, rows sum to 1, a large common offset of the
  scores changes nothing (stability); backward = scale P (dP - sum dP P), exactly 0 at masked keys."""
  L = _lib()
  B, H, scale = 4, 3, 0.125
  g = torch.Generator().manual_seed(T)
  lens = softmax_lens(T)
  scores = 3.0 * torch.randn(B, H, T, T, generator=g) + offset
  p64 = O.attn_softmax_forward(scores.double(), lens, scale)
  p32 = O.attn_softmax_forward(scores, lens, scale)
  p, lens_d = scores.to(dev), lens.to(dev)
  _check(L.lr_attn_softmax_forward(p.data_ptr(), lens_d.data_ptr(), scale, B, H, T, _st()), "lr_attn_softmax_forward")
  hold("softmax T %d offset %g P" % (T, offset), p, p64, p32)
  masked = (torch.arange(T).view(1, 1, 1, T) >= lens.view(B, 1, 1, 1)).expand(B, H, T, T)
  assert bool((p.cpu()[masked] == 0).all())
  hold("softmax T %d offset %g row sums" % (T, offset), p.double().sum(-1), torch.ones(B, H, T, dtype=torch.float64), p32.double().sum(-1))
  # the backward on its own: the float64 probabilities rounded to fp32 (zeros stay zeros)
  pf = p64.float()
  dP = torch.randn(B, H, T, T, generator=g)
  d64 = O.attn_softmax_backward(pf.double(), dP.double(), scale)
  d32 = O.attn_softmax_backward(pf, dP, scale)
  d, pfd = dP.to(dev), pf.to(dev)
  _check(L.lr_attn_softmax_backward(pfd.data_ptr(), d.data_ptr(), scale, B, H, T, _st()), "lr_attn_softmax_backward")
  hold("softmax T %d offset %g dS" % (T, offset), d, d64, d32)
  assert bool((d.cpu()[masked] == 0).all())


def attention_inputs(B, T, nhead, dh, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randn(B, T, 3 * nhead * dh, generator=g), torch.randn(B, T, nhead * dh, generator=g)


@pytest.mark.parametrize("T,dh", [(1, 64), (2, 32), (33, 32), (75, 64), (96, 64), (97, 64), (20, 16)])
def test_a_sample_of_length_zero_attends_to_key_zero(dev, T, dh):
  """The header's rule for both attention paths: key_lens is clamped to [1, T].  A batch that holds a zero-length sample,
  forward and backward: the fp32 path (lr_sgemm_batched + lr_attn_softmax_*, transformer._AttentionFunction) at the
  exact-fp32 bound, the fused kernels (where they take the shape) at their stated 2e-2 of the largest entry / 1e-2 of the
  norm.  torch gives NaN for such a sample, so the reference is oracle.attn_softmax_forward's clamp."""
  from lipreading_amd.transformer import _AttentionFunction
  B, nhead = 4, 2
  lens = softmax_lens(T, with_zero=True)
  qkv, dout = attention_inputs(B, T, nhead, dh, seed=T * 7 + dh)
  a64, p64 = O.attention_forward(qkv.double(), lens, nhead)
  d64 = O.attention_backward(qkv.double(), p64, dout.double(), nhead)
  a32, p32 = O.attention_forward(qkv, lens, nhead)
  d32 = O.attention_backward(qkv, p32, dout, nhead)
  assert bool((p64[3, :, :, 0] == 1).all())      # the zero-length sample: all of the weight on key 0
  fused_ok = bool(_lib().lr_attn_fused_supported(T, dh))
  assert fused_ok == (T <= 96 and dh in (32, 64))
  for fused in ([False, True] if fused_ok else [False]):
    x = qkv.to(dev).requires_grad_(True)
    out = _AttentionFunction.apply(x, lens.to(dev), nhead, fused)
    out.backward(dout.to(dev))
    if not fused:
      hold("len 0, T %d dh %d: context" % (T, dh), out.detach(), a64, a32)
      hold("len 0, T %d dh %d: dqkv" % (T, dh), x.grad, d64, d32)
    else:
      for what, a, b in (("context", out.detach().cpu().double(), a64), ("dqkv", x.grad.cpu().double(), d64)):
        print("len 0 fused, T %d dh %d: %s max %.2e norm %.2e" % (T, dh, what, float((a - b).abs().max() / b.abs().max()),
                                                                  float((a - b).norm() / b.norm())))
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max())
        assert float((a - b).norm()) <= 1e-2 * float(b.norm())
        # and the sample itself, not only the batch's norm
        assert float((a[3] - b[3]).norm()) <= 1e-2 * float(b[3].norm()) + 1e-30


# ---- part 1: lr_sgemm_batched in the five shapes of the attention ------------------------------------------------------
# measured on the CPU: 2e-8 .. 5.2e-7 (K = dh or T <= 130 terms per element); the device: 0.25 .. 0.27 of its bound

@pytest.mark.parametrize("dh", [16, 32, 64])
@pytest.mark.parametrize("T", [1, 33, 75, 130])
def test_sgemm_batched_in_the_attention_shapes(dev, T, dh):
  """QK^T, PV, dP = dO V^T, dV = P^T dO, dQ = dS K / dK = dS^T Q with the operands read in place from a [B][T][3D] tensor,
  the strides transformer._AttentionFunction passes; what a product does not own (the other two thirds of dqkv) stays
  untouched; and beta != 0."""
  L = _lib()
  B, nh = 2, 3
  D, D3 = nh * dh, 3 * nh * dh
  g = torch.Generator().manual_seed(T * 100 + dh)
  qkv = torch.randn(B, T, D3, generator=g)
  dout = torch.randn(B, T, D, generator=g)
  P = torch.randn(B, nh, T, T, generator=g)
  heads = lambda t: t.reshape(B, T, nh, dh).transpose(1, 2)        # [B,T,D] -> [B,nh,T,dh]
  q, k, v = [heads(t) for t in qkv.split(D, dim=-1)]
  do = heads(dout)
  flat = lambda t: t.transpose(1, 2).reshape(B, T, D)              # back
  qd, dd, Pd = qkv.to(dev), dout.to(dev), P.to(dev)
  qp, kp, vp = qd.data_ptr(), qd.data_ptr() + 4 * D, qd.data_ptr() + 8 * D
  PS, PI = nh * T * T, T * T

  def product(what, tA, tB, M, N, K, a, lda, sa, b, ldb, sb, c, c_off, ldc, sc, sci, alpha=1.0, beta=0.0):
    _check(L.lr_sgemm_batched(tA, tB, M, N, K, alpha, a, lda, sa[0], sa[1], b, ldb, sb[0], sb[1], beta, c.data_ptr() + 4 * c_off,
                              ldc, sc, sci, B, nh, _st()), what)

  f64 = lambda t: t.double()
  # QK^T and PV
  S = torch.full((B, nh, T, T), float("nan"), device=dev)
  product("QK^T", 0, 1, T, T, dh, qp, D3, (T * D3, dh), kp, D3, (T * D3, dh), S, 0, T, PS, PI)
  hold("sgemm T %d dh %d QK^T" % (T, dh), S, f64(q) @ f64(k).transpose(-1, -2), q @ k.transpose(-1, -2))
  out = torch.full((B, T, D), float("nan"), device=dev)
  product("PV", 0, 0, T, dh, T, Pd.data_ptr(), T, (PS, PI), vp, D3, (T * D3, dh), out, 0, D, T * D, dh)
  hold("sgemm T %d dh %d PV" % (T, dh), out, flat(f64(P) @ f64(v)), flat(P @ v))
  # dP = dO V^T
  dP = torch.full((B, nh, T, T), float("nan"), device=dev)
  product("dP", 0, 1, T, T, dh, dd.data_ptr(), D, (T * D, dh), vp, D3, (T * D3, dh), dP, 0, T, PS, PI)
  hold("sgemm T %d dh %d dP" % (T, dh), dP, f64(do) @ f64(v).transpose(-1, -2), do @ v.transpose(-1, -2))
  # dV = P^T dO, dQ = dS K, dK = dS^T Q into the thirds of one dqkv tensor (P stands for dS)
  dqkv = torch.full((B, T, D3), 7.0, device=dev)
  product("dV", 1, 0, T, dh, T, Pd.data_ptr(), T, (PS, PI), dd.data_ptr(), D, (T * D, dh), dqkv, 2 * D, D3, T * D3, dh)
  torch.cuda.synchronize()
  assert bool((dqkv[..., :2 * D] == 7.0).all())
  product("dQ", 0, 0, T, dh, T, Pd.data_ptr(), T, (PS, PI), kp, D3, (T * D3, dh), dqkv, 0, D3, T * D3, dh)
  torch.cuda.synchronize()
  assert bool((dqkv[..., D:2 * D] == 7.0).all())
  product("dK", 1, 0, T, dh, T, Pd.data_ptr(), T, (PS, PI), qp, D3, (T * D3, dh), dqkv, D, D3, T * D3, dh)
  Pt = P.transpose(-1, -2)
  hold("sgemm T %d dh %d dQ" % (T, dh), dqkv[..., :D], flat(f64(P) @ f64(k)), flat(P @ k))
  hold("sgemm T %d dh %d dK" % (T, dh), dqkv[..., D:2 * D], flat(f64(Pt) @ f64(q)), flat(Pt @ q))
  hold("sgemm T %d dh %d dV" % (T, dh), dqkv[..., 2 * D:], flat(f64(Pt) @ f64(do)), flat(Pt @ do))
  # alpha, beta != 0 on the strided output
  C0 = torch.randn(B, T, D3, generator=g)
  Cd = C0.to(dev)
  product("dQ, beta", 0, 0, T, dh, T, Pd.data_ptr(), T, (PS, PI), kp, D3, (T * D3, dh), Cd, 0, D3, T * D3, dh, alpha=2.0, beta=-0.5)
  hold("sgemm T %d dh %d 2 dS K - C / 2" % (T, dh), Cd[..., :D], 2.0 * flat(f64(P) @ f64(k)) - 0.5 * f64(C0[..., :D]),
       2.0 * flat(P @ k) - 0.5 * C0[..., :D])
  assert torch.equal(Cd[..., D:].cpu(), C0[..., D:])


# ---- part 2: one layer, every element ---------------------------------------------------------------------------------

def make_encoder(dev, name, mode, W, attention='f32', bf16_input=False):
  from lipreading_amd.transformer import TransformerVideoEncoder
  _, _, _, I, Dm, nhead, F, _ = C.CASES[name]
  enc = TransformerVideoEncoder(I, Dm, nhead, 1, F, enable_ctc=False)
  ly, at = enc.layers[0], enc.layers[0].self_attn
  params = [enc.input_proj.weight, enc.input_proj.bias, at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias,
            ly.linear1.weight, ly.linear1.bias, ly.linear2.weight, ly.linear2.bias, ly.norm1.weight, ly.norm1.bias,
            ly.norm2.weight, ly.norm2.bias]
  with torch.no_grad():
    for p, w in zip(params, W):
      p.copy_(w)
  enc.input_projection = 'bf16x3' if mode == C.X3 else 'f32'
  enc.attention = attention
  enc.input_is_bf16 = bf16_input
  return enc.to(dev).train(), params


def run_layer(dev, name, mode, rowblock, attention='f32', bf16_input=False, lens=None):
  """-> the reference record and the device's h, dx and 14 gradients by name (CPU tensors)"""
  import lipreading_amd.transformer as tfm
  r = C.reference(name, mode, bf16_input, lens)
  B, T, _, I, Dm, nhead, F, _ = C.CASES[name]
  C.assert_exclusion_is_harmless(r["marginal"])
  enc, params = make_encoder(dev, name, mode, r["W"], attention, bf16_input)
  want_rb = mode == C.X3 and rowblock and Dm == 256
  assert bool(_lib().lr_tfm_rowblock_supported(B, T, Dm, F, 1)) == (Dm == 256)
  x = r["x"].to(dev)
  x = (x.bfloat16() if bf16_input else x).requires_grad_(True)
  tfm.rowblock_layers = rowblock
  try:
    h, _ = enc(x, r["lens"], max_len=T)
    h.backward(r["dh"].to(dev))
  finally:
    tfm.rowblock_layers = True
  got = dict(zip(C.OUTPUTS, [h.detach().reshape(B * T, Dm).cpu(), x.grad.reshape(B * T, I).cpu()] + [p.grad.cpu() for p in params]))
  print("%s %s %s: %d rows, %.1f %% marginal at m = %.2e" % (name, mode, "row blocks" if want_rb else "five launches", B * T,
                                                             100 * float(r["marginal"].float().mean()), r["m"]))
  return r, got


def hold_layer(tag, r, got, mode, skip=()):
  """every element of h (ALL rows: the forward is continuous in z), dx and the 14 gradients within 4 x the CPU
  restatement's figure (tfm_layer_cases.CPU_FIGURE; X3: h 5.3e-6, dx 9.9e-6, weights 1.8e-5, vectors 8.8e-6 -> bounds
  2.1e-5, 4.0e-5, 7.2e-5, 3.5e-5; exact fp32: 3.6e-7, 5.3e-7, 5.4e-7, 4.4e-7 -> 1.4e-6, 2.1e-6, 2.2e-6, 1.8e-6)"""
  bad = []
  for k in C.OUTPUTS:
    if k in skip:
      continue
    err, bound = C.rel_err(got[k], r["want"][k]), 4 * C.cpu_figure(mode, k)
    print("  %-20s cpu (this case) %.2e  figure %.2e  bound %.2e  device %.2e%s" % (k, r["cpu_err"][k], C.cpu_figure(mode, k), bound, err,
                                                                                 "  <-- MISSES" if not err <= bound else ""))
    if not (err <= bound and bool(torch.isfinite(got[k]).all())):
      bad.append((k, err, bound))
  assert not bad, (tag, bad)


@pytest.mark.parametrize("rowblock", [True, False], ids=["rowblock", "five_launches"])
@pytest.mark.parametrize("name", C.ROWBLOCK_CASES)
def test_one_layer_every_element_d256(dev, name, rowblock):
  """d_model 256, X3 products: the row-block launch (lr_tfm_rowblock.hip) and the five-launch path, F = 256 .. 2048, row
  counts 32 k, 32 k + 1, 32 k + 31 and the bench's 32 x 75, ragged lengths including 1."""
  r, got = run_layer(dev, name, C.X3, rowblock)
  hold_layer(name, r, got, C.X3)


@pytest.mark.parametrize("mode", [C.X3, C.F32])
@pytest.mark.parametrize("name", C.GENERAL_CASES)
def test_one_layer_every_element_general_stack(dev, name, mode):
  """The general stack (lr_fgemm products + LayerNorm + fp32 attention) in X3 and in exact-fp32 mode at d_model 64 .. 1920."""
  r, got = run_layer(dev, name, mode, True)
  hold_layer(name, r, got, mode)


# ---- part 3: borders of the stack -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,fused", [("d128_t96", True), ("d128_t97", False), ("d64_f128", False)])
def test_fused_attention_border(dev, name, fused):
  """attention = 'bf16' takes the fused kernels up to T = 96 at head sizes 32 / 64 and the fp32 attention past that,
  silently.  Same model either side of the border; each run agrees with float64 at the bound of the path it took: the
  one-layer bound where the fp32 attention ran, the fused kernels' stated 2e-2 of the largest entry / 1e-2 of the norm
  (outputs only: ReLU switches cannot be excluded at that precision) where they ran."""
  B, T, _, I, Dm, nhead, F, _ = C.CASES[name]
  assert bool(_lib().lr_attn_fused_supported(T, Dm // nhead)) == fused
  r, got = run_layer(dev, name, C.X3, True, attention='bf16')
  if not fused:
    hold_layer(name, r, got, C.X3)
    return
  a, b = got["h"].double(), r["want"]["h"]
  print("fused: h max %.2e norm %.2e" % (float((a - b).abs().max() / b.abs().max()), float((a - b).norm() / b.norm())))
  assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max())
  assert float((a - b).norm()) <= 1e-2 * float(b.norm())
  assert float((a - b).abs().max()) > 4 * C.cpu_figure(C.X3, "h") * float(b.abs().max())   # (it WAS the bf16 path)
  assert all(bool(torch.isfinite(v).all()) for v in got.values())


@pytest.mark.parametrize("name,rowblock", [("d256_f512_r63", True), ("d256_f1024_r2400", True), ("d256_f512_r63", False)])
def test_bf16_input_and_bf16_dx(dev, name, rowblock):
  """LR_TFM_X_BF16 | LR_TFM_DX_BF16, what the pixel regime uses: features rounded to bf16 on the host, reference =
  float64 on the rounded values.  h and the 14 gradients at the one-layer bound; dx is STORED as bf16: each element
  within one bf16 rounding (2^-8 of itself) plus the fp32 bound of the float64 dx."""
  r, got = run_layer(dev, name, C.X3, rowblock, bf16_input=True)
  assert got["dx"].dtype == torch.bfloat16
  hold_layer(name, r, got, C.X3, skip=("dx",))
  want = r["want"]["dx"]
  slack = 2.0 ** -8 * want.abs() + 4 * C.cpu_figure(C.X3, "dx") * float(want.abs().max())
  over = (got["dx"].double() - want).abs() - slack
  print("  dx (bf16): worst element over its allowance by %.2e (max |dx| %.2e)" % (float(over.max()), float(want.abs().max())))
  assert float(over.max()) <= 0


@pytest.mark.parametrize("name,zero_at", [("d256_f256_r64", 2), ("d128_t96", 1)])
@pytest.mark.parametrize("attention", ["f32", "bf16"])
def test_zero_length_sample_through_a_stack(dev, name, zero_at, attention):
  """A batch with a sample of length 0 through one layer: the fp32 attention at the one-layer bound against the float64
  formula with the length clamped to 1 (the header's rule); the fused attention, which used to give that sample a context
  of 0, at its stated bound on the outputs."""
  lens = [int(v) for v in C.case_lens(name)]
  lens[zero_at] = 0
  r, got = run_layer(dev, name, C.X3, True, attention=attention, lens=tuple(lens))
  assert all(bool(torch.isfinite(v).all()) for v in got.values())
  if attention == "f32":
    hold_layer(name, r, got, C.X3)
    return
  B, T = C.CASES[name][:2]
  a, b = got["h"].double().reshape(B, T, -1), r["want"]["h"].reshape(B, T, -1)
  for what, u, v in (("batch", a, b), ("the zero-length sample", a[zero_at], b[zero_at])):
    print("fused, %s: h max %.2e norm %.2e" % (what, float((u - v).abs().max() / v.abs().max()), float((u - v).norm() / v.norm())))
    assert float((u - v).abs().max()) <= 2e-2 * float(v.abs().max())
    assert float((u - v).norm()) <= 1e-2 * float(v.norm())


def stack_pair(dev, layers, ff, seed=11, attention='bf16'):
  from tests.test_gpu_transformer import make_pair
  ref, enc = make_pair(dev, frame_dim=96, d_model=256, nhead=4, layers=layers, ff=ff, seed=seed, attention=attention)
  enc.input_projection = 'bf16x3'
  return ref, enc


def run_stack_both_ways(dev, ref, enc, B, T, lens):
  """test_rowblock_layers_equal_the_five_launch_path's run: -> names, oracle, {rowblock_layers: results}"""
  import lipreading_amd.transformer as tfm
  g = torch.Generator().manual_seed(12)
  x0 = torch.randn(B, T, 96, generator=g)
  lens_t = torch.tensor(lens)
  wgt = torch.randn(B, T, 65, generator=g)
  valid = (torch.arange(T).unsqueeze(0) < lens_t.unsqueeze(1)).float().unsqueeze(-1)
  xr = x0.clone().requires_grad_(True)
  lp_r, h_r = ref(xr.unsqueeze(-1), lens_t)
  ((lp_r * wgt * valid).sum() + (h_r * valid).pow(2).sum()).backward()
  want = dict(ref.named_parameters())
  names = ["log_probs", "hidden", "dx"] + [k for k, _ in enc.named_parameters()]
  oracle = [lp_r.detach() * valid, h_r.detach() * valid, xr.grad] + [(want[k] if k in want else want["encoder." + k]).grad for k in names[3:]]
  res, vd = {}, valid.to(dev)
  for rb in (False, True):
    tfm.rowblock_layers = rb
    try:
      enc.zero_grad()
      x = x0.to(dev).requires_grad_(True)
      lp, h, _ = enc(x, lens_t, max_len=T)
      ((lp * wgt.to(dev) * vd).sum() + (h * vd).pow(2).sum()).backward()
      res[rb] = [(lp.detach() * vd).cpu(), (h.detach() * vd).cpu(), x.grad.cpu()] + [p.grad.cpu().clone() for p in enc.parameters()]
    finally:
      tfm.rowblock_layers = True
  return names, oracle, res


@pytest.mark.parametrize("B,T,ff,layers,lens", [(4, 20, 2048, 2, [20, 13, 20, 5]),     # F = 2048: its own instantiation (8 chunks)
                                               (32, 75, 512, 8, None),                # the most layers the weight pack takes
                                               (16, 75, 2048, 8, None)])
def test_rowblock_widths_and_depths_never_run(dev, B, T, ff, layers, lens):
  """Row blocks at F = 2048 and at 8 layers against the five-launch path and torch.nn.TransformerEncoder on the CPU, in
  the form and at the bounds of test_rowblock_layers_equal_the_five_launch_path (norm-wise: several layers, ReLU switches
  cannot be excluded).  The 8-layer cases have the bench's row count: the norm-wise form assumes that ONE switch is far
  below the bound, and with a few dozen rows a single switched unit is 1e-2 of linear1.weight's gradient by itself
  (1 / sqrt(rows x active units); seen at 3 x 11 rows and 8 layers: 1.8e-2 at layers.5.linear1.weight)."""
  assert _lib().lr_tfm_rowblock_supported(B, T, 256, ff, layers) == 1
  if lens is None:
    lens = [int(v) for v in torch.randint(20, T + 1, (B,), generator=torch.Generator().manual_seed(9))]
    lens[0] = T
  ref, enc = stack_pair(dev, layers, ff)
  names, oracle, res = run_stack_both_ways(dev, ref, enc, B, T, lens)
  for k, a, b, r in zip(names, res[False], res[True], oracle):
    assert torch.isfinite(b).all(), k
    scale = max(1e-6, float(r.norm()))
    err_five, err_rb, gap = float((a - r).norm()) / scale, float((b - r).norm()) / scale, float((a - b).norm()) / scale
    print("%-45s five %.2e  row blocks %.2e  gap %.2e" % (k, err_five, err_rb, gap))
    assert gap < (2e-4 if k in ("log_probs", "hidden") else 1e-2), (k, gap)
    assert err_rb <= 1.5 * err_five + (1e-4 if k in ("log_probs", "hidden") else 5e-3), (k, err_rb, err_five)


@pytest.mark.parametrize("ff,layers", [(384, 2), (512, 9)])
def test_unsupported_rowblock_shapes_fall_back(dev, ff, layers):
  """F = 384 and 9 layers are not row-block shapes: the stack runs without the mode bit (so the test hook changes nothing:
  bit-identical results) and agrees with the CPU oracle at test_transformer_bf16x3_linears_track_fp32's 3e-2 of the norm."""
  B, T, lens = 3, 11, [11, 11, 4]
  assert _lib().lr_tfm_rowblock_supported(B, T, 256, ff, layers) == 0
  ref, enc = stack_pair(dev, layers, ff, attention='f32')
  names, oracle, res = run_stack_both_ways(dev, ref, enc, B, T, lens)
  for k, a, b, r in zip(names, res[False], res[True], oracle):
    assert torch.equal(a, b), k
    err = float((b - r).norm()) / max(1e-6, float(r.norm()))
    print("%-45s %.2e" % (k, err))
    assert err < 3e-2, (k, err)


@pytest.mark.parametrize("name,mode", [("d256_f1024_r63", C.X3), ("d320_f388", C.F32), ("d320_f388", C.X3)])
def test_two_backward_passes_accumulate(dev, name, mode):
  """lr_tfm_backward_weights(accumulate != 0), the direct-gradient path: a second backward into existing .grad buffers
  adds to them.  Same products, one more fp32 addition per element: |g12 - (g1 + g2)| <= 4 x 2^-23 x (|g1| + |g2|)
  element-wise, plus the same fraction of the tensor's largest entry for elements that nearly cancel."""
  r = C.reference(name, mode)
  B, T, _, I, Dm, nhead, F, _ = C.CASES[name]
  enc, params = make_encoder(dev, name, mode, r["W"])
  g = torch.Generator().manual_seed(77)
  dh = [torch.randn(B, T, Dm, generator=g).to(dev) for _ in range(2)]
  h, _ = enc(r["x"].to(dev), r["lens"], max_len=T)
  singles = []
  for d in dh:
    enc.zero_grad(set_to_none=True)
    h.backward(d, retain_graph=True)
    singles.append([p.grad.clone() for p in params])
  enc.zero_grad(set_to_none=True)
  h.backward(dh[0], retain_graph=True)      # .grad appears
  h.backward(dh[1])                          # accumulate = 1 straight into it
  for k, p, g1, g2 in zip(O.TFM_LAYER_NAMES, params, *singles):
    allowed = 4 * ULP * (g1.abs() + g2.abs() + (g1 + g2).abs().max())
    over = ((p.grad - (g1 + g2)).abs() - allowed).max()
    print("  %-20s worst |g12 - (g1 + g2)| / max %.2e" % (k, float((p.grad - (g1 + g2)).abs().max() / (g1 + g2).abs().max())))
    assert float(over) <= 0, k
    assert float((p.grad - g1).abs().max()) > 0.1 * float(g2.abs().max())   # (the second pass did arrive)


@pytest.mark.parametrize("attention,rowblock", [("f32", True), ("bf16", True), ("f32", False)])
def test_padding_cannot_reach_valid_frames(dev, attention, rowblock):
  """Two runs whose inputs differ only at frames >= lens[b] (second run: +-1e4 there), upstream gradient zero at padded
  frames.  A masked key has probability exactly 0 and a padded row's gradient is exactly 0, so every product that could
  carry padding into a valid frame or a parameter is 0 x finite: h and dx at valid frames and all 14 parameter
  gradients are bit-identical."""
  import lipreading_amd.transformer as tfm
  name = "d256_f512_r63"
  r = C.reference(name, C.X3)
  B, T, _, I, Dm, nhead, F, _ = C.CASES[name]
  lens = r["lens"]
  valid = torch.arange(T).unsqueeze(0) < lens.unsqueeze(1)
  assert int((~valid).sum()) > 0
  g = torch.Generator().manual_seed(3)
  x2 = r["x"].clone()
  x2[~valid] = 1e4 * torch.sign(torch.randn(int((~valid).sum()), I, generator=g))
  dh = torch.randn(B, T, Dm, generator=g) * valid.unsqueeze(-1)
  enc, params = make_encoder(dev, name, C.X3, r["W"], attention)
  res = []
  tfm.rowblock_layers = rowblock
  try:
    for xin in (r["x"], x2):
      enc.zero_grad(set_to_none=True)
      x = xin.to(dev).requires_grad_(True)
      h, _ = enc(x, lens, max_len=T)
      h.backward(dh.to(dev))
      assert torch.isfinite(h).all() and torch.isfinite(x.grad).all()
      res.append([h.detach().cpu()[valid], x.grad.cpu()[valid]] + [p.grad.cpu().clone() for p in params])
  finally:
    tfm.rowblock_layers = True
  for k, a, b in zip(C.OUTPUTS, *res):
    print("  %-20s max difference %.3e" % (k, float((a - b).abs().max())))
    assert torch.equal(a, b), k
