"""The layer-2 patch-resident kernel (lr_conv_patch.hip) on v_mfma_f32_16x16x32_bf16: its lane maps at tile shapes the
case table of tests/frontend_exact_cases.py lacks, and its rounding.

A wave of the kernel owns a frame of a tile of 4 frames x 8 rows x 24 columns as twelve 4 x 4 pixel blocks x 16-column
accumulator tiles; the A fragment of a block is read from LDS by position lane & 15 and k chunk lane >> 4, the B
fragment from the 32-column weight packing at a per-lane offset, and the epilogues take a lane's four C/D registers as
one 2 x 2 pooling window.  A wrong lane map moves whole products between pixels, channels or taps, so the exact cases
(small integers: every sum exact in any order, the bar is equality with fp64) catch it; the shapes put a clip boundary
on a tile edge and inside a tile, a ragged last tile, and halo rows between two row tiles.  The rounding-level cases use
random non-integer data against F.conv3d in fp64 on the same bf16-rounded operands.

The raw _C.lib() entry points are called, as in tests/test_gpu_frontend_exact.py; test_exactness_conditions runs without
a GPU and checks that equality is the right bar for the exact cases (it mirrors tests/test_frontend_exact_cpu.py)."""
import functools

import pytest
import torch

from tests import frontend_exact_cases as FC

BF, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
NAN = float("nan")
L2 = FC.L2
OPS = ("fwd", "fwd_pooled", "dgrad", "dgrad_pooled")
# (B, T, H): a clip boundary exactly on a tile edge, one row tile; a full tile plus a one-frame ragged tile, with halo
# rows between two row tiles; a clip boundary inside the third tile
SHAPES = ((2, 4, 8), (1, 5, 16), (2, 9, 8))
CASES = [FC.Case("patch2mfma-l2-B%dT%d-%dx24" % (B, T, H), "patch2", L2, B, T, H, 24, OPS, 0.5) for B, T, H in SHAPES]
IDS = [c.name for c in CASES]
ROUND_SHAPE = (2, 5, 16)


@functools.lru_cache(maxsize=None)
def _problem(name):
  return FC.Problem(next(c for c in CASES if c.name == name))


# ---------------------------------------------------------------------------------------------------------------
# host only
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_exactness_conditions(name):
  """Every expected bf16 output is an integer of magnitude <= 256 and every partial sum stays below 2^24: the sum of
  the magnitudes of an output's products bounds each of its partial sums in any order."""
  p = _problem(name)
  assert set(p.x.unique().tolist()) == {-1.0, 0.0, 1.0} and set(p.w.unique().tolist()) <= {-1.0, 0.0, 1.0}
  assert set(p.dP.unique().tolist()) == {-1.0, 0.0, 1.0} and float(p.bias.abs().max()) <= 3
  assert set(p.code.unique().tolist()) == {0, 1, 2, 3, 4}
  for op in OPS:
    for key, (want, kind) in p.expected(op).items():
      want = want.double()
      assert bool((want == want.round()).all()), (op, key)
      top = float(want.abs().max())
      assert top > 0, (op, key)
      assert top <= (FC.BF16_EXACT if kind == "bf16" else 4), (op, key, top)
  mag_fwd = FC.conv_forward(p.x.abs(), p.w.abs()) + p.bias.abs()
  mag_dx = FC.conv_dgrad(p.dz_unpooled.abs(), p.w.abs(), p.x.shape)
  assert float(mag_fwd.max()) < FC.F32_EXACT and float(mag_dx.max()) < FC.F32_EXACT
  # the pooled forward ties: the first-maximum rule decides window codes
  positive, tied, first = FC.pool_ties(p.z + p.bias)
  assert int((positive & tied).sum()) >= 100


# ---------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _abi():
  from lipreading_amd import _C
  return _C, _C.lib(), _C.stream_handle()


def _bf16(t, dev):
  return t.to(BF).to(dev).contiguous()


def _nans(shape, dev, dtype=BF):
  return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def _host(t, shape):
  torch.cuda.synchronize()
  return t.cpu().double().reshape(tuple(shape))


GEOM = tuple(L2.k) + (L2.stride,) + tuple(L2.pad)


def _pack(w, dgrad, dev):
  """The fragment-major operand (public flag 2) of the forward or, flipped and channel-transposed, the data gradient."""
  _C, L, st = _abi()
  kt, kh, kw = L2.k
  assert L.lr_conv3d_patch_supported(8, 24, L2.cin_pad, L2.cout, *GEOM) == 2
  assert L.lr_conv3d_patch_supported(8, 24, L2.cout, L2.cin, *GEOM) == 2
  shape = (L2.cin, kt * kh * kw, L2.cout) if dgrad else (L2.cout, kt * kh * kw, L2.cin_pad)
  w32 = w.to(F32).to(dev).contiguous()
  out = _nans(shape, dev)
  _C.check(L.lr_conv3d_pack_weights(w32.data_ptr(), out.data_ptr(), L2.cout, L2.cin, L2.cin_pad, kt, kh, kw,
                                    2 | (1 if dgrad else 0), st), "lr_conv3d_pack_weights")
  torch.cuda.synchronize()
  return out


def _forward(x, wp, bias, relu, B, T, H, dev):
  """x [B][T][H][24][32] (device bf16) -> y [B][T][H][24][64] as float64 on the host."""
  _C, L, st = _abi()
  y = _nans((B, T, H, 24, L2.cout), dev)
  _C.check(L.lr_conv3d_forward(x.data_ptr(), wp.data_ptr(), None if bias is None else bias.data_ptr(), y.data_ptr(),
                               B, T, H, 24, L2.cin_pad, L2.cout, *GEOM, (1 if relu else 0) | 2, st), "lr_conv3d_forward")
  return _host(y, y.shape)


def _forward_pooled(x, wp, bias, B, T, H, dev):
  _C, L, st = _abi()
  pooled = _nans((B, T, H // 2, 12, L2.cout), dev)
  code = torch.full(tuple(pooled.shape), 255, dtype=U8, device=dev)
  _C.check(L.lr_conv3d_forward_pooled(x.data_ptr(), wp.data_ptr(), bias.data_ptr(), pooled.data_ptr(), code.data_ptr(),
                                      B, T, H, 24, L2.cin_pad, L2.cout, *GEOM, 1 | 2, st), "lr_conv3d_forward_pooled")
  return _host(pooled, pooled.shape), _host(code, code.shape)


def _stage_dz(pooled, code, dP, B, T, H, dev):
  """dZ [B][T][H][24][64] in memory, un-pooled by lr_unpool_code_bf16 (device bf16)."""
  _C, L, st = _abi()
  dz = _nans((B, T, H, 24, L2.cout), dev)
  wbytes = L.lr_unpool_workspace_bytes(L2.cout)
  ws = torch.full((max(int(wbytes), 16),), 0xFF, dtype=U8, device=dev)
  _C.check(L.lr_unpool_code_bf16(pooled.data_ptr(), code.data_ptr(), dP.data_ptr(), dz.data_ptr(), None, 0, ws.data_ptr(),
                                 wbytes, B * T, H, 24, L2.cout, st), "lr_unpool_code_bf16")
  return dz


def _dgrad(dz, wd, B, T, H, dev):
  _C, L, st = _abi()
  kt, kh, kw = L2.k
  dx = _nans((B, T, H, 24, L2.cin), dev)
  _C.check(L.lr_conv3d_forward(dz.data_ptr(), wd.data_ptr(), None, dx.data_ptr(), B, T, H, 24, L2.cout, L2.cin, kt, kh,
                               kw, 1, *L2.pad, 2, st), "lr_conv3d_forward(dgrad)")
  return _host(dx, dx.shape)


def _dgrad_pooled(dP, code, wd, B, T, H, dev):
  _C, L, st = _abi()
  kt, kh, kw = L2.k
  assert L.lr_conv3d_dgrad_pooled_supported(H, 24, L2.cout, L2.cin, kt, kh, kw, *L2.pad) == 2
  dx = _nans((B, T, H, 24, L2.cin), dev)
  _C.check(L.lr_conv3d_dgrad_pooled(dP.data_ptr(), code.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, T, H, 24, L2.cout,
                                    L2.cin, kt, kh, kw, *L2.pad, st), "lr_conv3d_dgrad_pooled")
  return _host(dx, dx.shape)


# ---------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_forward_full_resolution_is_exact(dev, name):
  p = _problem(name)
  c = p.case
  x, bias, wp = _bf16(p.x, dev), p.bias.to(F32).to(dev), _pack(p.w, False, dev)
  for with_bias, relu in ((False, False), (True, True)):
    got = _forward(x, wp, bias if with_bias else None, relu, c.B, c.T, c.H, dev)
    FC.compare_exact(got, p.y(with_bias, relu), "y (bias %d, relu %d)" % (with_bias, relu))


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_forward_pooled_is_exact(dev, name):
  p = _problem(name)
  c = p.case
  pooled, code = _forward_pooled(_bf16(p.x, dev), _pack(p.w, False, dev), p.bias.to(F32).to(dev), c.B, c.T, c.H, dev)
  FC.compare_exact(pooled, p.pooled_code[0], "pooled")
  FC.compare_exact(code, p.pooled_code[1], "code")


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_data_gradient_from_a_staged_dz_is_exact(dev, name):
  p = _problem(name)
  c = p.case
  dz = _stage_dz(_bf16(p.pooled_code[0], dev), p.code.to(dev).contiguous(), _bf16(p.dP, dev), c.B, c.T, c.H, dev)
  FC.compare_exact(_host(dz, p.dz_unpooled.shape), p.dz_unpooled, "dZ")
  FC.compare_exact(_dgrad(dz, _pack(p.w, True, dev), c.B, c.T, c.H, dev), p.dx_pooled, "dX")


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_data_gradient_from_the_pooled_gradient_is_exact(dev, name):
  p = _problem(name)
  c = p.case
  got = _dgrad_pooled(_bf16(p.dP, dev), p.code.to(dev).contiguous(), _pack(p.w, True, dev), c.B, c.T, c.H, dev)
  FC.compare_exact(got, p.dx_pooled, "dX")


# ---------------------------------------------------------------------------------------------------------------
# rounding level
# ---------------------------------------------------------------------------------------------------------------
class _Rounding:
  """Random non-integer operands, rounded to bf16, and the fp64 reference on them.  Bound of an output:
  2^-7 |want| (one bf16 rounding of the output) + 2^-12 conv(|x|, |w|) (fp32 accumulation: at most 4800 additions,
  each within 2^-24 of the running sum of magnitudes); no output is exempt."""

  def __init__(self):
    B, T, H = ROUND_SHAPE
    g = FC.generator("patch2mfma-rounding")
    rnd = lambda shape, scale: (torch.randn(shape, generator=g) * scale).to(BF).double()
    self.x = rnd((B, T, H, 24, L2.cin), 1.0)
    self.w = rnd((L2.cout, L2.cin) + L2.k, 0.05)
    self.dz = rnd((B, T, H, 24, L2.cout), 1.0)
    self.dP = rnd((B, T, H // 2, 12, L2.cout), 1.0)
    self.code = torch.randint(0, 5, tuple(self.dP.shape), generator=g).to(U8)
    self.z = FC.conv_forward(self.x, self.w)
    self.z_mag = FC.conv_forward(self.x.abs(), self.w.abs())
    self.dx = FC.conv_dgrad(self.dz, self.w, self.x.shape)
    self.dx_mag = FC.conv_dgrad(self.dz.abs(), self.w.abs(), self.x.shape)
    self.dzu = FC.unpool_from_code(self.code, self.dP)
    self.dxu = FC.conv_dgrad(self.dzu, self.w, self.x.shape)
    self.dxu_mag = FC.conv_dgrad(self.dzu.abs(), self.w.abs(), self.x.shape)


@functools.lru_cache(maxsize=None)
def _rounding():
  return _Rounding()


def _within(got, want, mag, name):
  bound = 2.0 ** -7 * want.abs() + 2.0 ** -12 * mag
  err = (got - want).abs()
  worst = float((err / bound.clamp_min(1e-300)).max())
  print("%s: max |got - want| %.3e, largest share of the bound %.3f" % (name, float(err.max()), worst))
  bad = ~(err <= bound)
  assert not bool(bad.any()), "%s: %d of %d outputs outside the bound, worst at %.2f x" % (name, int(bad.sum()), bad.numel(), worst)


@pytest.mark.gpu
def test_rounding_forward(dev):
  r = _rounding()
  B, T, H = ROUND_SHAPE
  x, wp = _bf16(r.x, dev), _pack(r.w, False, dev)
  bias = torch.zeros(L2.cout, dtype=F32, device=dev)   # the pooled entry takes a bias: zeros add nothing
  _within(_forward(x, wp, None, False, B, T, H, dev), r.z, r.z_mag, "y")
  # ReLU -> max-pool: both are 1-Lipschitz per window, so a pooled value is within the largest bound of its window
  pooled, code = _forward_pooled(x, wp, bias, B, T, H, dev)
  bound = 2.0 ** -7 * r.z.abs() + 2.0 ** -12 * r.z_mag
  want = FC.maxpool(r.z.clamp_min(0))
  err = (pooled - want).abs()
  print("pooled: max |got - want| %.3e" % float(err.max()))
  assert bool((err <= FC.maxpool(bound)).all())
  assert bool((code <= 4).all())


@pytest.mark.gpu
def test_rounding_data_gradient(dev):
  r = _rounding()
  B, T, H = ROUND_SHAPE
  wd = _pack(r.w, True, dev)
  _within(_dgrad(_bf16(r.dz, dev), wd, B, T, H, dev), r.dx, r.dx_mag, "dX from dZ")
  got = _dgrad_pooled(_bf16(r.dP, dev), r.code.to(dev).contiguous(), wd, B, T, H, dev)
  _within(got, r.dxu, r.dxu_mag, "dX from the pooled gradient")


@pytest.mark.gpu
def test_a_clip_computes_the_same_bits_alone_and_in_a_batch(dev):
  """Clip 0 of a two-clip launch equals the one-clip launch bit for bit: a clip's sums do not depend on which tile
  (whole or ragged, and in which row of the launch) its frames fall into."""
  r = _rounding()
  B, T, H = ROUND_SHAPE
  x, dz, dP, code = _bf16(r.x, dev), _bf16(r.dz, dev), _bf16(r.dP, dev), r.code.to(dev).contiguous()
  bias = FC.biases(L2.cout, FC.generator("patch2mfma-batch")).to(F32).to(dev)
  wp, wd = _pack(r.w, False, dev), _pack(r.w, True, dev)
  both = (_forward(x, wp, bias, False, B, T, H, dev),) + _forward_pooled(x, wp, bias, B, T, H, dev) + (
      _dgrad(dz, wd, B, T, H, dev), _dgrad_pooled(dP, code, wd, B, T, H, dev))
  x1, dz1, dP1, code1 = x[:1].contiguous(), dz[:1].contiguous(), dP[:1].contiguous(), code[:1].contiguous()
  one = (_forward(x1, wp, bias, False, 1, T, H, dev),) + _forward_pooled(x1, wp, bias, 1, T, H, dev) + (
      _dgrad(dz1, wd, 1, T, H, dev), _dgrad_pooled(dP1, code1, wd, 1, T, H, dev))
  for name, a, b in zip(("y", "pooled", "code", "dX", "dX (pooled)"), both, one):
    FC.compare_exact(a[:1], b, name)
