"""GPU: every kernel of the 3-D conv frontend (A8) against an fp64 reference, to the last bit.

The operands are small integers (tests/frontend_exact_cases.py: exact in bf16, every sum below 2^24), so every partial
sum is exact in any order and the bar is equality: there is nothing here to measure or tune.  One dropped, doubled or
leaked product moves an output by at least 1; small integers tie constantly, so the max-pool's first-maximum rule is
exercised in every window-code test.  tests/test_frontend_exact_cpu.py checks, without a GPU, that every case below
meets the conditions under which equality is the right bar, and that a one-term error at an edge is caught.

Every output is pre-filled with NaN (or with a known integer where the call accumulates), the workspaces with NaN
bit patterns.  The raw _C.lib() entry points are called, as in tests/test_gpu_frontend.py."""
import ctypes

import pytest
import torch

from tests import frontend_exact_cases as FC

pytestmark = pytest.mark.gpu

BF, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
NAN = float("nan")
DW_FILL, DB_FILL = 3.0, -2.0      # what dW / dbias hold before a call that accumulates
VARIANTS = ((False, False), (True, False), (False, True), (True, True))   # (bias, relu)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _abi():
  from lipreading_amd import _C
  return _C, _C.lib(), _C.stream_handle()


def _ids(cases):
  return [c.name for c in cases]


def _bf16(t, dev):
  return t.to(BF).to(dev).contiguous()


def _f32(t, dev):
  return t.to(F32).to(dev).contiguous()


def _nans(shape, dev, dtype=BF):
  return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def _workspace(nbytes, dev):
  return torch.full((max(int(nbytes), 16),), 0xFF, dtype=U8, device=dev)   # fp32 NaNs: nothing may be read unwritten


def _host(t, shape):
  torch.cuda.synchronize()
  return t.cpu().double().reshape(tuple(shape))


def _geom(layer):
  return tuple(layer.k) + (layer.stride,) + tuple(layer.pad)


def _pack(w, layer, flags, dev):
  """The weight operand of lr_conv3d_forward: flags & 1 = the data gradient's, flags & 6 = fragment-major."""
  _C, L, st = _abi()
  kt, kh, kw = layer.k
  shape = (layer.cin, kt * kh * kw, layer.cout) if flags & 1 else (layer.cout, kt * kh * kw, layer.cin_pad)
  w32 = _f32(w, dev)
  out = _nans(shape, dev)
  _C.check(L.lr_conv3d_pack_weights(w32.data_ptr(), out.data_ptr(), layer.cout, layer.cin, layer.cin_pad, kt, kh, kw,
                                    flags, st), "lr_conv3d_pack_weights")
  torch.cuda.synchronize()
  return out


def _first_layer_input(p, src, dev):
  """(tensor, flag): the first layer's X as bf16 NDHWC with a zero fourth channel, or as the raw uint8 clip; `-unaligned`
  puts its base 8 bytes (bf16) / 1 byte (uint8) off the alignment the kernels' wide loads need."""
  c = p.case
  if src.startswith("bf16"):
    x4 = torch.zeros(c.B, c.T, c.H, c.W, 4, dtype=torch.float64)
    x4[..., :3] = p.x
    flat = x4.reshape(-1)
    shift = 4 if src.endswith("unaligned") else 0
    buf = torch.zeros(flat.numel() + 8, dtype=BF, device=dev)
    x = buf[shift:shift + flat.numel()]
    x.copy_(flat.to(BF))
    assert x.data_ptr() % 16 == 2 * shift
    return x, 0
  flat = p.clip.reshape(-1)
  shift = 1 if src.endswith("unaligned") else 0
  buf = torch.zeros(flat.numel() + 8, dtype=U8, device=dev)
  x = buf[shift:shift + flat.numel()]
  x.copy_(flat)
  assert x.data_ptr() % 4 == shift
  return x, 1


def _patch_bits(c):
  """(forward bit, data-gradient bit) of lr_conv3d_patch_supported; the case's group says which they must be."""
  _C, L, st = _abi()
  layer = c.layer
  frag = L.lr_conv3d_patch_supported(c.H, c.W, layer.cin_pad, layer.cout, *_geom(layer))
  fragd = L.lr_conv3d_patch_supported(c.H, c.W, layer.cout, layer.cin, *_geom(layer))
  want = {"patch2": 2, "patch3": 4, "igemm": 0}[c.group]
  assert (frag, fragd) == (want, want), (c.name, frag, fragd)
  return frag, fragd


# ---------------------------------------------------------------------------------------------------------------
# elementwise stages
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,H,W", FC.CLIP_CASES)
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_clip_to_ndhwc(dev, dtype, frames, H, W):
  """lr_clip_to_ndhwc_bf16: bytes {0, 255} / floats {0, 1} -> {0, 1}, channels last, the fourth channel zero."""
  _C, L, st = _abi()
  clip = FC.clip_bytes(1, frames, H, W, FC.generator("clip-%d-%dx%d" % (frames, H, W)))
  src = clip.to(dev) if dtype == "u8" else (clip.float() / 255.0).to(dev)
  out = _nans((frames, H, W, 4), dev)
  _C.check(L.lr_clip_to_ndhwc_bf16(src.data_ptr(), 1 if dtype == "u8" else 0, out.data_ptr(), frames, H, W, st))
  want = torch.zeros(1, frames, H, W, 4, dtype=torch.float64)
  want[..., :3] = FC.clip_to_ndhwc(clip)
  FC.compare_exact(_host(out, want.shape), want, "ndhwc")


def test_bf16_f32_conversions(dev):
  _C, L, st = _abi()
  v = torch.arange(-256, 257, dtype=torch.float64)
  src = _f32(v, dev)
  half = _nans(v.shape, dev)
  back = _nans(v.shape, dev, F32)
  _C.check(L.lr_f32_to_bf16(src.data_ptr(), half.data_ptr(), v.numel(), st))
  _C.check(L.lr_bf16_to_f32(half.data_ptr(), back.data_ptr(), v.numel(), st))
  FC.compare_exact(_host(half, v.shape), v, "bf16")
  FC.compare_exact(_host(back, v.shape), v, "f32")


@pytest.mark.parametrize("C,frames,H,W", FC.POOL_CASES)
def test_maxpool(dev, C, frames, H, W):
  _C, L, st = _abi()
  act, _ = FC.pool_problem(C, frames, H, W)
  want = FC.maxpool(act)
  out = _nans(want.shape, dev)
  a = _bf16(act, dev)
  _C.check(L.lr_maxpool_hw2_bf16(a.data_ptr(), out.data_ptr(), frames, H, W, C, st))
  FC.compare_exact(_host(out, want.shape), want, "pooled")


@pytest.mark.parametrize("C,frames,H,W", FC.POOL_CASES)
@pytest.mark.parametrize("kernel", ["relu_mask", "code"])
def test_unpool(dev, kernel, C, frames, H, W):
  """lr_unpool_relu_mask_bf16 (from the activation) and lr_unpool_code_bf16 (from the pooled activation and the window
  codes): the window's gradient goes to its FIRST maximum if that is > 0 — a quarter of these windows tie — and dbias
  is its column sum, written, added to a known value, or skipped (NULL)."""
  _C, L, st = _abi()
  act, dP = FC.pool_problem(C, frames, H, W)
  pooled, code = FC.relu_pool(act)
  want = FC.unpool_from_act(act, dP)
  want_db = FC.bias_grad(want)
  a, g, pl, cd = _bf16(act, dev), _bf16(dP, dev), _bf16(pooled, dev), code.to(dev)
  wbytes = L.lr_unpool_workspace_bytes(C)
  for dbias in ("null", 0, 1):
    dz = _nans(want.shape, dev)
    db = torch.full((C,), DB_FILL if dbias == 1 else NAN, dtype=F32, device=dev)
    ws = _workspace(wbytes, dev)
    dbp = None if dbias == "null" else db.data_ptr()
    acc = 1 if dbias == 1 else 0
    if kernel == "relu_mask":
      _C.check(L.lr_unpool_relu_mask_bf16(a.data_ptr(), g.data_ptr(), dz.data_ptr(), dbp, acc, ws.data_ptr(), wbytes,
                                          frames, H, W, C, st), "lr_unpool_relu_mask_bf16")
    else:
      _C.check(L.lr_unpool_code_bf16(pl.data_ptr(), cd.data_ptr(), g.data_ptr(), dz.data_ptr(), dbp, acc, ws.data_ptr(),
                                     wbytes, frames, H, W, C, st), "lr_unpool_code_bf16")
    FC.compare_exact(_host(dz, want.shape), want, "dZ (dbias %s)" % dbias)
    if dbias != "null":
      FC.compare_exact(_host(db, (C,)), want_db + DB_FILL * acc, "dbias (accumulate %d)" % acc, ("channel",))


# ---------------------------------------------------------------------------------------------------------------
# weight operands
# ---------------------------------------------------------------------------------------------------------------
def _plain_operand(w, layer, dgrad):
  """out[Cout][taps][Cin_pad] (channels >= Cin zero), or out[Cin][taps][Cout] with the taps flipped."""
  taps = layer.k[0] * layer.k[1] * layer.k[2]
  w3 = w.reshape(layer.cout, layer.cin, taps)
  if dgrad:
    return w3.flip(2).permute(1, 2, 0).contiguous()
  out = torch.zeros(layer.cout, taps, layer.cin_pad, dtype=torch.float64)
  out[:, :, :layer.cin] = w3.permute(0, 2, 1)
  return out


def test_pack_weights_plain_layouts(dev):
  """lr_conv3d_pack_weights and _multi, the two documented plain layouts of every layer (the fragment-major orders
  are internal: the convolutions below read them)."""
  _C, L, st = _abi()
  items = []
  for lname, layer in (("l1", FC.L1), ("l2", FC.L2), ("l3", FC.L3)):
    w = FC.weights(layer, FC.generator("pack-" + lname), keep=0.8)
    for dgrad in (0, 1):
      want = _plain_operand(w, layer, dgrad)
      FC.compare_exact(_host(_pack(w, layer, dgrad, dev), want.shape), want, "%s dgrad=%d" % (lname, dgrad),
                       ("row", "tap", "channel"))
      items.append((_f32(w, dev), _nans(want.shape, dev), layer, dgrad, want, lname))
  n = len(items)
  arr = lambda vals: (ctypes.c_int * n)(*vals)
  ptrs = (ctypes.c_void_p * n)(*[it[0].data_ptr() for it in items])
  outs = (ctypes.c_void_p * n)(*[it[1].data_ptr() for it in items])
  _C.check(L.lr_conv3d_pack_weights_multi(n, ptrs, outs, arr([it[2].cout for it in items]),
                                          arr([it[2].cin for it in items]), arr([it[2].cin_pad for it in items]),
                                          arr([it[2].k[0] for it in items]), arr([it[2].k[1] for it in items]),
                                          arr([it[2].k[2] for it in items]), arr([it[3] for it in items]), st),
           "lr_conv3d_pack_weights_multi")
  for _, out, _, dgrad, want, lname in items:
    FC.compare_exact(_host(out, want.shape), want, "multi %s dgrad=%d" % (lname, dgrad), ("row", "tap", "channel"))


# ---------------------------------------------------------------------------------------------------------------
# first layer (lr_conv1.hip)
# ---------------------------------------------------------------------------------------------------------------
SOURCES = ["bf16", "u8", "bf16-unaligned", "u8-unaligned"]


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("case", FC.cases("first", "fwd"), ids=_ids(FC.cases("first", "fwd")))
def test_first_layer_forward(dev, case, src):
  """lr_conv3d_forward on the first layer's geometry from the bf16 copy and from the raw clip (flags & 8), aligned for
  the pair loads and not, with and without bias and ReLU.  Up to 768 persistent workgroups: one tile each in the small
  cases, two in B28T7, two or three in B55T7, whose walks cross the ends of windows, tile rows and clips."""
  _C, L, st = _abi()
  p, layer = FC.problem(case.name), case.layer
  x, u8 = _first_layer_input(p, src, dev)
  wp = _pack(p.w, layer, 0, dev)
  bias = _f32(p.bias, dev)
  for with_bias, relu in VARIANTS:
    want = p.y(with_bias, relu)
    y = _nans(want.shape, dev)
    _C.check(L.lr_conv3d_forward(x.data_ptr(), wp.data_ptr(), bias.data_ptr() if with_bias else None, y.data_ptr(),
                                 case.B, case.T, case.H, case.W, layer.cin_pad, layer.cout, *_geom(layer),
                                 (1 if relu else 0) | (8 if u8 else 0), st), "lr_conv3d_forward")
    FC.compare_exact(_host(y, want.shape), want, "y (bias %d, relu %d)" % (with_bias, relu))


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("case", FC.cases("first", "fwd_pooled"), ids=_ids(FC.cases("first", "fwd_pooled")))
def test_first_layer_forward_pooled(dev, case, src):
  _C, L, st = _abi()
  p, layer = FC.problem(case.name), case.layer
  assert L.lr_conv3d_pool_fusion_supported(case.H, case.W, layer.cin_pad, layer.cout, *_geom(layer)) == 1
  x, u8 = _first_layer_input(p, src, dev)
  wp = _pack(p.w, layer, 0, dev)
  bias = _f32(p.bias, dev)
  want_p, want_c = p.pooled_code
  pooled = _nans(want_p.shape, dev)
  code = torch.full(tuple(want_c.shape), 255, dtype=U8, device=dev)
  _C.check(L.lr_conv3d_forward_pooled(x.data_ptr(), wp.data_ptr(), bias.data_ptr(), pooled.data_ptr(), code.data_ptr(),
                                      case.B, case.T, case.H, case.W, layer.cin_pad, layer.cout, *_geom(layer),
                                      1 | (8 if u8 else 0), st), "lr_conv3d_forward_pooled")
  FC.compare_exact(_host(pooled, want_p.shape), want_p, "pooled")
  FC.compare_exact(_host(code, want_c.shape), want_c, "code")


def _check_wgrad(got_w, got_b, want_w, want_b, accumulate):
  FC.compare_exact(_host(got_w, want_w.shape), want_w + DW_FILL * accumulate, "dW (accumulate %d)" % accumulate,
                   FC.WGT_AXES)
  FC.compare_exact(_host(got_b, want_b.shape), want_b + DB_FILL * accumulate, "dbias (accumulate %d)" % accumulate,
                   ("channel",))


def _wgrad_outputs(layer, accumulate, dev):
  dw = torch.full((layer.cout, layer.cin) + tuple(layer.k), DW_FILL if accumulate else NAN, dtype=F32, device=dev)
  db = torch.full((layer.cout,), DB_FILL if accumulate else NAN, dtype=F32, device=dev)
  return dw, db


def _run_wgrad(p, x, dev, accumulate):
  """lr_conv3d_wgrad on the case's x (bf16, channels padded) and dz.  Which kernel a case reaches is the host
  dispatch's choice, restated and checked per case in test_frontend_exact_cpu.py (the transpose-read kernel's tile
  table limit included)."""
  _C, L, st = _abi()
  c, layer = p.case, p.case.layer
  dz = _bf16(p.dz, dev)
  wbytes = L.lr_conv3d_wgrad_workspace_bytes(layer.cout, layer.cin_pad, *layer.k)
  ws = _workspace(wbytes, dev)
  dw, db = _wgrad_outputs(layer, accumulate, dev)
  _C.check(L.lr_conv3d_wgrad(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), wbytes,
                             accumulate, c.B, c.T, c.H, c.W, layer.cin_pad, layer.cin, layer.cout, *_geom(layer), st),
           "lr_conv3d_wgrad")
  want = p.expected("wgrad")
  _check_wgrad(dw, db, want["dw"][0], want["dbias"][0], accumulate)


def _run_wgrad_pooled(p, x, flags, kind, dev, accumulate):
  """lr_conv3d_wgrad_pooled on the case's x, window codes and pooled gradient (`pooled` is not read: NULL)."""
  _C, L, st = _abi()
  c, layer = p.case, p.case.layer
  geom = (c.H, c.W, layer.cin_pad, layer.cin, layer.cout) + _geom(layer)
  assert L.lr_conv3d_wgrad_pooled_supported(*geom) == kind
  assert L.lr_conv3d_wgrad_pooled_supported_frames(c.B * c.T, *geom) == kind
  dP, code = _bf16(p.dP, dev), p.code.to(dev).contiguous()
  wbytes = L.lr_conv3d_wgrad_workspace_bytes(layer.cout, layer.cin_pad, *layer.k)
  ws = _workspace(wbytes, dev)
  dw, db = _wgrad_outputs(layer, accumulate, dev)
  _C.check(L.lr_conv3d_wgrad_pooled(x.data_ptr(), None, code.data_ptr(), dP.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                    ws.data_ptr(), wbytes, accumulate, c.B, c.T, *geom, flags, st),
           "lr_conv3d_wgrad_pooled")
  want = p.expected("wgrad_pooled")
  _check_wgrad(dw, db, want["dw"][0], want["dbias"][0], accumulate)


def _with_accumulate(cases):
  return [pytest.param(c, a, id="%s-acc%d" % (c.name, a)) for c in cases for a in (0, 1)]


@pytest.mark.parametrize("case,accumulate", _with_accumulate(FC.cases("first", "wgrad")))
def test_first_layer_weight_gradient(dev, case, accumulate):
  """lr_conv3d_wgrad, first layer: 256 persistent workgroups walk 16 x 16 output tiles: two (B33T2, B10T7), three or
  four (B28T7), six or seven (B55T7: the frame ring goes round, loads run three tiles ahead); the smaller cases leave
  most of them idle."""
  p = FC.problem(case.name)
  x, _ = _first_layer_input(p, "bf16", dev)
  _run_wgrad(p, x, dev, accumulate)


@pytest.mark.parametrize("src", ["bf16", "u8", "u8-unaligned"])
@pytest.mark.parametrize("case,accumulate", _with_accumulate(FC.cases("first", "wgrad_pooled")))
def test_first_layer_weight_gradient_pooled(dev, case, accumulate, src):
  """lr_conv3d_wgrad_pooled, first layer, flags 0 (bf16 X) and 1 (the raw clip, read in dwords where the width and the
  base allow, else in bytes: 39 x 35 and the unaligned base): dZ rebuilt from dP and the codes."""
  p = FC.problem(case.name)
  x, u8 = _first_layer_input(p, src, dev)
  _run_wgrad_pooled(p, x, u8, 1, dev, accumulate)


# ---------------------------------------------------------------------------------------------------------------
# layers 2 and 3: forward and data gradient (patch-resident kernels and the implicit GEMM)
# ---------------------------------------------------------------------------------------------------------------
PATCH = FC.cases("patch2") + FC.cases("patch3")
CONV = PATCH + FC.cases("igemm")


@pytest.mark.parametrize("case", CONV, ids=_ids(CONV))
def test_forward(dev, case):
  """lr_conv3d_forward: the 24-wide and the 12 x 12 patch-resident kernels (fragment-major weights) and the implicit
  GEMM at (32, 64) and (64, 96), with and without bias and ReLU."""
  _C, L, st = _abi()
  p, layer = FC.problem(case.name), case.layer
  frag, _ = _patch_bits(case)
  x, bias = _bf16(p.x, dev), _f32(p.bias, dev)
  wp = _pack(p.w, layer, frag, dev)
  for with_bias, relu in VARIANTS:
    want = p.y(with_bias, relu)
    y = _nans(want.shape, dev)
    _C.check(L.lr_conv3d_forward(x.data_ptr(), wp.data_ptr(), bias.data_ptr() if with_bias else None, y.data_ptr(),
                                 case.B, case.T, case.H, case.W, layer.cin_pad, layer.cout, *_geom(layer),
                                 (1 if relu else 0) | frag, st), "lr_conv3d_forward")
    FC.compare_exact(_host(y, want.shape), want, "y (bias %d, relu %d)" % (with_bias, relu))


@pytest.mark.parametrize("case", CONV, ids=_ids(CONV))
def test_data_gradient(dev, case):
  """The data gradient as lr_conv3d_forward on dZ with the flipped, channel-transposed operand: patch-resident
  (64 -> 32 at 24 wide, 96 -> 64 at 12 x 12) and the implicit GEMM at (64, 32) and (96, 64)."""
  _C, L, st = _abi()
  p, layer = FC.problem(case.name), case.layer
  _, fragd = _patch_bits(case)
  dz = _bf16(p.dz, dev)
  wd = _pack(p.w, layer, 1 | fragd, dev)
  dx = _nans(p.dx.shape, dev)
  kt, kh, kw = layer.k
  _C.check(L.lr_conv3d_forward(dz.data_ptr(), wd.data_ptr(), None, dx.data_ptr(), case.B, case.T, case.H, case.W,
                               layer.cout, layer.cin, kt, kh, kw, 1, *layer.pad, fragd, st), "lr_conv3d_forward(dgrad)")
  FC.compare_exact(_host(dx, p.dx.shape), p.dx, "dX")


@pytest.mark.parametrize("case", PATCH, ids=_ids(PATCH))
def test_forward_pooled(dev, case):
  """lr_conv3d_forward_pooled, layers 2 and 3: ReLU -> MaxPool in the epilogue, pooled value and window code."""
  _C, L, st = _abi()
  p, layer = FC.problem(case.name), case.layer
  frag, _ = _patch_bits(case)
  assert L.lr_conv3d_pool_fusion_supported(case.H, case.W, layer.cin_pad, layer.cout, *_geom(layer)) == 1
  x, bias = _bf16(p.x, dev), _f32(p.bias, dev)
  wp = _pack(p.w, layer, frag, dev)
  want_p, want_c = p.pooled_code
  pooled = _nans(want_p.shape, dev)
  code = torch.full(tuple(want_c.shape), 255, dtype=U8, device=dev)
  _C.check(L.lr_conv3d_forward_pooled(x.data_ptr(), wp.data_ptr(), bias.data_ptr(), pooled.data_ptr(), code.data_ptr(),
                                      case.B, case.T, case.H, case.W, layer.cin_pad, layer.cout, *_geom(layer), 1 | frag,
                                      st), "lr_conv3d_forward_pooled")
  FC.compare_exact(_host(pooled, want_p.shape), want_p, "pooled")
  FC.compare_exact(_host(code, want_c.shape), want_c, "code")


@pytest.mark.parametrize("case", PATCH, ids=_ids(PATCH))
def test_data_gradient_pooled(dev, case):
  """lr_conv3d_dgrad_pooled: dX from the pooled gradient and the window codes, un-pooled on the way into LDS."""
  _C, L, st = _abi()
  p, layer = FC.problem(case.name), case.layer
  kt, kh, kw = layer.k
  fragd = L.lr_conv3d_dgrad_pooled_supported(case.H, case.W, layer.cout, layer.cin, kt, kh, kw, *layer.pad)
  assert fragd == _patch_bits(case)[1]
  dP, code = _bf16(p.dP, dev), p.code.to(dev).contiguous()
  wd = _pack(p.w, layer, 1 | fragd, dev)
  dx = _nans(p.dx_pooled.shape, dev)
  _C.check(L.lr_conv3d_dgrad_pooled(dP.data_ptr(), code.data_ptr(), wd.data_ptr(), dx.data_ptr(), case.B, case.T, case.H,
                                    case.W, layer.cout, layer.cin, kt, kh, kw, *layer.pad, st), "lr_conv3d_dgrad_pooled")
  FC.compare_exact(_host(dx, p.dx_pooled.shape), p.dx_pooled, "dX")


# ---------------------------------------------------------------------------------------------------------------
# layers 2 and 3: weight gradient (transpose-read, tap-stationary, split-pixel)
# ---------------------------------------------------------------------------------------------------------------
WGRAD = FC.cases("tr2") + FC.cases("ts") + FC.cases("split")


@pytest.mark.parametrize("case,accumulate", _with_accumulate(WGRAD))
def test_weight_gradient(dev, case, accumulate):
  """lr_conv3d_wgrad on the stride-1 layers: the transpose-read kernel (24 / 12 wide), the tap-stationary kernel
  (<32, 2, 7>, <64, 3, 5>, <32, 2, 3>) and the split-pixel kernel (<32, 2, 4>, <64, 3, 2>)."""
  p = FC.problem(case.name)
  _run_wgrad(p, _bf16(p.x, dev), dev, accumulate)


@pytest.mark.parametrize("case,accumulate", _with_accumulate(FC.cases("tr2", "wgrad_pooled")))
def test_weight_gradient_pooled(dev, case, accumulate):
  """lr_conv3d_wgrad_pooled on layers 2 and 3: the transpose-read kernel un-pools dP by the codes on its way into
  LDS; dbias leaves out the windows whose code is 4."""
  p = FC.problem(case.name)
  _run_wgrad_pooled(p, _bf16(p.x, dev), 0, 2, dev, accumulate)
