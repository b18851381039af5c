"""Shared by tests/test_frontend_exact_cpu.py and tests/test_gpu_frontend_exact.py: exact-integer cases for the 3-D
conv frontend and their fp64 reference.  Host only: no GPU, no import of the extension.

Every frontend kernel multiplies bf16 operands and accumulates in fp32.  With operands that are small integers (exact
in bf16) and every sum below 2^24, every partial sum is exact in any order — any tile split, any split-K slab count,
any MFMA schedule — so the fp32 outputs (dW, dbias) equal the fp64 reference exactly, and the bf16 outputs
(activations, pooled values, dX) equal it exactly while they are integers of magnitude <= 256 (every such integer is
a bf16 value).  test_frontend_exact_cpu.py checks those conditions on the reference for every case below; the GPU file
then asks for equality, and a single dropped, doubled or leaked product moves an output by at least 1.

Operands: activations and gradients from {-1, 0, 1}; pool-only inputs from {-2..3}; weights from {-1, 0, 1} with
about half (1 - keep) of the entries zeroed; biases in [-3, 3]; raw clips of the bytes {0, 255} only (the kernels
compute byte * (1.f/255.f) and round to bf16: 0 and 1), fp32 clips of the same {0, 1}.

All reference functions take and return NDHWC ([B][T][H][W][C]) float64 tensors; weights are torch's Conv3d layout
[Cout][Cin][KT][KH][KW].
"""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BF16_EXACT = 256          # every integer of magnitude <= 256 is a bf16 value
F32_EXACT = 1 << 24       # every integer of magnitude < 2^24 is an fp32 value, and so is every partial sum below it

ACT_AXES = ("clip", "frame", "row", "column", "channel")
WGT_AXES = ("output-channel", "input-channel", "kt", "kh", "kw")

Layer = collections.namedtuple("Layer", "cin cin_pad cout k stride pad")
L1 = Layer(3, 4, 32, (3, 5, 5), 2, (1, 2, 2))
L2 = Layer(32, 32, 64, (3, 5, 5), 1, (1, 2, 2))
L3 = Layer(64, 64, 96, (3, 3, 3), 1, (1, 1, 1))
L2K3 = Layer(32, 32, 64, (3, 3, 3), 1, (1, 1, 1))   # no layer of the frontend: the tap-stationary kernel's <32, 2, 3>


# ---------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------
def compare_exact(got, want, name, axes=None):
  """Values must be equal element by element (-0.0 equals 0.0; a NaN equals nothing).  On a mismatch the
  AssertionError carries the count and the first few indices, named by `axes`, so that it names the tile edge."""
  got = np.asarray(got.detach().cpu().double() if torch.is_tensor(got) else got, dtype=np.float64)
  want = np.asarray(want.detach().cpu().double() if torch.is_tensor(want) else want, dtype=np.float64)
  assert got.shape == want.shape, "%s: shape %s, expected %s" % (name, got.shape, want.shape)
  bad = ~(got == want)
  n = int(bad.sum())
  if n == 0:
    return
  if axes is None:
    axes = ACT_AXES if got.ndim == 5 else tuple("axis%d" % i for i in range(got.ndim))
  lines = []
  for idx in np.argwhere(bad)[:8]:
    where = ", ".join("%s %d" % (a, i) for a, i in zip(axes, idx))
    lines.append("  [%s]: got %r, expected %r" % (where, got[tuple(idx)], want[tuple(idx)]))
  raise AssertionError("%s: %d of %d values differ; first ones:\n%s" % (name, n, got.size, "\n".join(lines)))


# ---------------------------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------------------------
def _ncdhw(a):
  return a.permute(0, 4, 1, 2, 3)


def _ndhwc(a):
  return a.permute(0, 2, 3, 4, 1).contiguous()


def conv_forward(x, w, bias=None, relu=False, stride=1, pad=(1, 2, 2)):
  y = F.conv3d(_ncdhw(x.double()), w.double(), None if bias is None else bias.double(), stride=(1, stride, stride),
               padding=pad)
  y = _ndhwc(y)
  return y.clamp_min(0) if relu else y


def conv_dgrad(dz, w, in_shape, stride=1, pad=(1, 2, 2)):
  """dX [B][T][Hin][Win][Cin] of conv_forward at an input of in_shape (NDHWC), by autograd in double."""
  x = torch.zeros(in_shape, dtype=torch.float64, requires_grad=True)
  conv_forward(x, w, None, False, stride, pad).backward(dz.double())
  return x.grad


def conv_wgrad(x, dz, w_shape, stride=1, pad=(1, 2, 2)):
  """dW [Cout][Cin][KT][KH][KW] of conv_forward, by autograd in double."""
  w = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
  conv_forward(x, w, None, False, stride, pad).backward(dz.double())
  return w.grad


def bias_grad(dz):
  return dz.double().sum((0, 1, 2, 3))


def _windows(a):
  """[4][B][T][H/2][W/2][C]: the 2x2 windows' positions in row-major order."""
  a = a.numpy() if torch.is_tensor(a) else a
  return np.stack([a[:, :, 0::2, 0::2], a[:, :, 0::2, 1::2], a[:, :, 1::2, 0::2], a[:, :, 1::2, 1::2]])


def _argmax(s, first=True):
  return np.argmax(s, axis=0) if first else 3 - np.argmax(s[::-1], axis=0)


def maxpool(a):
  return torch.from_numpy(_windows(a).max(0))


def relu_pool(z, first=True):
  """ReLU -> MaxPool((1,2,2)): (pooled, code); code 4 where the window's maximum is <= 0, else the row-major index of
  its first maximum (first=False: of its last — the wrong rule, for the sensitivity checks)."""
  s = _windows(z)
  m = s.max(0)
  code = np.where(m > 0, _argmax(s, first), 4).astype(np.uint8)
  return torch.from_numpy(np.maximum(m, 0)), torch.from_numpy(code)


def _scatter(arg, live, dP):
  dP = dP.numpy() if torch.is_tensor(dP) else dP
  B, T, h, w, C = dP.shape
  dz = np.zeros((B, T, 2 * h, 2 * w, C))
  for j in range(4):
    dz[:, :, j // 2::2, j % 2::2] = np.where(live & (arg == j), dP, 0.0)
  return torch.from_numpy(dz)


def unpool_from_act(act, dP, first=True):
  """Backward of ReLU -> MaxPool from the full-resolution activation (before or after ReLU: the same windows)."""
  s = _windows(act)
  return _scatter(_argmax(s, first), s.max(0) > 0, dP)


def unpool_from_code(code, dP):
  code = code.numpy() if torch.is_tensor(code) else code
  return _scatter(code, code < 4, dP)


def pool_ties(z):
  """Per window of z: (positive, tied, first): the maximum is > 0; it occurs more than once; its first position."""
  s = _windows(z)
  m = s.max(0)
  return m > 0, (s == m).sum(0) > 1, np.argmax(s, axis=0)


# ---------------------------------------------------------------------------------------------------------------
# seeded operands
# ---------------------------------------------------------------------------------------------------------------
def generator(name):
  return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ternary(shape, g):
  return torch.randint(-1, 2, tuple(shape), generator=g).double()


def pool_values(shape, g):
  return torch.randint(-2, 4, tuple(shape), generator=g).double()


def weights(layer, g, keep=0.5):
  shape = (layer.cout, layer.cin) + layer.k
  return ternary(shape, g) * (torch.rand(shape, generator=g) < keep).double()


def biases(cout, g):
  return torch.randint(-3, 4, (cout,), generator=g).double()


def clip_bytes(B, T, H, W, g):
  """uint8 [B][T][3][H][W] of the bytes 0 and 255."""
  return (torch.randint(0, 2, (B, T, 3, H, W), generator=g) * 255).to(torch.uint8)


def clip_to_ndhwc(clip):
  """What lr_clip_to_ndhwc_bf16 makes of a {0, 255} byte clip or a {0, 1} fp32 clip, without the zero fourth channel:
  [B][T][H][W][3] float64 of {0, 1}."""
  x = clip.double() / 255.0 if clip.dtype == torch.uint8 else clip.double()
  return x.permute(0, 1, 3, 4, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------
# which kernel a shape reaches: a restatement of the host dispatch in lipreading_amd/csrc/lr_conv.hip (conv_forward_impl,
# lr_conv3d_wgrad), so that the case table can say — and the CPU test can check — which kernel each case is for
# ---------------------------------------------------------------------------------------------------------------
def out_hw(layer, H, W):
  (_, kh, kw), s, (_, ph, pw) = layer.k, layer.stride, layer.pad
  return (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1


def patch_bit(H, W, cin, cout, k):
  """lr_conv3d_patch_supported for a stride-1 'same' layer."""
  if k == (3, 5, 5) and W == 24 and H > 0 and H % 8 == 0 and (cin, cout) in ((32, 64), (64, 32)):
    return 2
  if k == (3, 3, 3) and W == 12 and H == 12 and (cin, cout) in ((64, 96), (96, 64)):
    return 4
  return 0


TR2_SLOTS, TS_SLOTS = 85, 85          # workgroups per temporal tap: LR_CONV_TR2_SLOTS, kTsWgsPerKt
C1_TILE, C1_FWD_WGS, C1_WGRAD_WGS = 16, 768, 256   # lr_conv1.hip: C1_T, LR_C1_FWD_WGS; LR_CONV1_WGRAD_WGS


def tr2_tile_rows(layer, H):
  """Rows per tile of the transpose-read weight gradient (lr_conv_wgrad.hip: tr2_tile_rows), 0: not its shape."""
  kt, kh, kw = layer.k
  if H % 6 == 0:
    return 6
  return 4 if (kh, kw) == (5, 5) and H % 4 == 0 else 0


def tr2_table_fits(layer, frames, H):
  """lr_conv_wgrad_tr2_supported: the tile table, (tiles of a workgroup + 1) x 32 bytes, has to fit in what the two
  LDS buffers of Tr2<CIN, MT, KH, KW, W, 2, TH> leave of 160 KB."""
  th = tr2_tile_rows(layer, H)
  if not th or frames <= 0:
    return False
  (kt, kh, kw), W = layer.k, (24 if layer.cin_pad == 32 else 12)
  ch, mt = layer.cin_pad // 32, layer.cout // 32
  xunits = ch * 2 * (th + kh - 1) * (W + kw - 1) * 4
  zunits = mt * 2 * th * W * 4
  buf = ((xunits + 255) // 256 + (zunits + 255) // 256) * 4096
  ntile = ((frames + 1) // 2) * (H // th)
  return ((ntile + TR2_SLOTS - 1) // TR2_SLOTS + 1) * 32 <= 160 * 1024 - 2 * buf


def ts_tile_rows(layer, H, W):
  """Rows per tile (TY) of the tap-stationary weight gradient as lr_conv3d_wgrad sizes it, 0 where no tile fits or
  the kernel has no instantiation for the layer."""
  kt, kh, kw = layer.k
  ho, wo = out_hw(layer, H, W)
  cin, mt = layer.cin_pad, layer.cout // 32
  units = kh * kw * (cin // 32)
  if layer.stride != 1 or cin not in (32, 64) or units > 28:
    return 0
  txp = (wo + 7) // 8 * 8
  ty = min(192 // txp, ho)

  def fits(t):
    lds = (t * txp * (mt * 32 + 8) + (t + kh - 1) * (txp + kw - 1) * (cin + 8)) * 2
    return ((t * txp) % 16 == 0 and lds <= 60 * 1024 and t * txp * mt * 4 <= 6 * 256
            and (t + kh - 1) * (txp + kw - 1) * (cin // 8) <= 6 * 256)
  while ty > 1 and not fits(ty):
    ty -= 1
  if fits(ty) and ((cin, mt, (units + 3) // 4) in ((32, 2, 7), (64, 3, 5), (32, 2, 3))):
    return ty
  return 0


def wgrad_path(layer, frames, H, W):
  """'first', 'tr2' (transpose-read, lr_conv_wgrad.hip), 'ts' (tap-stationary) or 'split' (split-pixel), as
  lr_conv3d_wgrad chooses for B * T = frames."""
  if layer.cin_pad == 4:
    return "first"
  kt, kh, kw = layer.k
  l2 = layer.cin_pad == 32 and layer.cout == 64 and (kh, kw) == (5, 5) and W == 24 and H % 4 == 0
  l3 = layer.cin_pad == 64 and layer.cout == 96 and (kh, kw) == (3, 3) and W == 12 and H % 6 == 0
  if (l2 or l3) and tr2_table_fits(layer, frames, H):
    return "tr2"
  return "ts" if ts_tile_rows(layer, H, W) else "split"


def split_stages(layer, frames, H, W):
  """Stages of 128 pixels (WG_PIX) that a workgroup of the split-pixel weight gradient contracts: lr_conv3d_wgrad
  splits the pixels into at most wgrad_splits ranges of whole stages."""
  ho, wo = out_hw(layer, H, W)
  ktot = layer.k[0] * layer.k[1] * layer.k[2] * layer.cin_pad
  nc = {32: 5, 64: 4}.get(layer.cout, 2) * 32
  splits = min(512, max(16, 1024 // ((ktot + nc - 1) // nc)))
  m = frames * ho * wo
  return ((m + splits - 1) // splits + 127) // 128


def first_layer_walks(case, nwg):
  """The first layer's persistent kernels (lr_conv1.hip: c1_tile, c1_next): tile q = seq * T + t with seq = (clip,
  ty, tx), 16 x 16 outputs each; workgroup i of min(nwg, tiles) walks tiles [N i / G, N (i + 1) / G).  Returns one
  list of (clip, ty, tx, t) per workgroup."""
  ho, wo = out_hw(case.layer, case.H, case.W)
  tx, ty = (wo + C1_TILE - 1) // C1_TILE, (ho + C1_TILE - 1) // C1_TILE
  n = case.B * case.T * tx * ty
  g = min(nwg, n)
  walks = []
  for i in range(g):
    walk = []
    for q in range(n * i // g, n * (i + 1) // g):
      seq, t = divmod(q, case.T)
      walk.append((seq // (tx * ty), (seq // tx) % ty, seq % tx, t))
    walks.append(walk)
  return walks


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name group layer B T H W ops keep")


def _case(group, lname, layer, B, T, H, W, ops, keep=0.5):
  return Case("%s-%s-B%dT%d-%dx%d" % (group, lname, B, T, H, W), group, layer, B, T, H, W, tuple(ops), keep)


def _build_cases():
  cases = []
  # first layer (lr_conv1.hip): persistent workgroups walk 16 x 16 output tiles, frame after frame of one spatial
  # window, then the next window, then the next clip.  32x32: one tile per frame; 40x36 -> 20x18: four ragged tiles;
  # 19x21 -> 10x11: an odd width (per-pixel loads), no pooling.  In the B2T3 and B1T1 cases every workgroup has one
  # tile (24 at most, for 768 / 256 workgroups); B1T1 leaves both temporal neighbours outside the clip.
  for H, W in ((32, 32), (40, 36), (19, 21)):
    for B, T in ((2, 3), (1, 1)):
      pool = H % 4 == 0 and W % 4 == 0
      cases.append(_case("first", "l1", L1, B, T, H, W,
                         ("fwd", "wgrad") + (("fwd_pooled", "wgrad_pooled") if pool else ())))
  # the walks (test_frontend_exact_cpu.py counts them).  B33T2 at 40x36: 264 tiles, eight workgroups of the weight
  # gradient walk two.  B10T7: 280 tiles, 24 of its workgroups walk two, T = 7.  B28T7: 784 tiles: 16 of the forward's
  # 768 workgroups walk two, the weight gradient's 256 walk three or four.  B55T7: 1540 tiles: the forward's walk two
  # or three, the weight gradient's six or seven (its four-slot frame ring goes round, its loads run three tiles
  # ahead); walks cross t >= 3, the end of a window (t = 6 -> 0), of a tile row, of a frame's tiles and of a clip.
  every = ("fwd", "fwd_pooled", "wgrad", "wgrad_pooled")
  cases.append(_case("first", "l1", L1, 33, 2, 40, 36, ("wgrad", "wgrad_pooled")))
  cases.append(_case("first", "l1", L1, 10, 7, 40, 36, ("wgrad", "wgrad_pooled")))
  cases.append(_case("first", "l1", L1, 28, 7, 40, 36, every))
  cases.append(_case("first", "l1", L1, 55, 7, 40, 36, every))
  # 39x35 -> 20x18 is a width that is no multiple of 4, where the weight gradient reads the raw clip in bytes
  cases.append(_case("first", "l1", L1, 1, 2, 39, 35, ("wgrad", "wgrad_pooled")))
  # layer 2, patch-resident (lr_conv_patch.hip: tiles of 4 frames x 8 rows x 24 columns): B3T7 = 21 frames, a ragged
  # last tile and clip boundaries inside tiles; B1T1, B2T2: tiles that are mostly past the end, T <= 2
  for H in (24, 16, 8):
    for B, T in ((3, 7), (1, 1), (2, 2)):
      cases.append(_case("patch2", "l2", L2, B, T, H, 24, ("fwd", "fwd_pooled", "dgrad", "dgrad_pooled")))
  # layer 3, patch-resident (conv_patch16_kernel: 2 frames per workgroup): odd frame counts, single-frame clips
  for B, T in ((3, 7), (1, 1), (5, 1)):
    cases.append(_case("patch3", "l3", L3, B, T, 12, 12, ("fwd", "fwd_pooled", "dgrad", "dgrad_pooled")))
  # implicit GEMM (conv3d_igemm_kernel, 256 output pixels per workgroup): forward = (32, 64) / (64, 96), data gradient
  # = (64, 32) / (96, 64).  B2T4 at 10x10 = 800 pixels: four workgroups, the last one ragged; B1T1 at 6x6: 36 pixels
  for lname, layer in (("l2", L2), ("l3", L3)):
    for H, W in ((10, 10), (6, 6), (6, 10)):
      for B, T in ((2, 4), (1, 1)):
        cases.append(_case("igemm", lname, layer, B, T, H, W, ("fwd", "dgrad")))
  # transpose-read weight gradient (lr_conv_wgrad.hip: 3 x 85 workgroups, tiles of 2 frames x 6 or 4 rows): B2T45 = 90
  # frames gives a workgroup up to three tiles; 21 and 1 frames leave workgroups idle and end the batch inside a tile
  for lname, layer, W, Hs in (("l2", L2, 24, (24, 16)), ("l3", L3, 12, (12, 6))):
    for H in Hs:
      for B, T in ((3, 7), (1, 1), (1, 2), (2, 45)):
        cases.append(_case("tr2", lname, layer, B, T, H, W, ("wgrad", "wgrad_pooled")))
  # tap-stationary weight gradient (conv3d_wgrad_ts_kernel), one tile per workgroup: <32, 2, 7>, <64, 3, 5> and —
  # with 3x3x3 taps on layer 2's channels, which no layer of the frontend has — <32, 2, 3>
  for lname, layer, hws in (("l2", L2, ((10, 10), (6, 10))), ("l3", L3, ((6, 6), (4, 4))), ("l2k3", L2K3, ((6, 10),))):
    for H, W in hws:
      for B, T in ((2, 3), (1, 2)):
        cases.append(_case("ts", lname, layer, B, T, H, W, ("wgrad",)))
  # ... and its walk: 85 workgroups per temporal tap take row tiles slot, slot + 85, ...  49 frames of 14x10 (layer 2:
  # 12-row tiles) / 20x6 (layer 3: 16-row tiles) are 98 row tiles, every second one ragged (2 / 4 rows): workgroups
  # load a second tile while they contract the first, tiles start below row 0
  cases.append(_case("ts", "l2", L2, 7, 7, 14, 10, ("wgrad",)))
  cases.append(_case("ts", "l3", L3, 7, 7, 20, 6, ("wgrad",)))
  # split-pixel weight gradient (conv3d_wgrad_kernel): reached only where no tile of the tap-stationary kernel fits —
  # a 72-wide (layer 2: <32, 2, 4>) or 56-wide (layer 3: <64, 3, 2>) input, two rows high to keep it tiny
  for lname, layer, W in (("l2", L2, 72), ("l3", L3, 56)):
    # B7T7: 49 frames = 7056 / 5488 pixels over at most 53 / 37 pixel ranges (wgrad_splits) of whole 128-pixel stages:
    # 256 pixels, two stages, per workgroup; the smaller cases are one stage
    for B, T in ((2, 3), (1, 2), (7, 7)):
      cases.append(_case("split", lname, layer, B, T, 2, W, ("wgrad",)))
  return cases


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases(group, op=None):
  return [c for c in CASES if c.group == group and (op is None or op in c.ops)]


# pool-only kernels: (C, frames, H, W)
POOL_CASES = [(C, frames, H, W) for C in (32, 64, 96) for frames, H, W in ((1, 6, 10), (5, 12, 12))]


def pool_problem(C, frames, H, W):
  """(act [1][frames][H][W][C] from {-2..3}, dP [1][frames][H/2][W/2][C] from {-1, 0, 1})"""
  g = generator("pool-C%d-F%d-%dx%d" % (C, frames, H, W))
  return pool_values((1, frames, H, W, C), g), ternary((1, frames, H // 2, W // 2, C), g)


# clip conversion: (frames, H, W)
CLIP_CASES = [(3, 19, 21), (2, 32, 32), (1, 5, 7)]


class Problem:
  """The operands of one case and, computed on first use, the fp64 reference of every operation on them."""

  def __init__(self, case):
    self.case = case
    L, g = case.layer, generator(case.name)
    B, T, H, W = case.B, case.T, case.H, case.W
    self.ho, self.wo = out_hw(L, H, W)
    if L.cin == 3:
      self.clip = clip_bytes(B, T, H, W, g)
      self.x = clip_to_ndhwc(self.clip)
    else:
      self.x = ternary((B, T, H, W, L.cin), g)
    self.w = weights(L, g, case.keep)
    self.bias = biases(L.cout, g)
    self.dz = ternary((B, T, self.ho, self.wo, L.cout), g)
    if self.ho % 2 == 0 and self.wo % 2 == 0:
      self.dP = ternary((B, T, self.ho // 2, self.wo // 2, L.cout), g)

  def _conv(self, x, w):
    return conv_forward(x, w, None, False, self.case.layer.stride, self.case.layer.pad)

  def _dgrad(self, dz, w):
    return conv_dgrad(dz, w, self.x.shape, self.case.layer.stride, self.case.layer.pad)

  def _wgrad(self, x, dz):
    return conv_wgrad(x, dz, self.w.shape, self.case.layer.stride, self.case.layer.pad)

  @functools.cached_property
  def z(self):   # pre-activation without the bias
    return self._conv(self.x, self.w)

  def y(self, bias, relu):
    y = self.z + self.bias if bias else self.z
    return y.clamp_min(0) if relu else y

  @functools.cached_property
  def pooled_code(self):
    return relu_pool(self.z + self.bias)

  @functools.cached_property
  def code(self):
    """The window codes the backward kernels read: the forward's where the case runs the pooled forward, else drawn
    uniformly from 0..4 (the kernels that un-pool route by the code alone, so any code is a valid input)."""
    if "fwd_pooled" in self.case.ops:
      return self.pooled_code[1]
    return torch.randint(0, 5, tuple(self.dP.shape), generator=generator(self.case.name + "/code")).to(torch.uint8)

  @functools.cached_property
  def dz_unpooled(self):
    return unpool_from_code(self.code, self.dP)

  @functools.cached_property
  def dx(self):
    return self._dgrad(self.dz, self.w)

  @functools.cached_property
  def dx_pooled(self):
    return self._dgrad(self.dz_unpooled, self.w)

  @functools.cached_property
  def dw(self):
    return self._wgrad(self.x, self.dz)

  @functools.cached_property
  def dw_pooled(self):
    return self._wgrad(self.x, self.dz_unpooled)

  def expected(self, op):
    """{name: (tensor, 'bf16' | 'f32' | 'u8')}: everything the kernels of `op` write."""
    if op == "fwd":
      return {"y": (self.y(False, False), "bf16"), "y+bias": (self.y(True, False), "bf16"),
              "relu(y)": (self.y(False, True), "bf16"), "relu(y+bias)": (self.y(True, True), "bf16")}
    if op == "fwd_pooled":
      return {"pooled": (self.pooled_code[0], "bf16"), "code": (self.pooled_code[1], "u8")}
    if op == "dgrad":
      return {"dx": (self.dx, "bf16")}
    if op == "dgrad_pooled":
      return {"dx": (self.dx_pooled, "bf16")}
    if op == "wgrad":
      return {"dw": (self.dw, "f32"), "dbias": (bias_grad(self.dz), "f32")}
    if op == "wgrad_pooled":
      return {"dw": (self.dw_pooled, "f32"), "dbias": (bias_grad(self.dz_unpooled), "f32")}
    raise KeyError(op)


@functools.lru_cache(maxsize=2)
def problem(name):
  return Problem(BY_NAME[name])
