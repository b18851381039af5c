"""The seeded cases of tests/test_gpu_head_fp64.py (the output head of lr_proj.hip through lr_proj_logsoftmax_forward /
_backward, the three products it hands to lr_sgemm, and the token loss of lr_misc.hip through lr_nll_mean_forward /
lr_nll_forward3 / lr_nll_mean_backward), what float64 and float32 torch say about them on the CPU, and the helpers that
call the C ABI.  Shared with tests/test_head_cases_cpu.py, which checks on the CPU that the tables are what they claim to
be.  Importable without a GPU; nothing here looks at a device result.

The references are the float64 formula of the same operation on the kernel's own float32 inputs:
  forward   log_softmax(hidden W^T + bias + log(mask + 2^-149)); 1e-45f is the smallest fp32 subnormal, 2^-149, and its
            log is -103.27892990343184, so masked classes stay finite
  backward  the float32 log_probs it is given are DATA: dlogits = g - exp(lp) . sum_c g, dhidden = dlogits W,
            dW = dlogits^T hidden, dbias = sum_r dlogits
  loss      sum over the non-PAD rows of -lp[r, label_r] / their count, and d_lp[r, label_r] = -g / count
and the float32 CPU restatement whose error sets the bound is the same formula, left to right, in float32 torch.

The shapes are the smallest at which each dispatch branch can still go wrong, not the workload's: every case says which
kernels it must reach (`path`), plan() recomputes that from the dispatch rules of lr_proj.hip and lr_misc.hip, and every
case carries the reason it is in the table."""
import collections
import functools
import math
import zlib

import torch

ULP = 2.0 ** -23
TINY = 2.0 ** -149                    # 1e-45f
LOG_TINY = -103.27892990343184        # log(2^-149)
GUARD = 64                            # NaN floats behind every output
MAX_CLASSES = 256                     # kMaxClasses of lr_proj.hip
FUSED_BWD_MAX_CLASSES = 128           # kPbMaxC

# ---- forward: (R, K, C, mask kind) --------------------------------------------------------------------------------------
# mask kinds: two = classes 1 and 2 masked (the shipped mask), none, all = every class masked (the whole row rides on
# -103.28), frac = values in (0, 1).  off_hidden / off_w: the operand starts that many floats past a 16-byte boundary.
# data: the case whose seeded inputs this one shares (the misaligned copies of a fused case).
Fwd = collections.namedtuple("Fwd", "name R K C mask off_hidden off_w saturated data path why")


def _f(name, R, K, C, mask, path, why, off_hidden=0, off_w=0, saturated=False, data=None):
  return Fwd(name, R, K, C, mask, off_hidden, off_w, saturated, data or name, path, why)


FWD_CASES = collections.OrderedDict((c.name, c) for c in [
    # fused kernel: steps = K / 16 around the pipeline's group of four, rows around the 16-row workgroup, classes around
    # the 16-class wave tiles
    _f("k16_r1_c1", 1, 16, 1, "none", "fused", "one step: the first group is all clamped tail; one row, one class, one wave"),
    _f("k48_r15_c15", 15, 48, 15, "two", "fused", "three steps: a ragged first group, no prefetch; a short row and class tile"),
    _f("k64_r16_c16", 16, 64, 16, "two", "fused", "four steps: exactly one group, every prefetch clamped; exact tiles"),
    _f("k80_r17_c17", 17, 80, 17, "two", "fused", "five steps: a group and a tail of one; one row and one class into the next tile"),
    _f("k144_r33_c65", 33, 144, 65, "two", "fused", "nine steps: two groups and a tail; three workgroups; the shipped C = 65"),
    _f("k512_r33_c128", 33, 512, 128, "frac", "fused", "32 steps, the shipped K; 8 waves; fractional mask values"),
    _f("k64_r17_c129", 17, 64, 129, "none", "fused", "nine waves, the last with one class"),
    _f("k16_r16_c255", 16, 16, 255, "two", "fused", "16 waves, the last one class short, at one step"),
    _f("k80_r33_c256", 33, 80, 256, "all", "fused", "16 full waves (1024 threads), the most the head takes; every class masked"),
    _f("k48_r17_c65_all", 17, 48, 65, "all", "fused", "every class masked at the shipped C: the row rides on -103.28"),
    _f("k64_r17_c65", 17, 64, 65, "two", "fused", "the data of the two misaligned copies below, through the fused kernel"),
    _f("k64_r17_c65_sat", 17, 64, 65, "two", "fused", "hidden x 30: one class ahead by > 100 nats, every other exp underflows",
       saturated=True),
    # fallback chain: mask_bias_kernel -> lr_sgemm_impl with the folded bias -> log_softmax_rows_kernel
    _f("k1_r5_c3", 5, 1, 3, "two", "fallback", "K = 1: a product of one term; only the unmasked class 0 survives"),
    _f("k7_r17_c17", 17, 7, 17, "none", "fallback", "K % 16 != 0 and K % 4 != 0: scalar operand loads"),
    _f("k40_r33_c65", 33, 40, 65, "two", "fallback", "K % 16 = 8: vector loads, one ragged k stage; the shipped C"),
    _f("k40_r5_c17_all", 5, 40, 17, "all", "fallback", "every class masked through the row kernel"),
    _f("k72_r16_c129", 16, 72, 129, "frac", "fallback", "three 64-class column tiles; lanes past C in the row kernel's third pass"),
    _f("k520_r50_c256", 50, 520, 256, "two", "fallback", "the largest case: split K, the row kernel's four full passes"),
    _f("k64_r17_c65_hidden_off", 17, 64, 65, "two", "fallback", "K % 16 == 0 but hidden one float past a 16-byte boundary",
       off_hidden=1, data="k64_r17_c65"),
    _f("k64_r17_c65_w_off", 17, 64, 65, "two", "fallback", "K % 16 == 0 but W one float past a 16-byte boundary",
       off_w=1, data="k64_r17_c65"),
])
# the same data through the fused kernel and through each misaligned copy
TWINS = [("k64_r17_c65", "k64_r17_c65_hidden_off"), ("k64_r17_c65", "k64_r17_c65_w_off")]
REFUSED = _f("c257", 4, 16, 257, "none", None, "C > 256: LR_ERR_UNSUPPORTED")

# ---- backward: (R, K, C) ------------------------------------------------------------------------------------------------
Bwd = collections.namedtuple("Bwd", "name R K C saturated path why")


def _b(name, R, K, C, path, why, saturated=False):
  return Bwd(name, R, K, C, saturated, path, why)


BWD_CASES = collections.OrderedDict((c.name, c) for c in [
    # fused: 16 rows x 64 k columns per workgroup, slab rows Cp = ceil(C / 8) . 8, 16-class tiles in LDS
    _b("r1_k1_c1", 1, 1, 1, "fused", "one row, one column, one class: every tile ragged; dlogits is exactly 0"),
    _b("r16_k63_c7", 16, 63, 7, "fused", "a full row block; one column short of a workgroup; Cp = 8 > C"),
    _b("r17_k64_c8", 17, 64, 8, "fused", "one row into the second slab; exactly one column workgroup; Cp = C"),
    _b("r50_k65_c9", 50, 65, 9, "fused", "four slabs (the reduce kernel's four thread rows, one each); one column into the "
       "second column workgroup; Cp = 16"),
    _b("r17_k200_c65", 17, 200, 65, "fused", "four column workgroups, the last of 8 columns; the shipped C: 5 class tiles"),
    _b("r50_k64_c128", 50, 64, 128, "fused", "the fused path's last C: LDS rows full, 8 class tiles"),
    _b("r1_k200_c9", 1, 200, 9, "fused", "one row against many columns: 15 zero rows in every MFMA"),
    _b("r16_k65_c128", 16, 65, 128, "fused", "one slab; the second column workgroup owns one column at C = 128"),
    _b("r17_k64_c65_sat", 17, 64, 65, "fused", "lp with one class at 0 and the rest below -100, g with a row sum near 200: "
       "g - exp(lp) . sum g cancels at the dominant class", saturated=True),
    # chain: log_softmax_bwd_rows_kernel -> two lr_sgemm_impl -> lr_colsum_partial -> colsum_final_kernel
    _b("r17_k64_c129", 17, 64, 129, "chain", "the first C past the fused path"),
    _b("r33_k63_c256", 33, 63, 256, "chain", "K % 4 != 0: scalar loads of W and hidden in both products; the last C"),
    _b("r50_k520_c256", 50, 520, 256, "chain", "the largest case"),
])

# ---- token loss: (B, L, V, label row stride, PAD pattern) -----------------------------------------------------------------
# pad: the ignore index (0, as data.py has it; -1 at V = 1, where 0 is the only class).  pattern: none / tail (PAD behind a
# ragged length) / rows (tail, and every third row all PAD) / all (every position).
Nll = collections.namedtuple("Nll", "name B L V stride pad pattern path why")


def _n(name, B, L, V, stride, pattern, path, why):
  return Nll(name, B, L, V, stride, 0 if V > 1 else -1, pattern, path, why)


NLL_CASES = collections.OrderedDict((c.name, c) for c in [
    _n("n1_v1", 1, 1, 1, 4, "none", "scalar", "one row, one class"),
    _n("n1023_v3", 33, 31, 3, 40, "tail", "scalar", "one row short of one row per thread"),
    _n("n1024_v4", 32, 32, 4, 33, "tail", "vec4", "exactly one row per thread of the forward; the smallest vector V"),
    _n("n1025_v65", 41, 25, 65, 26, "rows", "scalar", "thread 0 takes a second row; the shipped V; whole rows of PAD"),
    _n("n1025_v4", 5, 205, 4, 300, "tail", "vec4", "thread 0 takes a second row through the vector kernel"),
    _n("n3000_v68", 100, 30, 68, 37, "rows", "vec4", "three rows per thread, then the tree; V % 4 == 0 past 64"),
    _n("n3000_v3", 3, 1000, 3, 1001, "tail", "scalar", "three rows per thread over long label rows"),
    _n("all_pad_v68", 4, 8, 68, 9, "all", "vec4", "no label counts: count 0, the loss 0 / 0"),
    _n("all_pad_v3", 3, 5, 3, 8, "all", "scalar", "no label counts, through the scalar kernel"),
    # (not in the issue's list: past 1024 workgroups of 256 threads the backward kernels walk the tensor in grid strides)
    _n("n4100_v65", 41, 100, 65, 101, "tail", "scalar", "R . V > 1024 . 256: the scalar kernel's second grid stride"),
    _n("n15500_v68", 155, 100, 68, 128, "rows", "vec4", "R . V / 4 > 1024 . 256: the vector kernel's second grid stride"),
])
NLL_G = 0.7    # the upstream gradient of the loss


def plan(case, offset=0):
  """The dispatch rule, restated: which kernels a case must reach.  Forward (lr_proj_logsoftmax_forward): `fused` when
  K % 16 == 0 and hidden and W are 16-byte aligned, else `fallback`.  Backward: `fused` when C <= 128, else `chain`.
  Token-loss backward (lr_nll_mean_backward): `vec4` when V % 4 == 0 and d_log_probs is 16-byte aligned (offset: floats
  past such a boundary), else `scalar`."""
  if isinstance(case, Fwd):
    return "fused" if case.K % 16 == 0 and case.off_hidden % 4 == 0 and case.off_w % 4 == 0 else "fallback"
  if isinstance(case, Bwd):
    return "fused" if case.C <= FUSED_BWD_MAX_CLASSES else "chain"
  if isinstance(case, Nll):
    return "vec4" if case.V % 4 == 0 and offset % 4 == 0 else "scalar"
  raise TypeError(case)


def figures(got, want64):
  """Largest element-wise error relative to the float64 tensor's largest entry."""
  scale = max(float(want64.abs().max()), 1e-30)
  return float((got.double() - want64).abs().max()) / scale


def bound(cpu_err):
  """The project's rule (hold() of tests/test_gpu_transformer_fp64.py): 4 x the float32 CPU formula's error, never less
  than 4 ulp."""
  return 4 * max(cpu_err, ULP)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------

HeadInputs = collections.namedtuple("HeadInputs", "hidden W bias mask g prior_dW prior_db")
SAT_CLASS = 3      # the class a saturated case lets dominate (not one of the two masked ones)


@functools.lru_cache(maxsize=None)
def _draw(seed, R, K, C, kind, saturated):
  gen = torch.Generator().manual_seed(zlib.crc32(seed.encode()))
  hidden = torch.randn(R, K, generator=gen)
  W = torch.randn(C, K, generator=gen) / math.sqrt(K)
  bias = torch.randn(C, generator=gen)
  frac = torch.rand(C, generator=gen) * 0.98 + 0.01
  g = torch.randn(R, C, generator=gen)
  prior_dW = torch.randn(C, K, generator=gen)
  prior_db = torch.randn(C, generator=gen)
  mask = torch.ones(C)
  if kind == "two":
    mask[1:3] = 0
  elif kind == "all":
    mask.zero_()
  elif kind == "frac":
    mask = frac
  else:
    assert kind == "none"
  if saturated:
    # hidden x 30 around a common direction s that W[SAT_CLASS] points along: that class's logit is 30 . 4 . sqrt(K) = 960
    # at K = 64, give or take 30, every other one 0 give or take 30 . sqrt(17) = 124
    s = torch.randint(0, 2, (K,), generator=gen).float() * 2 - 1
    hidden = 30 * (hidden + 4 * s)
    W[SAT_CLASS] = s / math.sqrt(K)
    g = g + 3      # a row sum near 3 C
  return HeadInputs(hidden, W, bias, mask, g, prior_dW, prior_db)


def fwd_inputs(case):
  return _draw(case.data, case.R, case.K, case.C, case.mask, case.saturated)


@functools.lru_cache(maxsize=None)
def _bwd_inputs(name):
  case = BWD_CASES[name]
  inp = _draw("bwd_" + name, case.R, case.K, case.C, "two" if case.C >= 3 else "none", case.saturated)
  return inp, forward_formula(inp.hidden, inp.W, inp.bias, inp.mask, torch.float32)


def bwd_inputs(case):
  """(hidden, W, g and the priors of accumulate = 1; the float32 log_probs the backward is given: the float32 CPU forward
  of the case under the shipped mask — no mask below three classes)."""
  return _bwd_inputs(case.name)


# ---- the formulas, in the dtype asked for -------------------------------------------------------------------------------

def forward_formula(hidden, W, bias, mask, dtype):
  h, w, b, m = (t.to(dtype) for t in (hidden, W, bias, mask))
  # float32: mask + 1e-45f, as the kernel has it (the CPU keeps subnormals too); float64: the same number, 2^-149
  term = torch.log(m + torch.tensor(TINY, dtype=dtype))
  return torch.log_softmax(h @ w.t() + b + term, dim=1)


def backward_formula(g, lp, hidden, W, dtype):
  g, lp, h, w = (t.to(dtype) for t in (g, lp, hidden, W))
  dlogits = g - torch.exp(lp) * g.sum(dim=1, keepdim=True)
  return {"dlogits": dlogits, "dhidden": dlogits @ w, "dW": dlogits.t() @ h, "dbias": dlogits.sum(dim=0)}


def autograd_formula(inp, dtype):
  """torch.autograd on the forward formula in `dtype` with inp.g as the upstream gradient, on copies of the inputs:
  {lp, dhidden, dW, dbias} — what encoder._ProjLogSoftmaxFunction returns, whose backward uses its OWN log_probs."""
  h, w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (inp.hidden, inp.W, inp.bias))
  term = torch.log(inp.mask.to(dtype) + torch.tensor(TINY, dtype=dtype))
  lp = torch.log_softmax(h @ w.t() + b + term, dim=1)
  lp.backward(inp.g.to(dtype))
  return {"lp": lp.detach(), "dhidden": h.grad, "dW": w.grad, "dbias": b.grad}


@functools.lru_cache(maxsize=None)
def fwd_reference(name):
  """(float64 truth, float32 CPU yardstick) of a forward case's log_probs: computed once, shared, never written to."""
  inp = fwd_inputs(FWD_CASES[name])
  return (forward_formula(inp.hidden, inp.W, inp.bias, inp.mask, torch.float64),
          forward_formula(inp.hidden, inp.W, inp.bias, inp.mask, torch.float32))


@functools.lru_cache(maxsize=None)
def bwd_reference(name):
  inp, lp = bwd_inputs(BWD_CASES[name])
  return (backward_formula(inp.g, lp, inp.hidden, inp.W, torch.float64),
          backward_formula(inp.g, lp, inp.hidden, inp.W, torch.float32))


BWD_KEYS = ("dlogits", "dhidden", "dW", "dbias")


def masked_columns(case):
  """bool [C]: the classes whose mask is 0 — their log_probs sit near -103 and are held on their own, so that they do not
  set the scale for the others."""
  return fwd_inputs(case).mask == 0


# ---- token loss ---------------------------------------------------------------------------------------------------------

NllInputs = collections.namedtuple("NllInputs", "lp wide labels")


@functools.lru_cache(maxsize=None)
def nll_inputs(name):
  """lp (B, L, V) float32; wide (B, stride) int64 whose columns 1 .. L are the labels (column 0 and the columns past L
  hold valid class ids that no kernel may read as labels); labels = wide[:, 1:1 + L], a view of row stride `stride` > L."""
  c = NLL_CASES[name]
  assert c.stride >= c.L + 1
  gen = torch.Generator().manual_seed(zlib.crc32(("nll_" + name).encode()))
  if c.V > 1:
    lp = torch.log_softmax(3 * torch.randn(c.B, c.L, c.V, generator=gen), dim=-1)
    lab = torch.randint(1, c.V, (c.B, c.L), generator=gen)
    junk = torch.randint(1, c.V, (c.B, c.stride), generator=gen)
  else:
    lp = -5 * torch.rand(c.B, c.L, c.V, generator=gen)
    lab = torch.zeros(c.B, c.L, dtype=torch.int64)
    junk = torch.zeros(c.B, c.stride, dtype=torch.int64)
  lens = torch.randint(1, c.L + 1, (c.B,), generator=gen)
  lens[c.B - 1] = c.L
  if c.B >= 2 and c.L >= 2:
    lens[0] = 1
  if c.pattern in ("tail", "rows"):
    lab[torch.arange(c.L).unsqueeze(0) >= lens.unsqueeze(1)] = c.pad
  if c.pattern == "rows":
    lab[1:-1:3] = c.pad      # the last row stays whole
  if c.pattern == "all":
    lab[:] = c.pad
  wide = junk.clone()
  wide[:, 1:1 + c.L] = lab
  return NllInputs(lp, wide, wide[:, 1:1 + c.L])


def nll_formula(lp, labels, pad, g, dtype):
  """{loss, count, sum, d_lp}: sum over the non-PAD rows of -lp[r, label_r], their count, the quotient, and the quotient's
  gradient times g."""
  lp = lp.to(dtype)
  on = labels != pad
  count = int(on.sum())
  picked = torch.gather(lp, 2, labels.clamp(min=0).unsqueeze(-1)).squeeze(-1)
  total = -(picked * on.to(dtype)).sum()
  cnt = torch.tensor(float(count), dtype=dtype)
  d_lp = torch.zeros_like(lp)
  d_lp.scatter_(2, labels.clamp(min=0).unsqueeze(-1), (-(torch.tensor(g, dtype=dtype) / cnt) * on.to(dtype)).unsqueeze(-1))
  return {"loss": total / cnt, "count": count, "sum": total, "d_lp": d_lp}


@functools.lru_cache(maxsize=None)
def nll_reference(name):
  c, inp = NLL_CASES[name], nll_inputs(name)
  g = float(torch.tensor(NLL_G, dtype=torch.float32))      # the float32 value the kernel is handed
  return nll_formula(inp.lp, inp.labels, c.pad, g, torch.float64), nll_formula(inp.lp, inp.labels, c.pad, g, torch.float32)


# ---- the products the head hands to lr_sgemm ------------------------------------------------------------------------------
# (transA, transB, M, N, K, bias, beta): NT with the folded bias at the fallback forward's shapes (R x C x K), NN (dhidden,
# R x K x C) and TN with beta = 1 (dW, C x K x R) at the chain's
def gemm_shapes():
  out = []
  for c in FWD_CASES.values():
    if c.path == "fallback" and c.data == c.name:
      out.append(("nt_bias_%dx%dx%d" % (c.R, c.C, c.K), 0, 1, c.R, c.C, c.K, True, 0.0))
  for c in BWD_CASES.values():
    if c.path == "chain":
      out.append(("nn_%dx%dx%d" % (c.R, c.K, c.C), 0, 0, c.R, c.K, c.C, False, 0.0))
      out.append(("tn_beta1_%dx%dx%d" % (c.C, c.K, c.R), 1, 0, c.C, c.K, c.R, False, 1.0))
  return out


# (leading-dimension padding, floats the base pointers sit past a 16-byte boundary): a padding of 4 keeps 16-byte loads
# wherever the tight layout has them; 5 with the bases one float off takes every scalar branch
GEMM_LAYOUTS = [(4, 0), (5, 1)]


@functools.lru_cache(maxsize=None)
def gemm_inputs(name):
  _, ta, tb, M, N, K, bias, beta = [s for s in gemm_shapes() if s[0] == name][0]
  gen = torch.Generator().manual_seed(zlib.crc32(("gemm_" + name).encode()))
  A = torch.randn((K, M) if ta else (M, K), generator=gen)
  B = torch.randn((N, K) if tb else (K, N), generator=gen) / math.sqrt(K)
  bv = torch.randn(N, generator=gen) if bias else None
  C0 = torch.randn(M, N, generator=gen) if beta else None
  return A, B, bv, C0


def gemm_formula(name, dtype):
  _, ta, tb, M, N, K, bias, beta = [s for s in gemm_shapes() if s[0] == name][0]
  A, B, bv, C0 = gemm_inputs(name)
  A, B = A.to(dtype), B.to(dtype)
  out = (A.t() if ta else A) @ (B.t() if tb else B)
  if bv is not None:
    out = out + bv.to(dtype)
  if C0 is not None:
    out = out + beta * C0.to(dtype)
  return out


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

def place(t, dev, offset=0):
  """t's values in a device buffer of their own, `offset` floats past a 16-byte boundary."""
  buf = torch.full((t.numel() + offset + 4,), float("nan"), dtype=torch.float32, device=dev)
  assert buf.data_ptr() % 16 == 0
  view = buf[offset:offset + t.numel()].view(t.shape)
  view.copy_(t)
  assert view.data_ptr() % 16 == 4 * (offset % 4)
  return view


def place2d(t, dev, pad, offset):
  """A (rows, cols) matrix in a device buffer with leading dimension cols + pad, `offset` floats past a 16-byte boundary;
  the padding, and GUARD floats behind the last row, hold NaN.  (buffer, the (rows, cols + pad) view, cols + pad)."""
  rows, cols = t.shape
  ld = cols + pad
  buf = torch.full((rows * ld + offset + GUARD,), float("nan"), dtype=torch.float32, device=dev)
  assert buf.data_ptr() % 16 == 0
  full = buf[offset:offset + rows * ld].view(rows, ld)
  full[:, :cols].copy_(t)
  return buf, full, ld


def poisoned(n, dev):
  """n floats of NaN and GUARD more behind them."""
  return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev)


def workspace(nbytes, dev):
  return torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device=dev)


def run_forward(case, dev, short=0):
  """lr_proj_logsoftmax_forward on a case: (status, log_probs (R, C) on the CPU, the GUARD floats behind them).  The
  output and its guard band start as NaN, the workspace as 0xFF bytes.  short: bytes kept back from workspace_bytes."""
  from lipreading_amd import _C
  L = _C.lib()
  inp = fwd_inputs(case)
  R, K, C = case.R, case.K, case.C
  hidden, W = place(inp.hidden, dev, case.off_hidden), place(inp.W, dev, case.off_w)
  bias, mask = inp.bias.to(dev), inp.mask.to(dev)
  out = poisoned(R * C, dev)
  wbytes = L.lr_proj_workspace_bytes(R, K, C)
  ws = workspace(wbytes, dev)
  status = L.lr_proj_logsoftmax_forward(hidden.data_ptr(), W.data_ptr(), bias.data_ptr(), mask.data_ptr(), out.data_ptr(),
                                        ws.data_ptr(), wbytes - short, R, K, C, _C.stream_handle())
  torch.cuda.synchronize()
  out = out.cpu()
  return status, out[:R * C].view(R, C), out[R * C:]


def run_backward(case, dev, null_dhidden=False, accumulate=False):
  """lr_proj_logsoftmax_backward on a case: every output on the CPU under BWD_KEYS (no dhidden when it was NULL), and
  "guards": the GUARD floats behind each.  dlogits and dhidden start as NaN, the workspace as 0xFF bytes; dW and dbias
  start as NaN (accumulate = 0) or as the case's priors (accumulate = 1)."""
  from lipreading_amd import _C
  L = _C.lib()
  inp, lp = bwd_inputs(case)
  R, K, C = case.R, case.K, case.C
  g, lpd, hidden, W = inp.g.to(dev), lp.to(dev), inp.hidden.to(dev), inp.W.to(dev)
  bufs = {"dlogits": poisoned(R * C, dev), "dW": poisoned(C * K, dev), "dbias": poisoned(C, dev)}
  if not null_dhidden:
    bufs["dhidden"] = poisoned(R * K, dev)
  if accumulate:
    bufs["dW"][:C * K].copy_(inp.prior_dW.reshape(-1))
    bufs["dbias"][:C].copy_(inp.prior_db)
  wbytes = L.lr_proj_workspace_bytes(R, K, C)
  ws = workspace(wbytes, dev)
  _C.check(L.lr_proj_logsoftmax_backward(g.data_ptr(), lpd.data_ptr(), hidden.data_ptr(), W.data_ptr(),
                                         bufs["dlogits"].data_ptr(), _C.ptr(bufs.get("dhidden")), bufs["dW"].data_ptr(),
                                         bufs["dbias"].data_ptr(), ws.data_ptr(), wbytes, 1 if accumulate else 0, R, K, C,
                                         _C.stream_handle()), "lr_proj_logsoftmax_backward")
  torch.cuda.synchronize()
  shapes = {"dlogits": (R, C), "dhidden": (R, K), "dW": (C, K), "dbias": (C,)}
  out, guards = {}, {}
  for k, buf in bufs.items():
    buf = buf.cpu()
    n = buf.numel() - GUARD
    out[k], guards[k] = buf[:n].view(shapes[k]), buf[n:]
  out["guards"] = guards
  return out


def run_gemm(name, dev, pad, offset, ws_factor):
  """lr_sgemm on a product of gemm_shapes(): (C (M, N) on the CPU, its padding columns, the floats behind it, the
  workspace size lr_sgemm_workspace_bytes gave).  Operands and C have leading dimensions `pad` past tight, with NaN in the
  padding, and start `offset` floats past a 16-byte boundary; C starts as NaN (beta = 0) or as the seeded C0; the
  workspace is ws_factor x the size asked for, 0xFF-filled."""
  from lipreading_amd import _C
  L = _C.lib()
  _, ta, tb, M, N, K, bias, beta = [s for s in gemm_shapes() if s[0] == name][0]
  A, B, bv, C0 = gemm_inputs(name)
  _, Ad, lda = place2d(A, dev, pad, offset)
  _, Bd, ldb = place2d(B, dev, pad, offset)
  start = C0 if C0 is not None else torch.full((M, N), float("nan"))
  Cbuf, Cd, ldc = place2d(start, dev, pad, offset)
  bd = place(bv, dev, offset) if bv is not None else None
  wbytes = L.lr_sgemm_workspace_bytes(M, N, K)
  ws = workspace(ws_factor * wbytes, dev)
  _C.check(L.lr_sgemm(ta, tb, M, N, K, 1.0, Ad.data_ptr(), lda, Bd.data_ptr(), ldb, beta, Cd.data_ptr(), ldc, _C.ptr(bd),
                      0, 0, ws.data_ptr() if wbytes else None, ws_factor * wbytes, _C.stream_handle()), "lr_sgemm")
  torch.cuda.synchronize()
  full = Cd.cpu()
  return full[:, :N], full[:, N:], Cbuf[offset + M * ldc:].cpu(), wbytes


def _labels_on(name, dev):
  """The case's wide label tensor on the device and the view the product passes: wide[:, 1:], whose first L columns are
  the labels and whose row stride is the case's."""
  wide = nll_inputs(name).wide.to(dev)
  return wide, wide[:, 1:]


def run_nll_forward(name, dev, three):
  """lr_nll_mean_forward (out[0] = loss, out[1] = count) or lr_nll_forward3 (out[2] = the sum): (out on the CPU, the
  floats behind it)."""
  from lipreading_amd import _C
  L = _C.lib()
  c, inp = NLL_CASES[name], nll_inputs(name)
  lp = inp.lp.to(dev)
  wide, labels = _labels_on(name, dev)
  n = 3 if three else 2
  out = poisoned(n, dev)
  fn = L.lr_nll_forward3 if three else L.lr_nll_mean_forward
  _C.check(fn(lp.data_ptr(), labels.data_ptr(), labels.stride(0), c.L, c.pad, out.data_ptr(), c.B * c.L, c.V,
              _C.stream_handle()), "lr_nll_forward")
  torch.cuda.synchronize()
  out = out.cpu()
  return out[:n], out[n:]


def run_nll_backward(name, dev, offset=0):
  """lr_nll_mean_forward, then lr_nll_mean_backward with g = NLL_G into a NaN-filled d_log_probs that starts `offset`
  floats past a 16-byte boundary: (d_log_probs (B, L, V) on the CPU, the floats behind it)."""
  from lipreading_amd import _C
  L = _C.lib()
  c, inp = NLL_CASES[name], nll_inputs(name)
  lp = inp.lp.to(dev)
  wide, labels = _labels_on(name, dev)
  out2 = poisoned(2, dev)
  _C.check(L.lr_nll_mean_forward(lp.data_ptr(), labels.data_ptr(), labels.stride(0), c.L, c.pad, out2.data_ptr(),
                                 c.B * c.L, c.V, _C.stream_handle()), "lr_nll_mean_forward")
  g = torch.tensor([NLL_G], dtype=torch.float32, device=dev)
  n = c.B * c.L * c.V
  buf = poisoned(n + 4, dev)
  assert buf.data_ptr() % 16 == 0
  d_lp = buf[offset:offset + n]
  _C.check(L.lr_nll_mean_backward(labels.data_ptr(), labels.stride(0), c.L, c.pad, out2.data_ptr(), g.data_ptr(),
                                  d_lp.data_ptr(), c.B * c.L, c.V, _C.stream_handle()), "lr_nll_mean_backward")
  torch.cuda.synchronize()
  buf = buf.cpu()
  return buf[offset:offset + n].view(c.B, c.L, c.V), buf[offset + n:]
