"""The seeded cases of tests/test_gpu_rnn_fp64.py (one recurrent layer through lr_rnn_layer_forward / _backward), what
torch.nn.GRU / LSTM / RNN say about them in float64 and in float32, and the one helper that calls the C ABI.  Shared with
tests/test_rnn_layer_cases_cpu.py, which checks on the CPU that the table is what it claims to be.  Importable without a GPU;
nothing here looks at a device result.

The reference is the semantics include/lipreading_hip.h cites: pack_padded_sequence(enforce_sorted=False) -> nn.GRU /
LSTM / RNN(tanh), batch_first -> pad_packed_sequence(total_length=T); loss = (y . dy) + (h_n . dh_n) [+ (c_n . dc_n)]
with seeded dy, dh_n, dc_n, so autograd's gradients are what lr_rnn_layer_backward returns for those three inputs.

The shapes are the smallest at which each dispatch branch of lr_rnn_layer_forward / rnn_layer_backward_impl can still go
wrong, not the workload's: every case says which branch it expects (`proj`, `wgrad`, `recur`), and the CPU test recomputes
that from the arithmetic of lr_rnn.hip and lr_rnn_cluster.hip."""
import collections
import ctypes
import functools
import zlib

import torch

ULP = 2.0 ** -23
GATES = {"GRU": 3, "LSTM": 4, "RNN": 1}
SPLIT, X3, EXACT = "RECUR_SPLIT", "PROJ_BF16X3", "INPUT_BF16_EXACT"

# name cell B T I H D | flags | w_ih[1] - w_ih[0] modulo 4 floats | bias_ih[0::4] += 60, [1::4] -= 60 |
# proj:  the input projection's branch: fgemm_f32 / fgemm_x3 (lr_fgemm, I % 4 == 0, or PROJ_BF16X3 on an fp32 input),
#        xproj (lr_xproj_forward: PROJ_BF16X3 | INPUT_BF16_EXACT), sgemm_batched (I % 4 != 0, D = 2, W_ih a multiple of 4
#        floats apart), sgemm_each (I % 4 != 0 and D = 1 or W_ih[1] off by one float)
# wgrad: grouped (lr_sgemm_grouped_tn_impl, exact fp32) / fgemm_splitk (RECUR_SPLIT: weight_half with a K split) /
#        fgemm (PROJ_BF16X3: weight_half, one K range)
# recur: step / cluster32:<members> / cluster16:<members> / grid
Case = collections.namedtuple("Case", "name cell B T I H D flags offset saturated proj wgrad recur")


def _c(name, cell, B, T, I, H, D, proj, wgrad, recur, flags=(), offset=0, saturated=False):
  return Case(name, cell, B, T, I, H, D, tuple(flags), offset, saturated, proj, wgrad, recur)


CASES = collections.OrderedDict((c.name, c) for c in [
    # ---- step kernels (no mode flags): exact fp32 throughout ----
    _c("gru36_odd_i", "GRU", 5, 7, 51, 36, 2, "sgemm_batched", "grouped", "step"),
    _c("lstm20_uni_odd_i", "LSTM", 3, 6, 7, 20, 1, "sgemm_each", "grouped", "step"),
    _c("lstm20_w_ih_off_by_one", "LSTM", 5, 6, 51, 20, 2, "sgemm_each", "grouped", "step", offset=1),
    # (not in the issue's list: the same misplaced W_ih[1] with I % 4 == 0, where the projection is lr_fgemm's and has to
    # fall back from 16-byte loads for that operand alone)
    _c("lstm20_w_ih_off_by_one_i52", "LSTM", 5, 6, 52, 20, 2, "fgemm_f32", "grouped", "step", offset=1),
    _c("rnn12", "RNN", 4, 5, 8, 12, 2, "fgemm_f32", "grouped", "step"),
    _c("gru4_one_frame", "GRU", 1, 1, 3, 4, 1, "sgemm_each", "grouped", "step"),
    _c("lstm20_b17", "LSTM", 17, 9, 51, 20, 2, "sgemm_batched", "grouped", "step"),   # B and H cross the 16 x 16 tile
    _c("gru256_b17", "GRU", 17, 12, 204, 256, 2, "fgemm_f32", "grouped", "step"),
    # ---- one-launch recurrence ----
    _c("split_gru40", "GRU", 9, 6, 51, 40, 2, "sgemm_batched", "fgemm_splitk", "cluster32:2", [SPLIT]),
    # (not in the issue's list: B * T = 528 rows, the smallest at which wgrad_fgemm_plan really cuts K — in two — with I odd;
    # five groups of 8 samples, the last of one sample)
    _c("split_gru40_k_split", "GRU", 33, 16, 51, 40, 2, "sgemm_batched", "fgemm_splitk", "cluster32:2", [SPLIT]),
    _c("split_lstm36_uni", "LSTM", 3, 5, 7, 36, 1, "sgemm_each", "fgemm_splitk", "cluster32:2", [SPLIT]),
    _c("split_lstm768", "LSTM", 9, 12, 64, 768, 2, "fgemm_x3", "fgemm_splitk", "cluster32:24", [SPLIT]),
    _c("split_lstm800_uni", "LSTM", 4, 4, 12, 800, 1, "fgemm_x3", "fgemm_splitk", "cluster16:50", [SPLIT]),
    _c("split_gru896_uni", "GRU", 5, 4, 12, 896, 1, "fgemm_x3", "fgemm_splitk", "cluster16:56", [SPLIT]),
    _c("grid_lstm1156", "LSTM", 3, 3, 8, 1156, 2, "fgemm_x3", "fgemm_splitk", "grid", [SPLIT]),
    _c("grid_lstm1400_uni", "LSTM", 9, 3, 8, 1400, 1, "fgemm_x3", "fgemm_splitk", "grid", [SPLIT]),
    # ---- input-projection flags, with and without the one-launch recurrence ----
    _c("x3_step", "GRU", 5, 6, 24, 40, 2, "fgemm_x3", "fgemm", "step", [X3]),
    _c("x3_split", "GRU", 5, 6, 24, 40, 2, "fgemm_x3", "fgemm", "cluster32:2", [X3, SPLIT]),
    _c("x3exact_step", "GRU", 5, 6, 24, 40, 2, "xproj", "fgemm", "step", [X3, EXACT]),
    _c("x3exact_split", "GRU", 5, 6, 24, 40, 2, "xproj", "fgemm", "cluster32:2", [X3, EXACT, SPLIT]),
    # ---- saturated gates: pre-activations past +-44, where exp2 overflows and rcp sees inf ----
    _c("sat_gru_step", "GRU", 5, 6, 12, 40, 2, "fgemm_f32", "grouped", "step", saturated=True),
    _c("sat_lstm_step", "LSTM", 5, 6, 12, 40, 2, "fgemm_f32", "grouped", "step", saturated=True),
    _c("sat_rnn_step", "RNN", 5, 6, 12, 40, 2, "fgemm_f32", "grouped", "step", saturated=True),
    _c("sat_gru_split", "GRU", 5, 6, 12, 40, 2, "fgemm_f32", "fgemm_splitk", "cluster32:2", [SPLIT], saturated=True),
    _c("sat_lstm_split", "LSTM", 5, 6, 12, 40, 2, "fgemm_f32", "fgemm_splitk", "cluster32:2", [SPLIT], saturated=True),
])
PARTS_CASES = [n for n, c in CASES.items() if X3 in c.flags]
# where the bit-exact properties run: one step-path case, the two split-path ones the issue names, and the grid case
PROPERTY_CASES = ["gru36_odd_i", "split_gru40", "split_lstm768"]
GRID_CASE = "grid_lstm1156"
LSTM_STEP_CASE = "lstm20_b17"


def exact(case):
  """Every product of the case is exact fp32: held to hold()'s rule alone."""
  return not case.flags


def allowance(case, name):
  """(element-wise, relative norm) figures ADDED to the exact bound 4 x max(cpu fp32 error, 1 ulp) where the case leaves
  exact fp32 — the project's own figures for these paths, now against float64 instead of the step kernels: 1e-4 of the
  largest entry and 2e-5 in relative norm (test_split_recurrence_is_fp32_faithful,
  test_bf16x3_input_projection_tracks_the_fp32_path); dx of a bf16-exact input is contracted from the hi planes alone
  (bf16-level: 1e-2, element-wise and in norm).  (0, None) on the exact path: no norm check, nothing added."""
  if exact(case):
    return 0.0, None
  if name == "dx" and EXACT in case.flags:
    return 1e-2, 1e-2
  return 1e-4, 2e-5


def bounds(case, name, cpu_err):
  """(element-wise bound relative to the float64 tensor's largest entry, bound on the relative norm or None)."""
  base = 4 * max(cpu_err, ULP)
  elem, norm = allowance(case, name)
  return base + elem, None if norm is None else base + norm


def tensor_names(case):
  names = ["y", "h_n"] + (["c_n"] if case.cell == "LSTM" else []) + ["dx"]
  for d in range(case.D):
    names += ["dw_ih%d" % d, "dw_hh%d" % d, "db_ih%d" % d, "db_hh%d" % d]
  return names


Inputs = collections.namedtuple("Inputs", "x lens w_ih w_hh b_ih b_hh dy dh_n dc_n prefill garbage")


@functools.lru_cache(maxsize=None)
def inputs(name):
  """Seeded float32 inputs of a case (CPU).  lens: ragged, the last sample full (so it sits in the last tile of 16 / the
  last group of 8), sample 1 a single frame wherever B >= 3.  prefill: what accumulate = 1 adds to; garbage: values of
  magnitude 1e3 for the frames of x past each length."""
  c = CASES[name]
  g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
  GH = GATES[c.cell] * c.H
  x = torch.randn(c.B, c.T, c.I, generator=g)
  if EXACT in c.flags:
    x = x.to(torch.bfloat16).float()
  lens = torch.randint(1, max(c.T, 2), (c.B,), generator=g).clamp_(max=c.T)   # 1 .. T - 1: never the full length
  lens[c.B - 1] = c.T
  if c.B >= 3:
    lens[1] = 1
  k = c.H ** -0.5
  uni = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1) * k
  w_ih = [uni(GH, c.I) for _ in range(c.D)]
  w_hh = [uni(GH, c.H) for _ in range(c.D)]
  b_ih = [uni(GH) for _ in range(c.D)]
  b_hh = [uni(GH) for _ in range(c.D)]
  if c.saturated:
    for b in b_ih:
      b[0::4] += 60.0
      b[1::4] -= 60.0
  dy = torch.randn(c.B, c.T, c.D * c.H, generator=g)
  dh_n = torch.randn(c.D, c.B, c.H, generator=g)
  dc_n = torch.randn(c.D, c.B, c.H, generator=g)
  prefill = {}
  for d in range(c.D):
    for key, shape in (("dw_ih", (GH, c.I)), ("dw_hh", (GH, c.H)), ("db_ih", (GH,)), ("db_hh", (GH,))):
      prefill["%s%d" % (key, d)] = torch.randn(*shape, generator=g)
  sign = torch.randint(0, 2, (c.B, c.T, c.I), generator=g).float() * 2 - 1
  garbage = sign * (1e3 + 1e3 * torch.rand(c.B, c.T, c.I, generator=g))
  return Inputs(x, lens, w_ih, w_hh, b_ih, b_hh, dy, dh_n, dc_n, prefill, garbage)


def valid_mask(name):
  """[B, T, 1] bool: frame t of sample b exists."""
  c, inp = CASES[name], inputs(name)
  return (torch.arange(c.T).unsqueeze(0) < inp.lens.unsqueeze(1)).unsqueeze(-1)


def x_with_garbage(name):
  inp = inputs(name)
  return torch.where(valid_mask(name), inp.x, inp.garbage)


WRONG = ("swap_gates", "reverse_from_end", "drop_b_hn")


def applies(wrong, case):
  """Which deliberately wrong references can differ from the right one on a case."""
  if wrong == "swap_gates":
    return case.cell != "RNN"
  if wrong == "reverse_from_end":
    return case.D == 2 and case.B >= 2 and case.T >= 2
  if wrong == "drop_b_hn":
    return case.cell == "GRU"
  raise KeyError(wrong)


def evaluate(name, dtype, wrong=None):
  """torch.nn's layer on the case in `dtype` on the CPU: every tensor of tensor_names(case).  wrong: one of WRONG, a
  reference that is deliberately NOT the layer — gate blocks 0 and 1 swapped; the reverse direction run over the padded
  sequence from T - 1 instead of from lens - 1; b_hn taken out of r . (W_hn h + b_hn)."""
  c, inp = CASES[name], inputs(name)
  H = c.H
  cls = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM, "RNN": torch.nn.RNN}[c.cell]
  with torch.random.fork_rng():
    m = cls(c.I, H, num_layers=1, batch_first=True, bidirectional=c.D == 2).to(dtype)
  with torch.no_grad():
    for d in range(c.D):
      sfx = "_l0" + ("_reverse" if d else "")
      for key, src in (("weight_ih", inp.w_ih), ("weight_hh", inp.w_hh), ("bias_ih", inp.b_ih), ("bias_hh", inp.b_hh)):
        p = getattr(m, key + sfx)
        p.copy_(src[d].to(dtype))
        if wrong == "swap_gates":
          blk0, blk1 = p[:H].clone(), p[H:2 * H].clone()
          p[:H], p[H:2 * H] = blk1, blk0
        if wrong == "drop_b_hn" and key == "bias_hh":
          p[2 * H:] = 0
  x = inp.x.detach().to(dtype).clone().requires_grad_(True)
  packed = torch.nn.utils.rnn.pack_padded_sequence(x, inp.lens, batch_first=True, enforce_sorted=False)
  out, state = m(packed)
  y, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=c.T)
  h_n, c_n = state if c.cell == "LSTM" else (state, None)
  if wrong == "reverse_from_end":
    y_u, state_u = m(x)
    h_u, c_u = state_u if c.cell == "LSTM" else (state_u, None)
    y = torch.cat([y[..., :H], y_u[..., H:] * valid_mask(name).to(dtype)], dim=-1)
    h_n = torch.stack([h_n[0], h_u[1]])
    if c_n is not None:
      c_n = torch.stack([c_n[0], c_u[1]])
  loss = (y * inp.dy.to(dtype)).sum() + (h_n * inp.dh_n.to(dtype)).sum()
  if c_n is not None:
    loss = loss + (c_n * inp.dc_n.to(dtype)).sum()
  loss.backward()
  res = {"y": y.detach(), "h_n": h_n.detach(), "dx": x.grad}
  if c_n is not None:
    res["c_n"] = c_n.detach()
  for d in range(c.D):
    sfx = "_l0" + ("_reverse" if d else "")
    for key, attr in (("dw_ih", "weight_ih"), ("dw_hh", "weight_hh"), ("db_ih", "bias_ih"), ("db_hh", "bias_hh")):
      res["%s%d" % (key, d)] = getattr(m, attr + sfx).grad
  return res


@functools.lru_cache(maxsize=None)
def reference(name):
  """(float64 truth, float32 CPU yardstick) of a case: computed once, shared, never written to."""
  return evaluate(name, torch.float64), evaluate(name, torch.float32)


def figures(got, want64):
  """(largest element-wise error relative to the float64 tensor's largest entry, relative norm of the error)."""
  diff = got.double() - want64
  scale = max(float(want64.abs().max()), 1e-30)
  return float(diff.abs().max()) / scale, float(diff.norm()) / max(float(want64.norm()), 1e-30)


# ---- the C ABI, called as lipreading_amd.encoder._RNNLayerFunction calls it ---------------------------------------------

def mode_of(case):
  from lipreading_amd import _C
  mode = {"GRU": _C.LR_RNN_GRU, "LSTM": _C.LR_RNN_LSTM, "RNN": _C.LR_RNN_TANH}[case.cell]
  for f in case.flags:
    mode |= getattr(_C, "LR_RNN_" + f)
  return mode


def dims_of(case):
  return case.B, case.T, case.I, case.H, case.D


def _ptrs(tensors):
  return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def run_layer(name, dev, accumulate=False, null_dh=False, null_dc=False, zero_state_grads=False, null_dx=False,
              null_hn=False, backwards=1, poison=True, x=None, parts=None, raise_on_error=True):
  """lr_rnn_layer_forward, then lr_rnn_layer_backward (or lr_rnn_layer_backward_parts once per entry of `parts`, into the
  same workspace) on the case; every output as a CPU tensor under tensor_names' keys.

  poison: outputs start as NaN, `reserve` / `workspace` as 0xFF bytes before the forward / each backward (the product
  hands over torch.empty memory: the kernels must define every word they later read); else everything starts as zeros.
  accumulate: the parameter gradients start as inputs(name).prefill and accumulate = 1 is passed.
  null_dh / null_dc / null_dx / null_hn: that pointer is NULL (h_n NULL: c_n too); zero_state_grads: dh_n, dc_n are zeros.
  backwards = 2: a second backward over the same forward's reserve; its results under "second".
  raise_on_error False: a non-zero status comes back as {"status": status} instead of raising."""
  from lipreading_amd import _C
  L = _C.lib()
  c, inp = CASES[name], inputs(name)
  B, T, I, H, D = dims_of(c)
  mode, GH, lstm = mode_of(c), GATES[c.cell] * H, c.cell == "LSTM"
  fill = float("nan") if poison else 0.0
  byte = 0xFF if poison else 0
  new = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=dev)

  # W_ih of both directions in ONE buffer: a multiple of 4 floats apart (separate torch tensors always are), plus
  # case.offset floats — W_ih[1] then starts that far past a 16-byte boundary
  stride = (GH * I + 3) // 4 * 4 + c.offset
  wbuf = torch.zeros(stride + GH * I + 4, dtype=torch.float32, device=dev)
  assert wbuf.data_ptr() % 16 == 0
  w_ih = [wbuf[d * stride:d * stride + GH * I].view(GH, I) for d in range(D)]
  for d in range(D):
    w_ih[d].copy_(inp.w_ih[d])
  w_hh = [t.to(dev) for t in inp.w_hh]
  b_ih = [t.to(dev) for t in inp.b_ih]
  b_hh = [t.to(dev) for t in inp.b_hh]
  xd = (inp.x if x is None else x).to(dev).contiguous()
  lens = inp.lens.to(torch.int32).to(dev)
  st = _C.stream_handle()
  dims = (B, T, I, H, D)

  y = new(B, T, D * H)
  h_n = None if null_hn else new(D, B, H)
  c_n = new(D, B, H) if (lstm and not null_hn) else None
  rbytes = L.lr_rnn_reserve_bytes(mode, *dims)
  reserve = torch.full((rbytes,), byte, dtype=torch.uint8, device=dev)
  status = L.lr_rnn_layer_forward(mode, xd.data_ptr(), lens.data_ptr(), _ptrs(w_ih), _ptrs(w_hh), _ptrs(b_ih), _ptrs(b_hh),
                                  y.data_ptr(), _C.ptr(h_n), _C.ptr(c_n), reserve.data_ptr(), rbytes, *dims, st)
  if status != 0 and not raise_on_error:
    return {"status": status}
  _C.check(status, "lr_rnn_layer_forward")

  zero = torch.zeros(D, B, H, device=dev)
  dy = inp.dy.to(dev)
  dh_n = None if null_dh else (zero if zero_state_grads else inp.dh_n.to(dev))
  dc_n = None if (null_dc or not lstm) else (zero if zero_state_grads else inp.dc_n.to(dev))
  wbytes = L.lr_rnn_workspace_bytes(mode, *dims)
  ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)
  keys = ("dw_ih", "dw_hh", "db_ih", "db_hh")
  shapes = {"dw_ih": (GH, I), "dw_hh": (GH, H), "db_ih": (GH,), "db_hh": (GH,)}
  out = {"y": y.cpu()}
  if h_n is not None:
    out["h_n"] = h_n.cpu()
  if c_n is not None:
    out["c_n"] = c_n.cpu()
  result = out
  for n in range(backwards):
    if accumulate:
      grads = {k: [inp.prefill["%s%d" % (k, d)].to(dev) for d in range(D)] for k in keys}
    else:
      grads = {k: [new(*shapes[k]) for d in range(D)] for k in keys}
    dx = None if null_dx else new(B, T, I)
    ws.fill_(byte)
    args = (mode, xd.data_ptr(), lens.data_ptr(), _ptrs(w_ih), _ptrs(w_hh), _ptrs(b_ih), _ptrs(b_hh), y.data_ptr(),
            dy.data_ptr(), _C.ptr(dh_n), _C.ptr(dc_n), _C.ptr(dx), _ptrs(grads["dw_ih"]), _ptrs(grads["dw_hh"]),
            _ptrs(grads["db_ih"]), _ptrs(grads["db_hh"]), reserve.data_ptr(), rbytes, ws.data_ptr(), wbytes,
            1 if accumulate else 0, *dims)
    if parts is None:
      statuses = [(L.lr_rnn_layer_backward(*args, st), "lr_rnn_layer_backward")]
    else:
      statuses = []
      for p in parts:
        statuses.append((L.lr_rnn_layer_backward_parts(*args, p, st), "lr_rnn_layer_backward_parts(%d)" % p))
        if statuses[-1][0] != 0:
          break
    for status, what in statuses:
      if status != 0 and not raise_on_error:
        return {"status": status}
      _C.check(status, what)
    if n == 1:
      result = out["second"] = {}
    if dx is not None:
      result["dx"] = dx.cpu()
    for k in keys:
      for d in range(D):
        result["%s%d" % (k, d)] = grads[k][d].cpu()
  return out
