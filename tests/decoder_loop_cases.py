"""The seeded cases of tests/test_gpu_decoder_fp64.py (the attention decoder loop through lr_decoder_forward /
lr_decoder_backward[_parts]), what a plain restatement of the reference's CharDecodingStep loop says about them in float64
and in float32, the sampler's rule in Python integers, and the one helper that calls the C ABI.  Shared with
tests/test_decoder_loop_cases_cpu.py, which checks on the CPU that the table is what it claims to be.  Importable without a
GPU; nothing here looks at a device result.

The reference is the step include/lipreading_hip.h cites (better_model.py:161-231, oracle.torch_oracle.OracleCharDecodingStep)
looped L times: embedding -> torch.nn cells, one layer at a time so that the inter-layer drop mask can sit between them ->
attention over the encoder states -> the oracle's masked_softmax -> context -> concat_layer + tanh -> output_proj -> the
oracle's masked_log_softmax (whose log(mask + 1e-45) is evaluated in float32 in BOTH dtypes: -103.2789, what the kernel
adds).  loss = (log_probs . d_log_probs) + (h_n . dh_n) [+ (c_n . dc_n)] with seeded factors, so autograd's gradients are
what lr_decoder_backward returns for those three inputs.

The shapes are the smallest at which each dispatch branch of lr_decoder_forward / lr_decoder_backward_parts can still go
wrong, not the workload's: every case says which branch it expects (`recur`, `bwd`, `wgrad`, `out_rows`), and the CPU test
recomputes that from the arithmetic of lr_decoder.hip and lr_rnn_cluster.hip."""
import collections
import ctypes
import functools
import zlib

import torch

from oracle import torch_oracle as O

ULP = 2.0 ** -23
GATES = {"GRU": 3, "LSTM": 4, "RNN": 1}
ATTN = {"none": 0, "dot": 1, "general": 2, "1_layer_nn": 3, "concat": 4}
PAD_ID, BOS_ID = 0, 1            # the two classes the output mask removes (better_model.py:142-144)
DRAW_SLACK = 1e-5                # |u * total - class boundary| below which either neighbour is a correct draw

# name cell layers attn B L T Hd Cd V A | tf: teacher_forced_host | drop: a seeded inter-layer mask (entries 0 or 2.0) |
# bias: what is ADDED to the attention's score bias (attn_proj_1_layer_nn.bias) | seed: the sampler's |
# recur:    the FORWARD recurrence: step / cluster32:<members> / cluster16:<members> / grid (one launch: every step after
#           the first teacher forced, on a shape the cluster recurrence covers)
# bwd:      the BACKWARD recurrence: the loop's backward needs no draw, so it takes the one-launch kernels wherever the shape
#           has them, whatever the teacher-forcing pattern (lr_decoder_backward_parts: `else if (w.xch_bytes)`) — a case with
#           sampled-input steps runs its forward on the step kernels and its backward on the cluster recurrence
# wgrad:    grouped (lr_sgemm_grouped_tn_impl, exact fp32) / fgemm (split-bf16 products, G * Hd >= 1536)
# out_rows: rows per workgroup of dec_out_fwd_kernel (8, halved while (Hd + V) * 4 * rows > 60 KiB)
Case = collections.namedtuple("Case", "name cell layers attn B L T Hd Cd V A tf drop bias seed recur bwd wgrad out_rows")


def _c(name, cell, layers, attn, B, L, T, Hd, Cd, V, recur, wgrad, out_rows=8, A=0, tf=None, drop=False, bias=0.0, seed=11,
       bwd=None):
  tf = tuple(int(x) for x in (tf if tf is not None else [1] * L))
  assert len(tf) == L
  return Case(name, cell, layers, attn, B, L, T, Hd, Cd, V, A, tf, drop, bias, seed, recur, bwd if bwd is not None else recur, wgrad, out_rows)


CASES = collections.OrderedDict((c.name, c) for c in [
    # ---- step kernels: a mixed teacher-forcing pattern (head flushes between the runs), or G = 1 ----
    _c("step_gru40_1lnn", "GRU", 1, "1_layer_nn", 5, 6, 9, 40, 10, 64, "step", "grouped", tf=[1, 1, 0, 1, 0, 0], bwd="cluster32:2"),
    # (the first step is "not teacher forced" and must still read tokens; T > 64: two passes of the softmax kernels' lanes,
    # with lengths below 64; V, Cd, A all odd)
    _c("step_lstm36_concat_l2_drop", "LSTM", 2, "concat", 5, 5, 70, 36, 7, 37, "step", "grouped", A=23, tf=[0, 1, 0, 1, 1],
       drop=True, bwd="cluster32:2"),
    _c("step_gru24_general_l3", "GRU", 3, "general", 17, 4, 3, 24, 12, 64, "step", "grouped", tf=[1, 0, 1, 1], seed=12,
       bwd="cluster32:1"),
    # (G = 1 never takes the one-launch path; V = 130: three passes of the class loops, the last of two classes)
    _c("step_rnn20_dot", "RNN", 1, "dot", 3, 5, 6, 20, 6, 130, "step", "grouped"),
    # ---- the one-launch recurrence: every step teacher forced ----
    _c("one_gru40_dot", "GRU", 1, "dot", 9, 6, 12, 40, 10, 64, "cluster32:2", "grouped"),
    # (every valid logit near -25: the 1e-13 of masked_softmax carries about 1 % of the attention weights, and the score bias
    # has a real gradient)
    _c("one_lstm36_1lnn_bias25", "LSTM", 1, "1_layer_nn", 5, 5, 9, 36, 9, 50, "cluster32:2", "grouped", bias=-25.0),
    _c("one_lstm384_general", "LSTM", 1, "general", 4, 3, 7, 384, 12, 64, "cluster32:12", "fgemm"),
    _c("one_gru512_none_l2", "GRU", 2, "none", 9, 3, 4, 512, 10, 64, "cluster32:16", "fgemm"),
    _c("one_lstm800_concat", "LSTM", 1, "concat", 4, 4, 5, 800, 12, 64, "cluster16:50", "fgemm", A=70),
    _c("one_lstm1156_dot", "LSTM", 1, "dot", 3, 3, 4, 1156, 8, 64, "grid", "fgemm"),
    _c("one_gru900_none_v1024", "GRU", 1, "none", 9, 2, 3, 900, 6, 1024, "cluster16:58", "fgemm", out_rows=4),
    _c("one_lstm20_none_single", "LSTM", 1, "none", 1, 1, 1, 20, 5, 64, "cluster32:1", "grouped"),
])
# where the bit-exact properties run: one step case, one cluster case, the wide case and the grid case
PROPERTY_CASES = ["step_gru40_1lnn", "one_gru40_dot", "one_lstm384_general", "one_lstm1156_dot"]
NONE_CASE = "one_gru512_none_l2"           # attention none: d_enc is zero throughout; two layers: parts 1 / 2 are refused
BIAS_CASE = "one_lstm36_1lnn_bias25"


def one_launch(case):
  """The forward recurrence (and so the backward one) is one launch per layer."""
  return case.recur != "step"


def one_launch_bwd(case):
  return case.bwd != "step"


FORWARD_KEYS = ("log_probs", "h_n", "c_n")


def wide(case):
  return case.wgrad == "fgemm"


def step_twin(case):
  """The case also runs on the step kernels, forward and backward, through the lr_rnn_debug_disable_cluster hook."""
  return one_launch_bwd(case)


def upper_keys(case):
  return ["%s%d" % (k, l) for l in range(1, case.layers) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]


def attn_keys(case):
  return {"none": [], "dot": [], "general": ["attn_w1", "attn_b1"], "1_layer_nn": ["attn_w1", "attn_b1"],
          "concat": ["attn_w1", "attn_b1", "attn_w2", "attn_b2"]}[case.attn]


FIELDS = ("emb", "w_ih", "w_hh", "b_ih", "b_hh", "attn_w1", "attn_b1", "attn_w2", "attn_b2", "w_c", "b_c", "w_o", "b_o")


def param_keys(case):
  """The parameters the case's loop reads (lr_decoder_params' field names; `<field><layer>` for the layers above the first)."""
  keys = ["emb", "w_ih", "w_hh", "b_ih", "b_hh"] + attn_keys(case)
  if case.attn != "none":
    keys += ["w_c", "b_c"]
  return keys + ["w_o", "b_o"] + upper_keys(case)


def grad_keys(case):
  return ["d_" + k for k in param_keys(case)]


def state_keys(case):
  return ["h_n"] + (["c_n"] if case.cell == "LSTM" else [])


def tensor_names(case):
  """Every tensor the ABI returns for the case."""
  return ["log_probs"] + state_keys(case) + ["d_enc", "dh0"] + (["dc0"] if case.cell == "LSTM" else []) + grad_keys(case)


# The score bias of '1_layer_nn' and attn_proj_layer2.bias of 'concat' have a mathematically zero gradient unless the
# 1e-13 matters (softmax shift invariance): float64 says 1e-12 and fp32 rounding is 5e4 times that.  They are held on the
# scale of the sibling weight gradient, the CPU figure taken on the same scale.
def scale_key(case, key):
  if case.attn == "1_layer_nn" and key == "d_attn_b1":
    return "d_attn_w1"
  if case.attn == "concat" and key == "d_attn_b2":
    return "d_attn_w2"
  return key


def allowance(case, key, hooked=False):
  """(element-wise, relative norm) figures ADDED to the exact bound 4 x max(cpu fp32 error, 1 ulp) where the case leaves
  exact fp32 — the project's own figures: the 1e-4 of rnn_layer_cases.allowance and the 5e-5 in relative norm of
  test_decoder_loop_on_the_cluster_recurrence_equals_the_step_kernels.  On the one-launch recurrence every tensor is
  downstream of the states — every tensor of a case whose forward is one launch, every tensor of the BACKWARD where only
  the backward is; on the step kernels (hooked: lr_rnn_debug_disable_cluster, or a shape without a one-launch kernel) only
  a wide case's split-bf16 weight gradients (W_hh of every layer, W_ih of the layers above the first).  (0, None): no norm
  check, nothing added."""
  if not hooked and (one_launch(case) or (one_launch_bwd(case) and key not in FORWARD_KEYS)):
    return 1e-4, 5e-5
  if wide(case) and (key.startswith("d_w_hh") or (key.startswith("d_w_ih") and key != "d_w_ih")):
    return 1e-4, 5e-5
  return 0.0, None


def bounds(case, key, cpu_err, hooked=False):
  base = 4 * max(cpu_err, ULP)
  elem, norm = allowance(case, key, hooked)
  return base + elem, None if norm is None else base + norm


def figures(got, want64, scale64=None):
  """(largest element-wise error relative to the largest entry of scale64, relative norm of the error against scale64's);
  scale64 defaults to the float64 tensor itself."""
  ref = want64 if scale64 is None else scale64
  diff = got.double() - want64
  if diff.numel() == 0:
    return 0.0, 0.0
  return float(diff.abs().max()) / max(float(ref.abs().max()), 1e-30), float(diff.norm()) / max(float(ref.norm()), 1e-30)


def out_mask(V):
  m = torch.ones(V)
  m[PAD_ID] = 0
  m[BOS_ID] = 0
  return m


def split_log_probs(lp):
  """log_probs in two column groups: the masked classes sit at about -103 and would hide an error 20 times the size of the
  live classes' values — (live [B, L, V - 2], masked [B, L, 2])."""
  return lp[..., 2:], lp[..., :2]


def pieces(case, key, got, want64):
  """What of a tensor is held against what, on which scale: [(label, got, float64 truth, float64 tensor that sets the
  scale)] — log_probs in its two column groups, the shift-invariant biases on their sibling's scale."""
  if key == "log_probs":
    return [(key + tag, a, b, b) for tag, a, b in zip((" live", " masked"), split_log_probs(got[key]), split_log_probs(want64[key]))]
  return [(key, got[key], want64[key], want64[scale_key(case, key)])]


Inputs = collections.namedtuple("Inputs", "enc lens h0 c0 tokens params drop d_lp dh_n dc_n prefill garbage")


@functools.lru_cache(maxsize=None)
def inputs(name):
  """Seeded float32 inputs of a case (CPU).  lens: ragged, the last sample full, no other one, sample 1 a single frame
  wherever B >= 3.  prefill: what accumulate = 1 adds to; garbage: values of magnitude 1e3 for the frames of enc past each
  length."""
  c = CASES[name]
  g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
  G, Hd, NL = GATES[c.cell], c.Hd, c.layers
  GH = G * Hd
  enc = torch.randn(c.B, c.T, Hd, generator=g) * 0.5
  lens = torch.randint(1, max(c.T, 2), (c.B,), generator=g).clamp_(max=c.T)      # 1 .. T - 1: never the full length
  lens[c.B - 1] = c.T
  if c.B >= 3:
    lens[1] = 1
  h0 = torch.randn(NL, c.B, Hd, generator=g) * 0.5
  c0 = torch.randn(NL, c.B, Hd, generator=g) * 0.5
  tokens = torch.randint(2, c.V, (c.B, c.L), generator=g)
  uni = lambda k, *shape: (torch.rand(*shape, generator=g) * 2 - 1) * k
  k = Hd ** -0.5
  P = collections.OrderedDict()
  P["emb"] = torch.randn(c.V, c.Cd, generator=g)
  P["w_ih"], P["w_hh"], P["b_ih"], P["b_hh"] = uni(k, GH, c.Cd), uni(k, GH, Hd), uni(k, GH), uni(k, GH)
  k2 = (2 * Hd) ** -0.5
  if c.attn == "general":
    P["attn_w1"], P["attn_b1"] = uni(k, Hd, Hd), uni(k, Hd)
  elif c.attn == "1_layer_nn":
    P["attn_w1"], P["attn_b1"] = uni(k2, 1, 2 * Hd), uni(k2, 1) + c.bias
  elif c.attn == "concat":
    ka = c.A ** -0.5
    P["attn_w1"], P["attn_b1"], P["attn_w2"], P["attn_b2"] = uni(k2, c.A, 2 * Hd), uni(k2, c.A), uni(ka, 1, c.A), uni(ka, 1)
  if c.attn != "none":
    P["w_c"], P["b_c"] = uni(k2, Hd, 2 * Hd), uni(k2, Hd)
  P["w_o"], P["b_o"] = uni(k, c.V, Hd), uni(k, c.V)
  for l in range(1, NL):
    P["w_ih%d" % l], P["w_hh%d" % l], P["b_ih%d" % l], P["b_hh%d" % l] = uni(k, GH, Hd), uni(k, GH, Hd), uni(k, GH), uni(k, GH)
  assert sorted(P) == sorted(param_keys(c))
  drop = None
  if c.drop:
    drop = torch.randint(0, 2, (NL - 1, c.B, c.L, Hd), generator=g).float() * 2.0
  d_lp = torch.randn(c.B, c.L, c.V, generator=g) / 10
  dh_n = torch.randn(NL, c.B, Hd, generator=g) / 10
  dc_n = torch.randn(NL, c.B, Hd, generator=g) / 10
  prefill = {"d_" + key: torch.randn(*p.shape, generator=g) for key, p in P.items()}
  sign = torch.randint(0, 2, (c.B, c.T, Hd), generator=g).float() * 2 - 1
  garbage = sign * (1e3 + 1e3 * torch.rand(c.B, c.T, Hd, generator=g))
  return Inputs(enc, lens, h0, c0, tokens, P, drop, d_lp, dh_n, dc_n, prefill, garbage)


def valid_mask(name):
  """[B, T, 1] bool: frame t of sample b exists."""
  c, inp = CASES[name], inputs(name)
  return (torch.arange(c.T).unsqueeze(0) < inp.lens.unsqueeze(1)).unsqueeze(-1)


def enc_with_garbage(name):
  inp = inputs(name)
  return torch.where(valid_mask(name), inp.enc, inp.garbage)


# ---- the sampler, as lr_decoder_dev.h defines it -------------------------------------------------------------------------

M64 = (1 << 64) - 1


def hash_uniform(seed, step, sample):
  """hash_uniform of lr_decoder_dev.h in Python integers: 24 random bits -> [0, 1), exact in float32 and float64."""
  x = (seed + 0x9E3779B97F4A7C15 * ((step * 0x100000001B3 + sample + 1) & M64)) & M64
  x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
  x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
  x ^= x >> 31
  return (x >> 40) / 16777216.0


def draw(lp_row, u):
  """The first class whose cumulative mass of exp(lp_row) exceeds u * total (V - 1 if none does), the cumulative sum in
  float64 -> (pick, lowest and highest class that a draw within DRAW_SLACK of a boundary may give instead, distance of
  u * total to the nearest class boundary)."""
  p = lp_row.double().exp()
  p = torch.where(lp_row.float().exp() == 0, torch.zeros_like(p), p)      # (a masked class: no mass in float32, none here)
  cum = torch.cumsum(p, 0)
  total = float(cum[-1])
  x = u * total
  V = len(cum)

  def first_past(y):
    hit = (cum > y).nonzero()
    return int(hit[0]) if len(hit) else V - 1
  live = cum[p > 0]                                    # the boundaries a draw can cross (a class of mass 0 has none)
  margin = float((live - x).abs().min())
  return first_past(x), first_past(x - DRAW_SLACK), first_past(x + DRAW_SLACK), margin


def draws(lp, seed):
  """draw() for every (sample, step) row of log_probs [B, L, V] -> (picks [B, L] int64, lo, hi, margins [B, L])."""
  B, L, _ = lp.shape
  pick, lo, hi = (torch.zeros(B, L, dtype=torch.int64) for _ in range(3))
  margin = torch.zeros(B, L, dtype=torch.float64)
  for b in range(B):
    for i in range(L):
      pick[b, i], lo[b, i], hi[b, i], margin[b, i] = draw(lp[b, i], hash_uniform(seed, i, b))
  return pick, lo, hi, margin


# ---- the reference ---------------------------------------------------------------------------------------------------------

WRONG = ("drop_1e13", "swap_concat_halves", "gru_b_hn_outside", "step0_sampled", "drop_top_layer", "lens_off_by_one")


def applies(wrong, case):
  """Which deliberately wrong references can differ from the right one on a case."""
  if wrong == "drop_1e13":
    return case.attn != "none" and case.B >= 3
  if wrong == "swap_concat_halves":
    return case.attn != "none"
  if wrong == "gru_b_hn_outside":
    return case.cell == "GRU"
  if wrong == "step0_sampled":
    return case.tf[0] == 0
  if wrong == "drop_top_layer":
    return case.drop
  if wrong == "lens_off_by_one":
    return case.attn != "none" and case.B >= 3
  raise KeyError(wrong)


def _masked_softmax_without_eps(vector, mask):
  mask = mask.float().unsqueeze(1) if mask.dim() < vector.dim() else mask.float()
  result = torch.softmax(vector * mask, dim=-1) * mask
  return result / result.sum(dim=-1, keepdim=True)


def _cell_step(case, cell, x, state, wrong):
  """One step of one layer: torch.nn's cell, or — wrong == "gru_b_hn_outside" — the GRU with b_hn outside r * (W_hn h)."""
  if case.cell == "LSTM":
    h, c = cell(x, state)
    return h, (h, c)
  if case.cell == "GRU" and wrong == "gru_b_hn_outside":
    H, h = case.Hd, state
    gi = x @ cell.weight_ih.t() + cell.bias_ih
    gh = h @ cell.weight_hh.t()
    r = torch.sigmoid(gi[:, :H] + gh[:, :H] + cell.bias_hh[:H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H] + cell.bias_hh[H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:] + cell.bias_hh[2 * H:])
    h = (1 - z) * n + z * h
    return h, h
  h = cell(x, state)
  return h, h


def evaluate(name, dtype, sampled=None, wrong=None):
  """The loop of the case in `dtype` on the CPU: every tensor of tensor_names(case), plus "sampled" (what fed the
  sampled-input steps).  sampled [B, L]: the draws to replay at the steps that are not teacher forced; None: the
  reference draws its own from its own log_probs by draw() with the case's seed.  wrong: one of WRONG, a reference that is
  deliberately NOT the loop."""
  c, inp = CASES[name], inputs(name)
  Hd, NL, B, L, V = c.Hd, c.layers, c.B, c.L, c.V
  P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in inp.params.items()}
  cls = {"GRU": torch.nn.GRUCell, "LSTM": torch.nn.LSTMCell, "RNN": torch.nn.RNNCell}[c.cell]
  cells = []
  for l in range(NL):
    sfx = "" if l == 0 else str(l)
    with torch.random.fork_rng():
      cell = cls(c.Cd if l == 0 else Hd, Hd).to(dtype)
    # the cell computes with OUR leaves, so autograd's gradients land on P
    del cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh
    cell.weight_ih, cell.weight_hh = P["w_ih" + sfx], P["w_hh" + sfx]
    cell.bias_ih, cell.bias_hh = P["b_ih" + sfx], P["b_hh" + sfx]
    cells.append(cell)
  enc = inp.enc.detach().to(dtype).clone().requires_grad_(True)
  h0 = inp.h0.detach().to(dtype).clone().requires_grad_(True)
  c0 = inp.c0.detach().to(dtype).clone().requires_grad_(True)
  lens = inp.lens
  if wrong == "lens_off_by_one":
    lens = (lens + 1).clamp(max=c.T)
  enc_mask = torch.arange(c.T).expand(B, c.T) < lens.unsqueeze(1)
  omask = out_mask(V)                                            # float32 in both dtypes
  softmax = _masked_softmax_without_eps if wrong == "drop_1e13" else O.masked_softmax
  drop = None if inp.drop is None else inp.drop.to(dtype)
  state = [(h0[l], c0[l]) if c.cell == "LSTM" else h0[l] for l in range(NL)]
  replay = None if sampled is None else sampled.long()
  drawn = torch.zeros(B, L, dtype=torch.int64)
  rows = []
  for i in range(L):
    if c.tf[i] or (i == 0 and wrong != "step0_sampled"):
      ids = inp.tokens[:, i]
    elif i == 0:       # (wrong) what a gather without its i == 0 rule reads: the word in front of the sample's row
      flat = (replay if replay is not None else inp.tokens).reshape(-1)
      ids = torch.stack([flat[b * L - 1] if b else torch.tensor(PAD_ID) for b in range(B)])
    else:
      ids = (replay if replay is not None else drawn)[:, i - 1].clone()
    x = P["emb"][ids]
    for l in range(NL):
      if l > 0 and drop is not None:
        x = x * drop[l - 1, :, i]
      x, state[l] = _cell_step(c, cells[l], x, state[l], wrong)
    if wrong == "drop_top_layer":
      x = x * drop[NL - 2, :, i]
    h = x
    if c.attn != "none":
      if c.attn == "1_layer_nn":
        w = P["attn_w1"][0]
        logits = enc @ w[:Hd] + (h @ w[Hd:]).unsqueeze(1) + P["attn_b1"]
      elif c.attn == "general":
        logits = ((h @ P["attn_w1"].t() + P["attn_b1"]).unsqueeze(1) * enc).sum(-1)
      elif c.attn == "dot":
        logits = (h.unsqueeze(1) * enc).sum(-1)
      else:
        both = torch.cat([enc, h.unsqueeze(1).expand_as(enc)], dim=2)
        logits = ((both @ P["attn_w1"].t() + P["attn_b1"]).tanh() @ P["attn_w2"].t() + P["attn_b2"]).squeeze(-1)
      wts = softmax(logits, enc_mask).unsqueeze(1)
      ctx = wts.bmm(enc).squeeze(1)
      w_c = P["w_c"]
      if wrong == "swap_concat_halves":
        w_c = torch.cat([w_c[:, Hd:], w_c[:, :Hd]], dim=1)
      h = (torch.cat([ctx, h], dim=1) @ w_c.t() + P["b_c"]).tanh()
    out = h @ P["w_o"].t() + P["b_o"]
    lp = O.masked_log_softmax(out, omask.expand(B, V))
    rows.append(lp)
    if replay is None:
      with torch.no_grad():
        for b in range(B):
          drawn[b, i] = draw(lp[b], hash_uniform(c.seed, i, b))[0]
  log_probs = torch.stack(rows, 1)
  h_n = torch.stack([s[0] if c.cell == "LSTM" else s for s in state])
  loss = (log_probs * inp.d_lp.to(dtype)).sum() + (h_n * inp.dh_n.to(dtype)).sum()
  res = {"log_probs": log_probs.detach(), "h_n": h_n.detach(), "sampled": drawn if replay is None else replay}
  if c.cell == "LSTM":
    c_n = torch.stack([s[1] for s in state])
    loss = loss + (c_n * inp.dc_n.to(dtype)).sum()
    res["c_n"] = c_n.detach()
  loss.backward()
  zeros = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
  res["d_enc"], res["dh0"] = zeros(enc), zeros(h0)
  if c.cell == "LSTM":
    res["dc0"] = zeros(c0)
  for k in param_keys(c):
    res["d_" + k] = zeros(P[k])
  return res


_REF = {}


def reference(name, sampled=None):
  """(float64 truth, float32 CPU yardstick) of a case for the given draws: computed once per (case, draws), shared, never
  written to.  With draws of its own the float32 yardstick replays the float64 result's."""
  key = (name, None if sampled is None else tuple(sampled.reshape(-1).tolist()))
  if key not in _REF:
    want64 = evaluate(name, torch.float64, sampled)
    _REF[key] = (want64, evaluate(name, torch.float32, want64["sampled"]))
  return _REF[key]


def needs_draws(case):
  """Some step of the loop is fed a draw: the reference has to replay the device's own."""
  return any(not t for t in case.tf[1:])


# ---- the C ABI, called as lipreading_amd.attention_decoder._AttnDecoderFunction calls it ----------------------------------

def mode_of(case):
  from lipreading_amd import _C
  return {"GRU": _C.LR_RNN_GRU, "LSTM": _C.LR_RNN_LSTM, "RNN": _C.LR_RNN_TANH}[case.cell]


def dims_of(case):
  return case.B, case.L, case.T, case.Hd, case.Cd, case.V, case.A


def run_loop(name, dev, accumulate=False, parts=None, null_dh=False, null_dc=False, zero_state_grads=False,
             null_hn=False, backwards=1, poison=True, enc=None, seed=None, steps=False, forward_only=False,
             raise_on_error=True):
  """lr_decoder_forward, then lr_decoder_backward (or lr_decoder_backward_parts once per entry of `parts`, into the same
  workspace) on the case; every output as a CPU tensor under tensor_names' keys, plus "sampled".

  poison: outputs start as NaN, `reserve` / `workspace` as 0xFF bytes before the forward / each backward (the product
  hands over torch.empty memory: the kernels must define every word they later read); else everything starts as zeros.
  accumulate: the parameter gradients start as inputs(name).prefill and accumulate = 1 is passed.
  null_dh / null_dc / null_hn: that pointer is NULL (h_n NULL: c_n too); zero_state_grads: dh_n, dc_n are zeros.
  enc: other encoder states than inputs(name).enc; seed: another sampler seed than the case's.
  backwards = 2: a second backward over the same forward's reserve; its results under "second".
  steps: the lr_rnn_debug_disable_cluster hook is set for the forward and its backwards (the step kernels run), and
  restored in any event.
  raise_on_error False: a non-zero status comes back as {"status": status} instead of raising."""
  from lipreading_amd import _C
  Lb = _C.lib()
  if steps:
    Lb.lr_rnn_debug_disable_cluster(1)
  try:
    return _run_loop(Lb, name, dev, accumulate, parts, null_dh, null_dc, zero_state_grads, null_hn, backwards, poison, enc,
                     seed, forward_only, raise_on_error)
  finally:
    if steps:
      Lb.lr_rnn_debug_disable_cluster(0)


def _run_loop(Lb, name, dev, accumulate, parts, null_dh, null_dc, zero_state_grads, null_hn, backwards, poison, enc, seed,
              forward_only, raise_on_error):
  from lipreading_amd import _C
  c, inp = CASES[name], inputs(name)
  B, L, T, Hd, Cd, V, A = dims_of(c)
  NL, lstm = c.layers, c.cell == "LSTM"
  mode, at = mode_of(c), ATTN[c.attn]
  fill = float("nan") if poison else 0.0
  byte = 0xFF if poison else 0
  new = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=dev)

  P = {k: v.to(dev).contiguous() for k, v in inp.params.items()}
  omask = out_mask(V).to(dev)
  pstruct = _C.DecoderParams(*[_C.ptr(P.get(k)) for k in FIELDS], omask.data_ptr())
  drop = None if inp.drop is None else inp.drop.to(dev).contiguous()
  ustruct = None
  if NL > 1:
    ustruct = _C.DecoderUpper()
    ustruct.num_layers = NL
    for l in range(1, NL):
      for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
        getattr(ustruct, k)[l - 1] = P["%s%d" % (k, l)].data_ptr()
    ustruct.drop_mask = _C.ptr(drop)
  uref = ctypes.byref(ustruct) if ustruct is not None else None
  encd = (inp.enc if enc is None else enc).to(dev).contiguous()
  lens = inp.lens.to(torch.int32).to(dev)
  step_lens = torch.full((B,), L, dtype=torch.int32, device=dev)
  tokens = inp.tokens.to(torch.int32).to(dev).contiguous()
  h0 = inp.h0.to(dev).contiguous()
  c0 = inp.c0.to(dev).contiguous() if lstm else None
  tf = (ctypes.c_uint8 * L)(*c.tf)
  st = _C.stream_handle()
  dims = (B, L, T, Hd, Cd, V, A)

  lp = new(B, L, V)
  sampled = torch.full((B, L), -1, dtype=torch.int32, device=dev)
  h_n = None if null_hn else new(NL, B, Hd)
  c_n = new(NL, B, Hd) if (lstm and not null_hn) else None
  rbytes = Lb.lr_decoder_reserve_bytes(mode, at, NL, *dims)
  assert rbytes > 0, "lr_decoder_reserve_bytes rejects the case's sizes"
  reserve = torch.full((rbytes,), byte, dtype=torch.uint8, device=dev)
  status = Lb.lr_decoder_forward(mode, at, ctypes.byref(pstruct), uref, tokens.data_ptr(), tf, encd.data_ptr(),
                                 lens.data_ptr(), h0.data_ptr(), _C.ptr(c0), step_lens.data_ptr(),
                                 (c.seed if seed is None else seed) & M64, lp.data_ptr(), sampled.data_ptr(), _C.ptr(h_n),
                                 _C.ptr(c_n), reserve.data_ptr(), rbytes, *dims, st)
  if status != 0 and not raise_on_error:
    return {"status": status}
  _C.check(status, "lr_decoder_forward")
  out = {"log_probs": lp.cpu(), "sampled": sampled.cpu().long()}
  if h_n is not None:
    out["h_n"] = h_n.cpu()
  if c_n is not None:
    out["c_n"] = c_n.cpu()
  if forward_only:
    return out

  zero = torch.zeros(NL, B, Hd, device=dev)
  d_lp = inp.d_lp.to(dev).contiguous()
  dh_n = None if null_dh else (zero if zero_state_grads else inp.dh_n.to(dev))
  dc_n = None if (null_dc or not lstm) else (zero if zero_state_grads else inp.dc_n.to(dev))
  wbytes = Lb.lr_decoder_workspace_bytes(mode, at, NL, *dims)
  assert wbytes > 0
  ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)
  result = out
  for n in range(backwards):
    if accumulate:
      G = {k: inp.prefill["d_" + k].to(dev).contiguous() for k in P}
    else:
      G = {k: new(*P[k].shape) for k in P}
    gstruct = _C.DecoderGrads(*[_C.ptr(G.get(k)) for k in FIELDS], PAD_ID)
    gustruct = None
    if NL > 1:
      gustruct = _C.DecoderUpperGrads()
      for l in range(1, NL):
        for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
          getattr(gustruct, k)[l - 1] = G["%s%d" % (k, l)].data_ptr()
    d_enc, dh0 = new(B, T, Hd), new(NL, B, Hd)
    dc0 = new(NL, B, Hd) if lstm else None
    ws.fill_(byte)
    args = (mode, at, ctypes.byref(pstruct), uref, ctypes.byref(gstruct),
            ctypes.byref(gustruct) if gustruct is not None else None, encd.data_ptr(), lens.data_ptr(), h0.data_ptr(),
            _C.ptr(c0), step_lens.data_ptr(), lp.data_ptr(), d_lp.data_ptr(), _C.ptr(dh_n), _C.ptr(dc_n), d_enc.data_ptr(),
            dh0.data_ptr(), _C.ptr(dc0), reserve.data_ptr(), rbytes, ws.data_ptr(), wbytes, 1 if accumulate else 0, *dims)
    if parts is None:
      statuses = [(Lb.lr_decoder_backward(*args, st), "lr_decoder_backward")]
    else:
      statuses = []
      for p in parts:
        statuses.append((Lb.lr_decoder_backward_parts(*args, p, st), "lr_decoder_backward_parts(%d)" % p))
        if statuses[-1][0] != 0:
          break
    for status, what in statuses:
      if status != 0 and not raise_on_error:
        return {"status": status}
      _C.check(status, what)
    if n == 1:
      result = out["second"] = {}
    result["d_enc"], result["dh0"] = d_enc.cpu(), dh0.cpu()
    if dc0 is not None:
      result["dc0"] = dc0.cpu()
    for k in P:
      result["d_" + k] = G[k].cpu()
  return out
