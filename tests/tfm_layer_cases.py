"""The seeded one-layer cases of tests/test_gpu_transformer_fp64.py and what the float64 reference says about them.
Shared with tests/test_tfm_layer_reference.py, which checks on the CPU that every case keeps enough rows graded.

A one-layer stack: the only gradient that reaches the feed-forward half of row r is dh_out[r].  A row is MARGINAL when
any feed-forward pre-activation |z[r, j]| of the float64 evaluation lies below the margin m; dh_out is zeroed there, in
the device run and in the reference alike, so such a row contributes exactly nothing to any gradient whichever way its
ReLU falls, and every other row's ReLU pattern is the reference's.  m = 8 x max |z_restated - z_64| (Z_ERR), where the
restatement is the device's arithmetic on the CPU (oracle.torch_oracle: fp32 throughout, every Linear a split-bf16
product in X3 mode), so z carries the error of everything upstream of it.  Nothing here looks at a device result."""
import functools

import torch

from oracle import torch_oracle as O

X3, F32 = "x3", "f32"

# (B, T, lens): row counts 32 k, 32 k + 1, 32 k + 31 and the bench's 32 x 75; ragged, a length of 1, the last sample
# full so that the last 32-row block's last row is a real frame
SHAPES = {
    64: (4, 16, [16, 1, 9, 16]),
    33: (3, 11, [11, 1, 11]),
    63: (3, 21, [13, 1, 21]),
    2400: (32, 75, None),
}
# name -> (B, T, lens, I, d_model, heads, F, seed).  The seeds were picked (from the reference alone: test_tfm_layer_reference
# asserts it) so that every 32-row block keeps a quarter of its rows and the single-row tail block of R = 33 is graded.
CASES = {}
for _F in (256, 512, 1024, 2048):
  for _R, (_B, _T, _lens) in SHAPES.items():
    CASES["d256_f%d_r%d" % (_F, _R)] = (_B, _T, _lens, 96, 256, 4, _F, 1000 + _F + _R)
# more than 256 row blocks (the row-block backward's partial sums take a second launch), K-split weight gradients, and a
# last block of ONE row
CASES["d256_f256_r8481"] = (33, 257, None, 96, 256, 4, 256, 9000)
CASES["d64_f128"] = (4, 20, [20, 7, 1, 20], 204, 64, 4, 128, 21)
CASES["d320_f388"] = (3, 33, [33, 1, 18], 100, 320, 5, 388, 22)
CASES["d512_f2048"] = (2, 33, [20, 33], 96, 512, 8, 2048, 23)
CASES["d1920_f64"] = (2, 9, [4, 9], 24, 1920, 8, 64, 24)   # the LayerNorm backward's LDS limit
CASES["d128_t96"] = (2, 96, [96, 40], 48, 128, 4, 256, 25)  # either side of the fused attention's T <= 96
CASES["d128_t97"] = (2, 97, [97, 40], 48, 128, 4, 256, 25)
for _k, _seed in {"d256_f2048_r64": 3113, "d256_f2048_r63": 3112, "d256_f2048_r2400": 5461, "d512_f2048": 26}.items():
  CASES[_k] = CASES[_k][:7] + (_seed,)   # (F = 2048 sits at the 30 % limit: the first seed counting up that stays below it)
ROWBLOCK_CASES = [k for k in CASES if k.startswith("d256_")]
GENERAL_CASES = [k for k in CASES if not k.startswith("d256_")]

OUTPUTS = ["h", "dx"] + O.TFM_LAYER_NAMES

# The CPU restatement's largest element-wise error against float64, relative to the float64 tensor's largest entry: the
# maximum over every case above, per kind of output (measured with reference() below; test_tfm_layer_reference asserts
# that the figures are what the restatement gives).  The device is allowed 4 x the figure: the same arithmetic in another summation
# order.  Per kind and not per tensor because the restatement's row sums are torch's pairwise ones: the bias and
# LayerNorm gradients of a single case come out as low as 1.5e-7, which no blocked order of 2400 rows can be held to.
#                  h        dx       weight matrices  bias / LayerNorm vectors
CPU_FIGURE = {X3: (5.3e-6, 9.9e-6, 1.8e-5, 8.8e-6),
              F32: (3.6e-7, 5.3e-7, 5.4e-7, 4.4e-7)}


# max |z_restated - z_64| per (case, mode, bf16 input, other lengths), measured with reference() below: the margin is 8 x
# this RECORDED figure, so that the set of graded rows does not move with the BLAS the restatement happens to run on
# (test_tfm_layer_reference holds the measured figure to the recorded one)
Z_ERR = {
    ('d256_f256_r8481', X3, False, None): 1.67e-05,
    ('d256_f256_r64', X3, False, None): 1.47e-05,
    ('d256_f256_r33', X3, False, None): 1.17e-05,
    ('d256_f256_r63', X3, False, None): 1.31e-05,
    ('d256_f256_r2400', X3, False, None): 1.65e-05,
    ('d256_f512_r64', X3, False, None): 1.4e-05,
    ('d256_f512_r33', X3, False, None): 1.3e-05,
    ('d256_f512_r63', X3, False, None): 1.56e-05,
    ('d256_f512_r2400', X3, False, None): 1.67e-05,
    ('d256_f1024_r64', X3, False, None): 1.39e-05,
    ('d256_f1024_r33', X3, False, None): 1.4e-05,
    ('d256_f1024_r63', X3, False, None): 1.44e-05,
    ('d256_f1024_r2400', X3, False, None): 1.52e-05,
    ('d256_f2048_r64', X3, False, None): 1.56e-05,
    ('d256_f2048_r33', X3, False, None): 1.44e-05,
    ('d256_f2048_r63', X3, False, None): 1.49e-05,
    ('d256_f2048_r2400', X3, False, None): 1.6e-05,
    ('d64_f128', X3, False, None): 1.44e-05,
    ('d64_f128', F32, False, None): 9.54e-07,
    ('d320_f388', X3, False, None): 1.46e-05,
    ('d320_f388', F32, False, None): 1.76e-06,
    ('d512_f2048', X3, False, None): 1.54e-05,
    ('d512_f2048', F32, False, None): 1.48e-06,
    ('d1920_f64', X3, False, None): 1.17e-05,
    ('d1920_f64', F32, False, None): 7.28e-07,
    ('d128_t96', X3, False, None): 1.53e-05,
    ('d128_t96', F32, False, None): 1.2e-06,
    ('d128_t97', X3, False, None): 1.63e-05,
    ('d128_t97', F32, False, None): 1.7e-06,
    ('d256_f512_r63', X3, True, None): 1.36e-05,
    ('d256_f1024_r2400', X3, True, None): 1.4e-05,
    ('d256_f256_r64', X3, False, (16, 1, 0, 16)): 1.47e-05,
    ('d128_t96', X3, False, (96, 0)): 1.64e-05,
}


def kind(output):
  return 0 if output == "h" else 1 if output == "dx" else 2 if output.endswith("weight") and "norm" not in output else 3


def cpu_figure(mode, output):
  return CPU_FIGURE[mode][kind(output)]


def case_lens(name):
  B, T, lens = CASES[name][:3]
  if lens is None:   # the bench's ragged batch: lengths 20 .. T, one of 1, first and last full
    lens = [int(v) for v in torch.randint(20, T + 1, (B,), generator=torch.Generator().manual_seed(9))]
    lens[0], lens[1], lens[-1] = T, 1, T
  return torch.tensor(lens, dtype=torch.int64)


def case_tensors(name):
  """-> x [B,T,I], lens, the 14 weights (torch's initialisation, with the zero biases and unit LayerNorm weights moved
  off their special values), pe, dh_out [B,T,Dm]; all float32."""
  from lipreading_amd.transformer import sinusoidal_encoding
  B, T, _, I, Dm, nhead, F, seed = CASES[name]
  torch.manual_seed(seed)
  proj = torch.nn.Linear(I, Dm)
  layer = torch.nn.TransformerEncoderLayer(Dm, nhead, F, dropout=0.0, activation='relu', batch_first=True, norm_first=False)
  at = layer.self_attn
  W = [proj.weight, proj.bias, at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias, layer.linear1.weight,
       layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm1.weight, layer.norm1.bias, layer.norm2.weight,
       layer.norm2.bias]
  W = [w.detach().clone() for w in W]
  for i in (3, 5):
    W[i] = 0.02 * torch.randn_like(W[i])
  for i in (10, 12):
    W[i] = 1.0 + 0.1 * torch.randn_like(W[i])
  for i in (11, 13):
    W[i] = 0.1 * torch.randn_like(W[i])
  x = torch.randn(B, T, I)
  dh = torch.randn(B, T, Dm)
  return x, case_lens(name), W, sinusoidal_encoding(T, Dm), dh


def rel_err(a, ref):
  """largest element-wise deviation relative to the float64 tensor's largest entry"""
  return float((a.double() - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def reference(name, mode, bf16_input=False, lens=None):
  """-> dict: 'want' (float64 h, dx, 14 gradients by name), 'cpu_err' (the restatement's rel_err per output: the
  figure a bound is derived from), 'dh' (the upstream gradient with marginal rows zeroed, float32 [B,T,Dm]), 'marginal'
  [B*T] bool, 'm', 'z_err', and the float32 inputs.  bf16_input: x rounded to bf16 first; lens: other lengths (a tuple)."""
  x, case_len, W, pe, dh = case_tensors(name)
  lens_key = lens
  lens = case_len if lens is None else torch.tensor(lens, dtype=torch.int64)
  if bf16_input:
    x = x.bfloat16().float()
  nhead = CASES[name][5]
  mm = O.split_bf16_matmul if mode == X3 else torch.matmul
  W64 = [w.double() for w in W]
  c64 = O.tfm_layer_forward(x.double(), lens, W64, pe.double(), nhead)
  c32 = O.tfm_layer_forward(x, lens, W, pe, nhead, mm=mm)
  z_err = float((c32["z"].double() - c64["z"]).abs().max())
  m = 8.0 * Z_ERR[(name, mode, bf16_input, lens_key)]
  marginal = (c64["z"].abs() < m).any(-1)
  dh = dh.reshape(-1, dh.shape[-1]).clone()
  dh[marginal] = 0
  dx64, g64 = O.tfm_layer_backward(c64, W64, dh.double())
  dx32, g32 = O.tfm_layer_backward(c32, W, dh, mm=mm)
  want = dict(zip(OUTPUTS, [c64["h2"], dx64] + g64))
  got = dict(zip(OUTPUTS, [c32["h2"], dx32] + g32))
  return {"want": want, "cpu_err": {k: rel_err(got[k], want[k]) for k in OUTPUTS}, "dh": dh.reshape(x.shape[0], x.shape[1], -1),
          "marginal": marginal, "m": m, "z_err": z_err, "z_std": float(c64["z"].std()), "x": x, "lens": lens, "W": W, "pe": pe}


def exclusion_report(marginal):
  """-> (share of marginal rows, [(rows, graded) per 32-row block])"""
  R = marginal.numel()
  blocks = [(min(32, R - r0), int((~marginal[r0:r0 + 32]).sum())) for r0 in range(0, R, 32)]
  return float(marginal.float().mean()), blocks


def assert_exclusion_is_harmless(marginal):
  """the conditions that keep the exclusion from hiding a failure, from the float64 reference alone"""
  share, blocks = exclusion_report(marginal)
  assert share <= 0.30, share
  for i, (rows, graded) in enumerate(blocks):
    assert graded >= 1 and 4 * graded >= rows, (i, rows, graded)
