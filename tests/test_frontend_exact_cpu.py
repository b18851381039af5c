"""Host only: what makes tests/test_gpu_frontend_exact.py trustworthy without a GPU.  For every entry of the case
table of tests/frontend_exact_cases.py: the conditions under which equality with the fp64 reference is the right bar
(conditions on the reference alone, nothing measured on a kernel), that the pooling inputs tie often enough to
exercise the first-maximum rule, that the reference agrees with itself, and that compare_exact rejects four kinds of
wrong reference — so the operands are dense enough at the edges for a one-term error to surface."""
import numpy as np
import pytest
import torch

from tests import frontend_exact_cases as FC

NAMES = [c.name for c in FC.CASES]


def _rejects(mutant, want, what):
  with pytest.raises(AssertionError, match="values differ"):
    FC.compare_exact(mutant, want, what)


# ---------------------------------------------------------------------------------------------------------------
# conditions on the inputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_expected_output_is_an_exactly_representable_integer(name):
  p = FC.problem(name)
  for op in p.case.ops:
    for key, (want, kind) in p.expected(op).items():
      want = want.double()
      assert bool((want == want.round()).all()), (op, key)
      top = float(want.abs().max())
      assert top > 0, (op, key)
      if kind == "bf16":
        assert top <= FC.BF16_EXACT, (op, key, top)
      elif kind == "f32":
        assert top < FC.F32_EXACT, (op, key, top)
      else:
        assert top <= 4, (op, key, top)
  # the operands themselves
  assert set(p.w.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(p.dz.unique().tolist()) == {-1.0, 0.0, 1.0}
  assert float(p.bias.abs().max()) <= 3
  if p.case.layer.cin == 3:
    assert set(p.clip.unique().tolist()) == {0, 255} and set(p.x.unique().tolist()) == {0.0, 1.0}
  else:
    assert set(p.x.unique().tolist()) == {-1.0, 0.0, 1.0}


def test_the_measured_margins_hold():
  """Layer geometries at B = 2, T = 5 with half the weights zeroed: the pre-activation, dX and dW maxima stay well
  inside 256 (bf16) — the margin the case table relies on (pre-activation / dX / dW measured 109 / 147 / 206 on layer
  2, 87 / 107 / 107 on layer 3, 29 / 48 / 73 on layer 1)."""
  for lname, layer, H, W, bound in (("l2", FC.L2, 24, 24, 200), ("l3", FC.L3, 12, 12, 160), ("l1", FC.L1, 32, 32, 80)):
    ops = ("fwd", "wgrad") + (("dgrad",) if layer.stride == 1 else ())
    p = FC.Problem(FC.Case("margin-" + lname, "margin", layer, 2, 5, H, W, ops, 0.5))
    assert float(p.z.abs().max()) <= bound, (lname, float(p.z.abs().max()))
    if layer.stride == 1:
      assert float(p.dx.abs().max()) <= FC.BF16_EXACT - 56, (lname, float(p.dx.abs().max()))
    assert float(p.dw.abs().max()) < 1000, (lname, float(p.dw.abs().max()))


def _tie_census(z):
  positive, tied, first = FC.pool_ties(z)
  ties = positive & tied
  return int(positive.sum()), int(ties.sum()), {j: int((ties & (first == j)).sum()) for j in range(4)}


@pytest.mark.parametrize("name", [c.name for c in FC.CASES if any(op.endswith("_pooled") for op in c.ops)])
def test_conv_epilogue_cases_tie_and_use_every_code(name):
  p = FC.problem(name)
  assert set(np.unique(p.code.numpy()).tolist()) == {0, 1, 2, 3, 4}
  if "fwd_pooled" not in p.case.ops:
    return   # codes drawn uniformly: nothing to tie
  positive, ties, by_first = _tie_census(p.z + p.bias)
  assert ties >= 100, (ties, positive)
  assert min(by_first[0], by_first[1], by_first[2]) > 0, by_first
  # the code is 4 exactly where the pooled value is 0
  pooled, code = p.pooled_code
  assert bool(((code == 4) == (pooled == 0)).all())


@pytest.mark.parametrize("C,frames,H,W", FC.POOL_CASES)
def test_pool_only_cases_tie_and_use_every_code(C, frames, H, W):
  act, dP = FC.pool_problem(C, frames, H, W)
  assert set(act.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
  positive, ties, by_first = _tie_census(act)
  assert ties >= 0.2 * positive, (ties, positive)
  assert min(by_first[0], by_first[1], by_first[2]) > 0, by_first
  assert set(np.unique(FC.relu_pool(act)[1].numpy()).tolist()) == {0, 1, 2, 3, 4}
  assert float(FC.bias_grad(FC.unpool_from_act(act, dP)).abs().max()) < FC.F32_EXACT
  # the operands tell the first maximum from the last: in the routed gradient and in the codes
  _rejects(FC.unpool_from_act(act, dP, first=False), FC.unpool_from_act(act, dP), "dZ by the last maximum")
  _rejects(FC.relu_pool(act, first=False)[1], FC.relu_pool(act)[1], "code of the last maximum")


@pytest.mark.parametrize("name", NAMES)
def test_each_case_reaches_the_kernel_it_is_for(name):
  """The host dispatch of lipreading_amd/csrc/lr_conv.hip, restated in frontend_exact_cases: the group a case is listed under is the
  kernel its shape reaches."""
  c = FC.BY_NAME[name]
  L = c.layer
  if c.group == "first":
    assert L is FC.L1
    return
  bit = FC.patch_bit(c.H, c.W, L.cin, L.cout, L.k)
  assert bit == {"patch2": 2, "patch3": 4}.get(c.group, bit)
  if c.group in ("patch2", "patch3"):
    assert FC.patch_bit(c.H, c.W, L.cout, L.cin, L.k) == bit     # the data gradient too
  if c.group == "igemm":
    assert bit == 0 and FC.patch_bit(c.H, c.W, L.cout, L.cin, L.k) == 0
  if c.group in ("tr2", "ts", "split"):
    assert FC.wgrad_path(L, c.B * c.T, c.H, c.W) == c.group
  if "wgrad" in c.ops:
    # every weight-gradient group has a clip of one or two frames: temporal taps leave the clip on both sides
    assert any(o.T <= 2 for o in FC.cases(c.group, "wgrad") if o.layer is L)


def test_the_tile_table_limit_of_the_transpose_read_kernel_is_restated():
  """lr_conv_wgrad_tr2_supported: the 90-frame cases fit with room to spare; the restatement does say no somewhere
  (layer 2 at 24 rows: 160 KB - 2 x 73,728 bytes of buffers = 16,384 bytes = 512 table rows: 511 tiles per workgroup,
  43,435 tiles of two frames x six rows = 21,716 frames)."""
  assert FC.tr2_table_fits(FC.L2, 90, 24) and FC.tr2_table_fits(FC.L3, 90, 12)
  assert FC.wgrad_path(FC.L2, 21716, 24, 24) == "tr2" and FC.wgrad_path(FC.L2, 21717, 24, 24) == "ts"
  assert not FC.tr2_tile_rows(FC.L3, 8) and FC.tr2_tile_rows(FC.L2, 16) == 4


def _walk_census(walks):
  """What the walks of more than one tile go through: (longest, steps into t >= 3, from the end of a window to the
  next in the same tile row, to the next tile row, to the next clip)."""
  later, window, row, clip = 0, 0, 0, 0
  for walk in walks:
    for (c0, y0, x0, t0), (c1, y1, x1, t1) in zip(walk, walk[1:]):
      later += t1 >= 3
      window += t1 == 0 and (c1, y1) == (c0, y0) and x1 != x0
      row += t1 == 0 and c1 == c0 and y1 != y0
      clip += c1 != c0
  return max(len(w) for w in walks), later, window, row, clip


def test_the_first_layer_cases_make_the_persistent_workgroups_walk():
  """lr_conv1.hip: the forward launches min(tiles, 768) workgroups, the weight gradient 256; workgroup i walks tiles
  [N i / G, N (i + 1) / G) of the order (clip, tile row, tile column, t).  The small cases give every workgroup one
  tile; the four walk cases cover two tiles, several tiles, the steady state of the weight gradient's loads (three
  tiles ahead: walks of five and more), and steps into t >= 3, across the end of a window, of a tile row and of a
  clip — in the forward and in the weight gradient."""
  lengths = {}
  for c in FC.cases("first"):
    for op, nwg in (("fwd", FC.C1_FWD_WGS), ("wgrad", FC.C1_WGRAD_WGS)):
      if op in c.ops:
        walks = FC.first_layer_walks(c, nwg)
        assert sorted(t for w in walks for t in w) == sorted(
          (b, y, x, t) for b in range(c.B) for y in range(2 if c.H > 32 else 1) for x in range(2 if c.W > 32 else 1)
          for t in range(c.T))
        lengths[c.name, op] = _walk_census(walks)
  for (name, op), census in lengths.items():
    if "T7" not in name and "B33" not in name:
      assert census[0] == 1, (name, op)
  assert lengths["first-l1-B33T2-40x36", "wgrad"][0] == 2
  assert lengths["first-l1-B10T7-40x36", "wgrad"][0] == 2 and lengths["first-l1-B10T7-40x36", "wgrad"][1] > 0
  assert lengths["first-l1-B28T7-40x36", "fwd"][:2] == (2, 16)     # sixteen workgroups walk two tiles, inside a window
  longest, later, window, row, clip = lengths["first-l1-B28T7-40x36", "wgrad"]
  assert longest == 4 and min(later, window, row, clip) > 0
  longest, later, window, row, clip = lengths["first-l1-B55T7-40x36", "fwd"]
  assert longest == 3 and min(later, window, row, clip) > 0
  longest, later, window, row, clip = lengths["first-l1-B55T7-40x36", "wgrad"]
  assert longest == 7 and min(later, window, row, clip) > 0
  assert min(len(w) for w in FC.first_layer_walks(FC.BY_NAME["first-l1-B55T7-40x36"], FC.C1_WGRAD_WGS)) >= 6


def test_the_tap_stationary_cases_walk_and_have_a_ragged_row_tile():
  """conv3d_wgrad_ts_kernel: TS_SLOTS workgroups per temporal tap, workgroup `slot` takes row tiles slot, slot + 85,
  ... of frames x ceil(Ho / TY).  The small cases are one tile per frame and fewer than 85; the two walk cases have
  more, and a last row tile that is ragged."""
  for c in FC.cases("ts"):
    ty = FC.ts_tile_rows(c.layer, c.H, c.W)
    ntiles = c.B * c.T * ((c.H + ty - 1) // ty)
    if c.B * c.T == 49:
      assert ntiles == 98 > FC.TS_SLOTS and c.H % ty != 0 and c.H > ty, (c.name, ty)
    else:
      assert ntiles <= 6 and ty == c.H, (c.name, ty)
  assert FC.ts_tile_rows(FC.L2, 14, 10) == 12 and FC.ts_tile_rows(FC.L3, 20, 6) == 16
  # the split-pixel kernel: one 128-pixel stage per workgroup in the small cases, two in the 49-frame ones
  for c in FC.cases("split"):
    assert FC.split_stages(c.layer, c.B * c.T, c.H, c.W) == (2 if c.B * c.T == 49 else 1), c.name


# ---------------------------------------------------------------------------------------------------------------
# the reference against itself
# ---------------------------------------------------------------------------------------------------------------
def test_autograd_weight_gradient_equals_a_direct_sum():
  g = FC.generator("einsum")
  for layer, H, W in ((FC.L1, 7, 9), (FC.L3, 4, 5)):
    B, T = 2, 3
    (kt, kh, kw), s, (pt, ph, pw) = layer.k, layer.stride, layer.pad
    ho, wo = FC.out_hw(layer, H, W)
    x = FC.ternary((B, T, H, W, layer.cin), g)
    dz = FC.ternary((B, T, ho, wo, layer.cout), g)
    got = FC.conv_wgrad(x, dz, (layer.cout, layer.cin) + layer.k, s, layer.pad)
    xp = torch.zeros(B, T + 2 * pt, H + 2 * ph + s, W + 2 * pw + s, layer.cin, dtype=torch.float64)
    xp[:, pt:pt + T, ph:ph + H, pw:pw + W] = x
    want = torch.zeros_like(got)
    for a in range(kt):
      for b in range(kh):
        for c in range(kw):
          patch = xp[:, a:a + T, b:b + s * ho:s, c:c + s * wo:s]
          want[:, :, a, b, c] = torch.einsum("bthwn,bthwc->nc", dz, patch)
    FC.compare_exact(got, want, "dW", FC.WGT_AXES)
    # the data gradient is the adjoint of the forward: <conv(x, w), dz> = <x, dgrad(dz, w)>
    w = FC.weights(layer, g)
    lhs = float((FC.conv_forward(x, w, None, False, s, layer.pad) * dz).sum())
    assert lhs == float((x * FC.conv_dgrad(dz, w, x.shape, s, layer.pad)).sum())
    assert lhs == float((w * got).sum())


@pytest.mark.parametrize("C,frames,H,W", FC.POOL_CASES)
def test_the_two_unpool_formulations_agree(C, frames, H, W):
  act, dP = FC.pool_problem(C, frames, H, W)
  pooled, code = FC.relu_pool(act)
  FC.compare_exact(pooled, FC.maxpool(act).clamp_min(0), "pooled")
  FC.compare_exact(FC.unpool_from_code(code, dP), FC.unpool_from_act(act, dP), "dZ")
  FC.compare_exact(FC.unpool_from_act(act.clamp_min(0), dP), FC.unpool_from_act(act, dP), "dZ after ReLU")
  # torch's own max_pool backward takes the first maximum as well
  a = act.clamp_min(0).permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
  torch.nn.functional.max_pool3d(a, (1, 2, 2)).backward(dP.permute(0, 4, 1, 2, 3))
  routed = a.grad.permute(0, 2, 3, 4, 1) * (act > 0)
  FC.compare_exact(FC.unpool_from_act(act, dP), routed, "dZ against torch")


def test_compare_exact_names_the_place():
  want = torch.zeros(2, 3, 4, 5, 8, dtype=torch.float64)
  got = want.clone()
  got[0, 0, 0, 0, 0] = -0.0
  FC.compare_exact(got, want, "signed zero")
  got[1, 2, 3, 4, 7] = 1.0
  with pytest.raises(AssertionError, match=r"1 of 960 values differ.*\n.*clip 1, frame 2, row 3, column 4, channel 7"):
    FC.compare_exact(got, want, "y")
  got[1, 2, 3, 4, 7] = float("nan")
  _rejects(got, want, "nan")
  with pytest.raises(AssertionError, match="output-channel 1, input-channel 0, kt 2, kh 0, kw 1"):
    w = torch.zeros(2, 3, 3, 5, 5)
    w[1, 0, 2, 0, 1] = 2
    FC.compare_exact(w, torch.zeros(2, 3, 3, 5, 5), "dW", FC.WGT_AXES)


# ---------------------------------------------------------------------------------------------------------------
# sensitivity: four wrong references that compare_exact must reject at every case shape where they can be built
# ---------------------------------------------------------------------------------------------------------------
def _drop_one_product_in_the_last_column(p, op):
  """One (tap, contraction channel) product left out for the last output column: the centre tap in time and height
  (inside the clip and the frame at every shape), the tap whose input column the last output column still reads."""
  L = p.case.layer
  (kt, kh, kw), s, (pt, ph, pw) = L.k, L.stride, L.pad
  if op == "fwd":     # y[b,t,r,wo-1,n] -= x[b,t,r*s,(wo-1)*s-pw,c] * w[n,c,pt,ph,0]
    c = L.cin - 1
    xs = p.x[:, :, 0:s * p.ho:s, (p.wo - 1) * s - pw, c]
    out = p.z.clone()
    out[:, :, :, -1, :] -= xs.unsqueeze(-1) * p.w[:, c, pt, ph, 0]
    return out, p.z
  if op == "dgrad":   # stride 1: dx[b,t,r,W-1,c] -= dz[b,t,r,W-1,n] * w[n,c,pt,ph,pw]
    n = L.cout - 1
    out = p.dx.clone()
    out[:, :, :, -1, :] -= p.dz[:, :, :, -1, n].unsqueeze(-1) * p.w[n, :, pt, ph, pw]
    return out, p.dx
  c = L.cin - 1       # dW[n,c,pt,ph,0] -= sum_{b,t,r} dz[b,t,r,wo-1,n] * x[b,t,r*s,(wo-1)*s-pw,c]
  xs = p.x[:, :, 0:s * p.ho:s, (p.wo - 1) * s - pw, c]
  out = p.dw.clone()
  out[:, c, pt, ph, 0] -= torch.einsum("btrn,btr->n", p.dz[:, :, :, -1, :], xs)
  return out, p.dw


def _concatenate_the_clips(p, op):
  """All clips run as one: temporal taps leak across the clip boundaries."""
  c = p.case
  if c.B < 2:
    return None
  one = lambda a: a.reshape((1, c.B * c.T) + tuple(a.shape[2:]))
  if op == "fwd":
    return p._conv(one(p.x), p.w).reshape(p.z.shape), p.z
  if op == "dgrad":
    return FC.conv_dgrad(one(p.dz), p.w, one(p.x).shape, c.layer.stride, c.layer.pad).reshape(p.dx.shape), p.dx
  return p._wgrad(one(p.x), one(p.dz)), p.dw


def _double_the_last_frame(p, op):
  """The last frame's contribution counted twice (the last two frames of the last clip hold all it reaches)."""
  c = p.case
  nt = min(c.T, 2)
  src = (p.dz if op in ("dgrad", "wgrad") else p.x)[-1:, -nt:].clone()
  src[:, :-1] = 0
  if op == "fwd":
    out = p.z.clone()
    out[-1:, -nt:] += p._conv(src, p.w)
    return out, p.z
  if op == "dgrad":
    out = p.dx.clone()
    out[-1:, -nt:] += FC.conv_dgrad(src, p.w, p.x[-1:, -nt:].shape, c.layer.stride, c.layer.pad)
    return out, p.dx
  return p.dw + p._wgrad(p.x[-1:, -nt:], src), p.dw


def _pool_by_the_last_maximum(p, op):
  """Ties broken towards the last maximum instead of the first."""
  if "fwd_pooled" not in p.case.ops:
    return None   # codes drawn at random: there is no activation to tie
  act = p.z + p.bias
  if op == "fwd_pooled":
    return FC.relu_pool(act, first=False)[1], p.pooled_code[1]
  dz = FC.unpool_from_act(act, p.dP, first=False)
  if op == "dgrad_pooled":
    return p._dgrad(dz, p.w), p.dx_pooled
  return p._wgrad(p.x, dz), p.dw_pooled


@pytest.mark.parametrize("name", NAMES)
def test_compare_exact_rejects_the_wrong_references(name):
  p = FC.problem(name)
  built = 0
  for op in p.case.ops:
    if op.endswith("_pooled"):
      mutations = (_pool_by_the_last_maximum,)
    else:
      mutations = (_drop_one_product_in_the_last_column, _concatenate_the_clips, _double_the_last_frame)
    for mutate in mutations:
      pair = mutate(p, op)
      if pair is None:
        continue
      _rejects(pair[0], pair[1], "%s %s" % (op, mutate.__name__))
      built += 1
  assert built >= 2


def test_the_dropped_product_is_the_one_it_says():
  """_drop_one_product_in_the_last_column against the same operation with that weight entry zeroed."""
  p = FC.Problem(FC.Case("drop-check", "check", FC.L2, 2, 2, 4, 6, ("fwd", "dgrad", "wgrad"), 0.5))
  L = p.case.layer
  pt, ph, pw = L.pad
  w0 = p.w.clone()
  w0[:, L.cin - 1, pt, ph, 0] = 0
  want = p.z.clone()
  want[:, :, :, -1] = p._conv(p.x, w0)[:, :, :, -1]
  FC.compare_exact(_drop_one_product_in_the_last_column(p, "fwd")[0], want, "fwd")
  w0 = p.w.clone()
  w0[L.cout - 1, :, pt, ph, pw] = 0
  want = p.dx.clone()
  want[:, :, :, -1] = p._dgrad(p.dz, w0)[:, :, :, -1]
  FC.compare_exact(_drop_one_product_in_the_last_column(p, "dgrad")[0], want, "dgrad")
  dz0 = p.dz.clone()
  dz0[:, :, :, -1] = 0
  want = p.dw.clone()
  want[:, L.cin - 1, pt, ph, 0] = p._wgrad(p.x, dz0)[:, L.cin - 1, pt, ph, 0]
  FC.compare_exact(_drop_one_product_in_the_last_column(p, "wgrad")[0], want, "wgrad", FC.WGT_AXES)
