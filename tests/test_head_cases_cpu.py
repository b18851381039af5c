"""tests/head_cases.py is what tests/test_gpu_head_fp64.py takes it for (no GPU): every path plan() names has its cases and
every case sits on the path it names, every edge of the dispatch is in the tables, the float64 references are torch's
autograd and torch's nll_loss in float64, the float32 yardsticks are finite and tight enough for 4 x their error to mean
something, the saturated cases saturate — and a reference that is deliberately wrong is caught by the bound the GPU test
applies.

The float32 CPU formula's error against float64 per tensor, relative to the tensor's largest entry, measured over the
tables on an Intel host: forward 0 (one class) .. 2.4e-7 on the unmasked columns, 6.5e-8 .. 3.1e-7 on the masked ones,
4.3e-7 .. 5.7e-7 where every class is masked (every logit is rounded near 103, against a row of entries near log C);
backward 0 (one class) .. 6.9e-7 (dhidden of the largest case); the three products 2.4e-8 .. 5.7e-7; the loss and its
sum 0 .. 1.2e-7, its gradient at most one rounding (4e-8).  The 2e-6 asked of them below leaves a factor of three.  The
figures belong to the host's BLAS: the GPU test takes the yardstick of the host it runs on."""
import pytest
import torch
import torch.nn.functional as F

from tests import head_cases as C

TIGHT = 2e-6      # what keeps 4 x the figure a bound that a wrong element cannot hide under


# ---- the tables ---------------------------------------------------------------------------------------------------------

def test_every_path_has_its_cases_and_every_case_sits_on_its_path():
  for table in (C.FWD_CASES, C.BWD_CASES, C.NLL_CASES):
    for name, case in table.items():
      assert case.name == name and case.why
      assert C.plan(case) == case.path, name
  count = lambda table, path: sum(1 for c in table.values() if C.plan(c) == path)
  for path in ("fused", "fallback"):
    assert count(C.FWD_CASES, path) >= 3
  for path in ("fused", "chain"):
    assert count(C.BWD_CASES, path) >= 3
  live = {n: c for n, c in C.NLL_CASES.items() if c.pattern != "all"}
  for path in ("vec4", "scalar"):
    assert count(live, path) >= 3
  # the second backward call of the GPU test: one float off a 16-byte boundary takes the scalar kernel at V % 4 == 0
  assert all(C.plan(c, offset=1) == "scalar" for c in C.NLL_CASES.values())
  assert C.plan(C.REFUSED) == "fused" and C.REFUSED.C == C.MAX_CLASSES + 1
  assert 16 <= len(C.FWD_CASES) <= 20 and 12 <= len(C.BWD_CASES) <= 13


def test_forward_edges_are_in_the_table():
  fused = [c for c in C.FWD_CASES.values() if c.path == "fused"]
  fallback = [c for c in C.FWD_CASES.values() if c.path == "fallback"]
  # steps = K / 16 on every branch of the pipelined loop: 1, 3, 4, 5 around the group of four, then whole groups and a tail
  assert {16, 48, 64, 80, 144, 512} <= {c.K for c in fused}
  assert {1, 3, 4, 5, 9, 32} <= {c.K // 16 for c in fused}
  assert {1, 15, 16, 17, 33} <= {c.R for c in fused}
  assert {1, 15, 16, 17, 65, 128, 129, 255, 256} <= {c.C for c in fused}
  assert all(c.K % 16 == 0 and not c.off_hidden and not c.off_w for c in fused)
  assert {1, 7, 40, 72} <= {c.K for c in fallback if c.K % 16}
  assert any(c.K == 64 and c.off_hidden == 1 and not c.off_w for c in fallback)
  assert any(c.K == 64 and c.off_w == 1 and not c.off_hidden for c in fallback)
  for path in (fused, fallback):
    assert {"two", "all"} <= {c.mask for c in path}
  assert {"two", "none", "all", "frac"} == {c.mask for c in C.FWD_CASES.values()}
  assert sum(1 for c in C.FWD_CASES.values() if c.saturated) == 1
  # the misaligned copies run the data of a fused case
  for a, b in C.TWINS:
    ca, cb = C.FWD_CASES[a], C.FWD_CASES[b]
    assert (ca.path, cb.path) == ("fused", "fallback") and cb.data == a
    assert C.fwd_inputs(ca) is C.fwd_inputs(cb)
  assert {b for _, b in C.TWINS} == {c.name for c in C.FWD_CASES.values() if c.off_hidden or c.off_w}
  # the largest case
  assert max(c.R * c.K * c.C for c in C.FWD_CASES.values()) == 50 * 520 * 256
  assert all(c.C <= C.MAX_CLASSES for c in C.FWD_CASES.values())


def test_backward_edges_are_in_the_table():
  fused = [c for c in C.BWD_CASES.values() if c.path == "fused"]
  chain = [c for c in C.BWD_CASES.values() if c.path == "chain"]
  assert {1, 16, 17, 50} <= {c.R for c in fused}
  assert {1, 63, 64, 65, 200} <= {c.K for c in fused}
  assert {1, 7, 8, 9, 65, 128} <= {c.C for c in fused}
  assert {129, 256} <= {c.C for c in chain}
  assert [c.name for c in C.BWD_CASES.values() if c.saturated] == ["r17_k64_c65_sat"]
  assert max(c.R * c.K * c.C for c in C.BWD_CASES.values()) == 50 * 520 * 256
  # slab rows Cp = ceil(C / 8) . 8 both equal to C and past it; more slabs than the reduce kernel's four thread rows and fewer
  assert any(c.C % 8 == 0 for c in fused) and any(c.C % 8 for c in fused)
  assert {(c.R + 15) // 16 for c in fused} >= {1, 2, 4}


def test_token_loss_edges_are_in_the_table():
  cases = list(C.NLL_CASES.values())
  assert {1, 3, 4, 65, 68} <= {c.V for c in cases}
  assert {1, 1023, 1024, 1025, 3000} <= {c.B * c.L for c in cases}
  assert {"tail", "rows", "all"} <= {c.pattern for c in cases}
  for path in ("vec4", "scalar"):
    assert any(c.pattern == "all" and c.path == path for c in cases)
    # more than 1024 workgroups' worth: the grid-stride loop of either backward kernel takes a second turn
    per_thread = 4 if path == "vec4" else 1
    assert any(c.path == path and c.B * c.L * c.V // per_thread > 1024 * 256 for c in cases)
  for c in cases:
    inp = C.nll_inputs(c.name)
    assert inp.labels.shape == (c.B, c.L) and inp.labels.stride() == (c.stride, 1) and c.stride > c.L
    assert inp.labels.data_ptr() == inp.wide.data_ptr() + 8      # the view starts one label into the row
    on = inp.labels != c.pad
    assert ((inp.labels >= 0) & (inp.labels < c.V))[on].all()
    assert (inp.wide != c.pad).all() or c.pattern != "none"
    if c.pattern == "all":
      assert not on.any()
    if c.pattern == "rows":
      assert (~on).all(dim=1).any() and on.all(dim=1).sum() >= 1
    if c.pattern in ("tail", "rows"):
      assert (~on[:, -1]).any() and on[:, 0].any() and on[-1].all()
    # what sits around the labels in the wide tensor would change the loss if it were read as one
    if c.V > 1:
      assert (inp.wide[:, 0] != c.pad).all() and (inp.wide[:, 1 + c.L:] != c.pad).all()


# ---- the references -----------------------------------------------------------------------------------------------------

def test_the_mask_term_is_the_smallest_subnormal():
  assert C.TINY == float(torch.tensor(1e-45, dtype=torch.float32)) > 0
  assert abs(float(torch.log(torch.tensor(C.TINY, dtype=torch.float64))) - C.LOG_TINY) < 1e-13
  # float32 on this host keeps the subnormal too
  got = float(torch.log(torch.zeros(1) + torch.tensor(C.TINY, dtype=torch.float32)))
  assert abs(got - C.LOG_TINY) < 1e-5


@pytest.mark.parametrize("name", list(C.FWD_CASES))
def test_forward_reference_and_yardstick(name):
  case, inp = C.FWD_CASES[name], C.fwd_inputs(C.FWD_CASES[name])
  want64, cpu32 = C.fwd_reference(name)
  assert want64.dtype == torch.float64 and cpu32.dtype == torch.float32 and want64.shape == (case.R, case.C)
  assert torch.isfinite(want64).all() and torch.isfinite(cpu32).all()
  # the shared inputs stay plain data, whatever took a gradient through them (autograd_formula works on copies)
  before = [t.clone() for t in inp]
  auto = C.autograd_formula(inp, torch.float32)
  assert not any(t.requires_grad for t in inp) and all(torch.equal(a, b) for a, b in zip(before, inp))
  assert torch.equal(auto["lp"], cpu32)
  # rows of log-probabilities
  assert float((want64.exp().sum(dim=1) - 1).abs().max()) < 1e-12
  masked = C.masked_columns(case)
  assert int(masked.sum()) == {"two": 2, "all": case.C, "none": 0, "frac": 0}[case.mask]
  if case.mask == "two":
    assert float(want64[:, masked].max()) < -90
    assert not (case.saturated and masked[C.SAT_CLASS])
  if case.mask == "frac":
    assert float(inp.mask.min()) > 0 and float(inp.mask.max()) < 1
  for what, cols in (("unmasked", ~masked), ("masked", masked)):
    if cols.any():
      err = C.figures(cpu32[:, cols], want64[:, cols])
      print("%-26s %-9s float32 CPU against float64 %.2e  bound %.2e" % (name, what, err, C.bound(err)))
      assert err <= TIGHT, (what, err)
      if case.C == 1:
        assert err == 0 and C.bound(err) == 4 * C.ULP


@pytest.mark.parametrize("name", list(C.BWD_CASES))
def test_backward_reference_is_autograd_in_float64(name):
  """The formula of head_cases (the float32 log_probs as data) against torch.autograd in float64 on
  log_softmax(hidden W^T + b + log(mask + 2^-149)), g as the upstream gradient — given autograd's OWN float64 log_probs,
  so that the two can agree to 1e-12."""
  case = C.BWD_CASES[name]
  inp, lp32 = C.bwd_inputs(case)
  h = inp.hidden.double().requires_grad_(True)
  W = inp.W.double().requires_grad_(True)
  b = inp.bias.double().requires_grad_(True)
  logits = h @ W.t() + b + torch.log(inp.mask.double() + C.TINY)
  logits.retain_grad()
  lp = torch.log_softmax(logits, dim=1)
  lp.backward(inp.g.double())
  assert float((lp.detach() - C.forward_formula(inp.hidden, inp.W, inp.bias, inp.mask, torch.float64)).abs().max()) <= 1e-12 * \
      max(1.0, float(lp.detach().abs().max()))
  got = C.backward_formula(inp.g, lp.detach(), inp.hidden, inp.W, torch.float64)
  for key, auto in (("dlogits", logits.grad), ("dhidden", h.grad), ("dW", W.grad), ("dbias", b.grad)):
    assert got[key].shape == auto.shape
    assert C.figures(got[key], auto) <= 1e-12, key
  # the data the kernel is given is the float32 forward of the same inputs
  assert lp32.dtype == torch.float32 and float((lp32.double() - lp.detach()).abs().max()) <= 1e-5 * float(lp.detach().abs().max())


@pytest.mark.parametrize("name", list(C.BWD_CASES))
def test_backward_yardstick(name):
  case = C.BWD_CASES[name]
  want64, cpu32 = C.bwd_reference(name)
  shapes = {"dlogits": (case.R, case.C), "dhidden": (case.R, case.K), "dW": (case.C, case.K), "dbias": (case.C,)}
  for key in C.BWD_KEYS:
    assert want64[key].dtype == torch.float64 and cpu32[key].dtype == torch.float32
    assert want64[key].shape == cpu32[key].shape == shapes[key]
    assert torch.isfinite(want64[key]).all() and torch.isfinite(cpu32[key]).all()
    err = C.figures(cpu32[key], want64[key])
    print("%-18s %-8s float32 CPU against float64 %.2e  bound %.2e" % (name, key, err, C.bound(err)))
    assert err <= TIGHT, (key, err)
    if case.C == 1:
      assert err == 0 and not want64[key].any()      # g - exp(0) . g


def test_saturated_cases_saturate():
  """Forward: in every row one class leads by more than 100 nats and exp(second - first) is 0 in float32.  Backward: lp
  is 0 at that class and below -100 elsewhere, the row sum of g is large, and the dominant entry of dlogits is the
  difference of two numbers of that size."""
  case = [c for c in C.FWD_CASES.values() if c.saturated][0]
  inp = C.fwd_inputs(case)
  logits = inp.hidden.double() @ inp.W.double().t() + inp.bias.double() + torch.log(inp.mask.double() + C.TINY)
  top = logits.topk(2, dim=1).values
  assert (logits.argmax(dim=1) == C.SAT_CLASS).all()
  assert float((top[:, 0] - top[:, 1]).min()) > 100
  assert float(torch.exp((top[:, 1] - top[:, 0]).float()).max()) == 0
  want64, _ = C.fwd_reference(case.name)
  assert float(want64[:, C.SAT_CLASS].abs().max()) == 0
  bcase = C.BWD_CASES["r17_k64_c65_sat"]
  binp, lp = C.bwd_inputs(bcase)
  others = torch.ones(bcase.C, dtype=torch.bool)
  others[C.SAT_CLASS] = False
  assert float(lp[:, C.SAT_CLASS].abs().max()) == 0 and float(lp[:, others].max()) < -100
  rowsum = binp.g.double().sum(dim=1)
  assert float(rowsum.min()) > 150
  want64, _ = C.bwd_reference(bcase.name)
  assert float((want64["dlogits"][:, C.SAT_CLASS] - (binp.g[:, C.SAT_CLASS].double() - rowsum)).abs().max()) == 0


@pytest.mark.parametrize("name", list(C.NLL_CASES))
def test_token_loss_reference_is_nll_loss_in_float64(name):
  c, inp = C.NLL_CASES[name], C.nll_inputs(name)
  want64, cpu32 = C.nll_reference(name)
  on = inp.labels != c.pad
  assert want64["count"] == cpu32["count"] == int(on.sum())
  lp = inp.lp.double().requires_grad_(True)
  target = inp.labels.reshape(-1)
  total = F.nll_loss(lp.reshape(-1, c.V), target, ignore_index=c.pad, reduction="sum")
  assert c.pattern == "all" or int(on.sum()) > 0
  if c.pattern == "all":
    assert want64["count"] == 0 and float(want64["sum"]) == 0 and torch.isnan(want64["loss"])
    return
  loss = total / int(on.sum())
  (loss * float(torch.tensor(C.NLL_G, dtype=torch.float32))).backward()
  assert abs(float(want64["sum"]) - float(total.detach())) <= 1e-12 * abs(float(total.detach()))
  assert abs(float(want64["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
  assert C.figures(want64["d_lp"], lp.grad) <= 1e-12
  # the float32 restatement: nll_loss in float32
  total32 = F.nll_loss(inp.lp.reshape(-1, c.V), target, ignore_index=c.pad, reduction="sum")
  for key, ref32 in (("sum", total32), ("loss", total32 / int(on.sum()))):
    err = abs(float(cpu32[key]) - float(want64[key])) / abs(float(want64[key]))
    err_torch = abs(float(ref32) - float(want64[key])) / abs(float(want64[key]))
    print("%-12s %-5s float32 CPU against float64 %.2e (F.nll_loss in float32: %.2e)  bound %.2e"
          % (name, key, err, err_torch, C.bound(err)))
    assert err <= TIGHT and err_torch <= TIGHT
  err = C.figures(cpu32["d_lp"], want64["d_lp"])
  assert torch.isfinite(cpu32["d_lp"]).all() and err <= C.ULP      # one rounding of -g / count


@pytest.mark.parametrize("name", [s[0] for s in C.gemm_shapes()])
def test_product_yardstick(name):
  want64, cpu32 = C.gemm_formula(name, torch.float64), C.gemm_formula(name, torch.float32)
  assert torch.isfinite(want64).all() and torch.isfinite(cpu32).all()
  err = C.figures(cpu32, want64)
  print("%-26s float32 CPU against float64 %.2e  bound %.2e" % (name, err, C.bound(err)))
  assert err <= TIGHT


def test_products_are_the_heads():
  shapes = C.gemm_shapes()
  kinds = lambda prefix: [s for s in shapes if s[0].startswith(prefix)]
  assert len(kinds("nt_bias_")) >= 5 and len(kinds("nn_")) == len(kinds("tn_beta1_")) == 3
  assert all((s[1], s[2], s[6], s[7]) == (0, 1, True, 0.0) for s in kinds("nt_bias_"))
  assert all((s[1], s[2], s[6], s[7]) == (0, 0, False, 0.0) for s in kinds("nn_"))
  assert all((s[1], s[2], s[6], s[7]) == (1, 0, False, 1.0) for s in kinds("tn_beta1_"))
  assert len({s[0] for s in shapes}) == len(shapes)
  pads = {p for p, _ in C.GEMM_LAYOUTS}
  assert all(p > 0 for p in pads) and any(p % 4 == 0 for p in pads) and any(p % 4 for p in pads)
  assert {o for _, o in C.GEMM_LAYOUTS} == {0, 1}


# ---- a wrong reference is caught ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, c in C.FWD_CASES.items() if c.mask in ("two", "frac") and c.C >= 5])
def test_a_wrong_forward_is_caught(name):
  """The float32 CPU result (a stand-in for a correct device) against a float64 reference that is NOT the head — the mask
  term taken as log(mask + 1e-30), what a device that flushed the subnormal to something else might give; one weight
  column dropped, what a K loop that lost its last step gives: both fall outside the GPU test's bound."""
  case, inp = C.FWD_CASES[name], C.fwd_inputs(C.FWD_CASES[name])
  want64, cpu32 = C.fwd_reference(name)
  masked = C.masked_columns(case)
  if case.mask == "two":
    h, w, b, m = (t.double() for t in inp[:4])
    bad = torch.log_softmax(h @ w.t() + b + torch.log(m + 1e-30), dim=1)
    cpu_err = C.figures(cpu32[:, masked], want64[:, masked])
    assert C.figures(cpu32[:, masked], bad[:, masked]) > C.bound(cpu_err)
  W = inp.W.clone()
  W[:, -1] = 0
  bad = C.forward_formula(inp.hidden, W, inp.bias, inp.mask, torch.float64)
  cpu_err = C.figures(cpu32[:, ~masked], want64[:, ~masked])
  assert C.figures(cpu32[:, ~masked], bad[:, ~masked]) > C.bound(cpu_err)


@pytest.mark.parametrize("name", [n for n, c in C.BWD_CASES.items() if c.C > 1])
def test_a_wrong_backward_is_caught(name):
  """... and a backward whose last row never reached dW and dbias."""
  case = C.BWD_CASES[name]
  inp, lp = C.bwd_inputs(case)
  want64, cpu32 = C.bwd_reference(name)
  g = inp.g.clone()
  g[-1] = 0
  bad = C.backward_formula(g, lp, inp.hidden, inp.W, torch.float64)
  for key in ("dW", "dbias"):
    cpu_err = C.figures(cpu32[key], want64[key])
    assert C.figures(cpu32[key], bad[key]) > C.bound(cpu_err), key
