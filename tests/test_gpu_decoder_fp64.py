"""The attention decoder loop against float64, branch by branch (lr_decoder.hip, lr_decoder_dev.h through lr_decoder_forward
/ lr_decoder_backward[_parts]; the cases, the reference, the sampler's rule and the ABI helper are
tests/decoder_loop_cases.py, held to what they claim by tests/test_decoder_loop_cases_cpu.py).

Part 1: every element of log_probs, h_n, c_n, d_enc, dh0, dc0 and every parameter gradient of every case on the path it
names, and every GRU / LSTM case once more on the step kernels (lr_rnn_debug_disable_cluster), with NaN-filled outputs and
0xFF-filled reserve / workspace.  Part 2: the multinomial draw of every (sample, step) row against hash_uniform and the
device's own log_probs.  Part 3: bit-exact properties of the entry points (torch.equal between two device runs).

No bound here was tuned to a device result.  Exact fp32 paths are held by hold()'s rule (test_gpu_transformer_fp64.py):
element-wise, relative to the float64 tensor's largest entry, 4 x the error the float32 CPU loop makes on the same case,
never less than 4 ulp of fp32.  The one-launch recurrence (every tensor downstream of it) and the split-bf16 weight
gradients of a wide case on the step kernels get the project's own figures ADDED to that bound
(decoder_loop_cases.allowance): 1e-4 of the largest entry element-wise and 5e-5 in relative norm.  log_probs is held in two
column groups (live classes, masked classes); the shift-invariant score biases on the scale of their sibling weight
gradient.

What the first run of these cases showed about the dispatch: the loop's BACKWARD takes the one-launch recurrence wherever
the shape has one, whatever the teacher-forcing pattern (lr_decoder_backward_parts asks only `w.xch_bytes`; the forward
also asks that every step after the first be teacher forced).  So the three GRU / LSTM cases with sampled-input steps run
their forward on the step kernels and their backward on a cluster: their forward tensors are held exactly, their backward
tensors with the one-launch allowance (dh0 came out at 1.4e-6 .. 3.2e-6 there, 2.2 x the exact bound and 0.03 of the
allowed one — the same figure as the all-teacher-forced cluster cases), and their hooked twins hold the step kernels'
backward exactly.  The table's `bwd` column and the CPU test's restatement say so.

Measured on the MI355X: the device's element-wise error relative to the largest entry, its range over every tensor of the
path, then the tensor closest to its bound as (CPU fp32 figure, bound, device figure), then the worst relative norm against
its bound.  No bug came out of these cases: every tensor sits inside its bound, the exact ones at 0.55 of it at the most.
  step kernels both ways (RNN)     6.2e-8 .. 2.6e-7  step_rnn20_dot h_n              (9.79e-8, 4.77e-7, 1.41e-7)
  step kernels, hooked (11 cases)  0 .. 1.8e-6       step_gru24_general_l3 d_w_ih2   (1.56e-7, 6.25e-7, 3.41e-7)
    ... their fgemm gradients      4.4e-6 .. 7.6e-6  one_lstm384_general d_w_hh      (1.64e-7, 1.01e-4, 7.59e-6)   norm 4.2e-6 of 5.1e-5
  steps forward, cluster backward  2.3e-8 .. 3.2e-6  forward: step_gru24_general_l3 log_probs live (9.81e-8, 4.77e-7, 1.75e-7)
                                                     backward: step_lstm36_concat_l2_drop dh0 (5.08e-7, 1.02e-4, 3.23e-6)   norm 3.5e-6 of 5.2e-5
  clusters of 32-unit members      0 .. 9.7e-6       one_lstm384_general d_w_hh      (1.64e-7, 1.01e-4, 9.71e-6)   norm 4.6e-6 of 5.1e-5
  clusters of 16-unit members      0 .. 6.7e-6       one_gru900_none_v1024 d_w_hh    (3.93e-7, 1.02e-4, 6.68e-6)   norm 4.1e-6 of 5.1e-5 (one_lstm800_concat dh0)
  192-CU grid                      6.5e-8 .. 6.9e-6  one_lstm1156_dot d_w_hh         (5.94e-7, 1.02e-4, 6.94e-6)   norm 4.2e-6 of 5.2e-5
  (0: d_enc of attention none, and tensors that came out as the float64 result rounded.)
The score bias of the bias -25 case (a real gradient: 1.3e-4, 1.3e-3 of its sibling's largest entry, where float64 says 1e-12
for the other cases): (1.28e-7, 1.01e-4, 1.27e-7) on the
cluster, (1.28e-7, 5.11e-7, 3.74e-8) on the step kernels — inside the ordinary bound.  The shift-invariant biases elsewhere,
on their sibling's scale: 2.3e-8 .. 1.8e-6 against CPU figures of 3.4e-8 .. 4.9e-6.
The draws: 0 of 300 rows were decided by the 1e-5 slack.
Broken on purpose on a scratch copy, each of these made part 1 or part 2 fail: `+ 1e-13f` dropped in dec_attn_softmax_kernel
(part 1, the bias -25 case, both paths); the sampler's carry between 64-class chunks assigned instead of added (part 2,
V = 1024); u taken from step 0 for every step (part 2, 11 cases); the two halves of concat_layer.weight swapped in the
forward (part 1, every case with attention)."""
import pytest
import torch

from tests import decoder_loop_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _lib():
  from lipreading_amd import _C
  return _C.lib()


def run(name, dev, **kw):
  """C.run_loop between the checks that belong to the path: a one-launch case has its kernel on this device, the fault
  words start clear and read 0 afterwards (no member of a cluster timed out); with steps=True the hook is what the status
  query reports while it is set."""
  case, L = C.CASES[name], _lib()
  one = C.one_launch_bwd(case) and not kw.get("steps")
  shape = (C.mode_of(case), case.B, case.L, case.Hd, case.Hd, 1)
  if one:
    assert L.lr_rnn_one_launch_status(*shape) == 0
    L.lr_rnn_pair_errors()
  elif C.one_launch_bwd(case):
    L.lr_rnn_debug_disable_cluster(1)
    try:
      assert L.lr_rnn_one_launch_status(*shape) == 3
    finally:
      L.lr_rnn_debug_disable_cluster(0)
  got = C.run_loop(name, dev, **kw)
  if one:
    assert L.lr_rnn_pair_errors() == 0
  assert L.lr_rnn_one_launch_status(*shape) != 3      # the hook is restored
  return got


@pytest.fixture(scope="module")
def baseline(dev):
  """The plain run of a case (poisoned buffers, every pointer given, accumulate = 0): once per (case, path), shared."""
  runs = {}

  def get(name, steps=False):
    if (name, steps) not in runs:
      runs[name, steps] = run(name, dev, steps=steps)
    return runs[name, steps]
  return get


def where(got, want64, scale64, bound):
  """Where the elements outside the bound sit: up to 8 indices, for the assertion's message."""
  scale = max(float(scale64.abs().max()), 1e-30)
  bad = ((got.double() - want64).abs() / scale > bound).nonzero()
  return "%d of %d elements, first at %s" % (len(bad), want64.numel(), bad[:8].tolist())


def path_of(case, steps):
  if steps or not C.one_launch_bwd(case):
    return "steps" + (" (hooked)" if steps else "")
  return case.recur if C.one_launch(case) else "steps fwd, %s bwd" % case.bwd


def hold_tensor(case, key, label, got, want64, cpu32, scale64, steps, bad):
  """Prints (CPU fp32 figure, bound, device figure) element-wise and in relative norm; appends what is outside to `bad`."""
  cpu_err, _ = C.figures(cpu32, want64, scale64)
  elem, norm = C.bounds(case, key, cpu_err, hooked=steps)
  err, nerr = C.figures(got, want64, scale64)
  ok = bool(torch.isfinite(got).all()) and got.shape == want64.shape and err <= elem and (norm is None or nerr <= norm)
  print("%-28s %-26s %-18s cpu fp32 %.2e  bound %.2e  device %.2e   norm: bound %s  device %.2e%s" % (
      case.name, path_of(case, steps), label, cpu_err, elem, err, "none   " if norm is None else "%.2e" % norm, nerr,
      "" if ok else "  <-- MISSES"))
  if not ok:
    bad.append((label, err, elem, nerr, norm, where(got, want64, scale64, elem)))


def hold_run(name, got, steps):
  case = C.CASES[name]
  want64, cpu32 = C.reference(name, got["sampled"] if C.needs_draws(case) else None)
  bad = []
  for k in C.tensor_names(case):
    assert k in got, k
    for (label, g, w, s), (_, cpu, _, _) in zip(C.pieces(case, k, got, want64), C.pieces(case, k, cpu32, want64)):
      hold_tensor(case, k, label, g, w, cpu, s, steps, bad)
  assert not bad, (name, path_of(case, steps), bad)


def same_bits(a, b, keys=None):
  for k in (keys if keys is not None else [k for k in a if k != "second"]):
    assert not torch.isnan(a[k].float()).any(), k
    assert torch.equal(a[k], b[k]), k


# ---- part 1: every element against float64 ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.CASES))
def test_loop_matches_float64(dev, baseline, name):
  """Every tensor the ABI returns, on the path the case names.  A case with sampled-input steps has the device's own draws
  replayed through the reference (part 2 holds the draws themselves)."""
  hold_run(name, baseline(name), False)


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if C.step_twin(c)])
def test_loop_on_the_step_kernels_matches_float64(dev, baseline, name):
  """The same case through lr_rnn_step_fwd / _bwd, forward and backward: exact fp32 but for a wide case's split-bf16 weight
  gradients.  Every GRU / LSTM case has such a twin: without the hook the backward of a case with sampled-input steps is
  the cluster recurrence's too."""
  hold_run(name, baseline(name, True), True)


# ---- part 2: the draw -----------------------------------------------------------------------------------------------------

def check_draws(case, got, seed):
  """sampled = the first class past u * total of hash_uniform(seed, step, sample) and the run's own log_probs (cumulative
  sum in float64), either neighbour within DRAW_SLACK of a boundary; never a masked class.  -> rows that used the slack."""
  lp, s = got["log_probs"], got["sampled"]
  assert s.shape == (case.B, case.L)
  pick, lo, hi, _ = C.draws(lp, seed)
  assert bool(((s >= lo) & (s <= hi)).all()), (case.name, s.tolist(), pick.tolist())
  assert int(s.min()) >= 2 and int(s.max()) < case.V
  assert bool((torch.gather(lp, 2, s.unsqueeze(-1)).exp() > 0).all())      # a class with mass
  return int((s != pick).sum())


@pytest.mark.parametrize("name", list(C.CASES))
def test_draws_follow_the_hash_and_the_log_probs(dev, baseline, name):
  case = C.CASES[name]
  got = baseline(name)
  check_draws(case, got, case.seed)
  again = run(name, dev, forward_only=True)
  same_bits(again, got, keys=["log_probs", "sampled"] + C.state_keys(case))      # the same seed: the same draws
  other = run(name, dev, forward_only=True, seed=case.seed + 1)
  check_draws(case, other, case.seed + 1)
  if case.B * case.L >= 9:
    assert not torch.equal(other["sampled"], got["sampled"])                     # another seed: other draws


def test_draws_rarely_need_the_slack(dev, baseline):
  """A 64-term fp32 prefix sum errs by a few 1e-6: at most one row in 50 over the table may be decided by it (the float64
  reference alone needs none: test_decoder_loop_cases_cpu.py)."""
  rows = slack = 0
  for name, case in C.CASES.items():
    slack += check_draws(case, baseline(name), case.seed)
    rows += case.B * case.L
  print("draws decided by the slack: %d of %d rows" % (slack, rows))
  assert slack * 50 <= rows, (slack, rows)


# ---- part 3: properties, bit for bit --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.PROPERTY_CASES)
def test_poisoned_buffers_change_nothing(dev, baseline, name):
  """NaN outputs, 0xFF reserve and workspace (the baseline) against zero-filled ones: no NaN, the same bits."""
  same_bits(baseline(name), run(name, dev, poison=False))


@pytest.mark.parametrize("name", C.PROPERTY_CASES)
def test_enc_past_a_length_reaches_no_output(dev, baseline, name):
  """Seeded values of magnitude 1e3 in the frames of enc past each length: not one bit of any output changes."""
  same_bits(run(name, dev, enc=C.enc_with_garbage(name)), baseline(name))


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.NONE_CASE])
def test_padded_frames_get_exactly_zero_d_enc(dev, baseline, name):
  """... and with attention none d_enc is zero throughout, whatever it held before (NaN here)."""
  case, d_enc = C.CASES[name], baseline(name)["d_enc"]
  pad = ~C.valid_mask(name).expand_as(d_enc)
  assert pad.any()
  assert torch.equal(d_enc[pad], torch.zeros(int(pad.sum())))
  if case.attn == "none":
    assert torch.equal(d_enc, torch.zeros_like(d_enc))
  else:
    assert bool(d_enc[~pad].any())


@pytest.mark.parametrize("name", C.PROPERTY_CASES)
def test_null_state_gradients_are_zero_tensors(dev, name):
  case = C.CASES[name]
  zeros = run(name, dev, zero_state_grads=True)
  same_bits(run(name, dev, null_dh=True, null_dc=True), zeros)
  if case.cell == "LSTM":
    same_bits(run(name, dev, zero_state_grads=True, null_dc=True), zeros)


@pytest.mark.parametrize("name", C.PROPERTY_CASES)
def test_null_h_n_leaves_everything_else_unchanged(dev, baseline, name):
  case = C.CASES[name]
  got = run(name, dev, null_hn=True)
  assert "h_n" not in got and "c_n" not in got
  same_bits(got, baseline(name))


@pytest.mark.parametrize("name", C.PROPERTY_CASES)
def test_backward_parts_1_then_2_equal_parts_3(dev, baseline, name):
  """lr_decoder_backward_parts: the data half, then the weight half from what it left in the SAME workspace; and as the
  product calls them: adding to gradients that are already there."""
  halves, whole = run(name, dev, parts=(1, 2)), run(name, dev, parts=(3,))
  same_bits(halves, whole)
  same_bits(whole, baseline(name))                  # lr_decoder_backward
  same_bits(run(name, dev, parts=(1, 2), accumulate=True), run(name, dev, accumulate=True))


@pytest.mark.parametrize("parts", [1, 2])
def test_backward_parts_of_two_layers_are_refused(dev, parts):
  from lipreading_amd import _C
  assert C.CASES[C.NONE_CASE].layers == 2
  assert run(C.NONE_CASE, dev, parts=(parts,), raise_on_error=False) == {"status": _C.LR_ERR_INVALID_ARG}


@pytest.mark.parametrize("name", C.PROPERTY_CASES)
def test_second_backward_over_one_reserve(dev, baseline, name):
  """retain_graph: the second lr_decoder_backward over a forward's reserve must give the first one's bits."""
  case = C.CASES[name]
  got = run(name, dev, backwards=2)
  same_bits(got, baseline(name))
  same_bits(got["second"], baseline(name), keys=list(got["second"]))


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.NONE_CASE])
def test_accumulate_adds_to_the_prefill(dev, baseline, name):
  """accumulate = 1 on seeded gradients: pre-fill + gradient within the case's bound; log_probs, d_enc, dh0 as without."""
  case, inp = C.CASES[name], C.inputs(name)
  got = run(name, dev, accumulate=True)
  same_bits(got, baseline(name), keys=["log_probs", "sampled", "d_enc", "dh0"] + C.state_keys(case) +
            (["dc0"] if case.cell == "LSTM" else []))
  want64, cpu32 = C.reference(name, got["sampled"] if C.needs_draws(case) else None)
  bad = []
  for k in C.grad_keys(case):
    want = inp.prefill[k].double() + want64[k]
    hold_tensor(case, k, k + " +=", got[k], want, inp.prefill[k] + cpu32[k], want, False, bad)
  assert not bad, (name, bad)
