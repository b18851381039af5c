"""The recurrent layer's entry points against float64, path by path (lr_rnn.hip, lr_rnn_cluster.hip, lr_rnn_grid.hip
through lr_rnn_layer_forward / lr_rnn_layer_backward[_parts]; the cases, the torch.nn reference and the ABI helper are
tests/rnn_layer_cases.py, held to what they claim by tests/test_rnn_layer_cases_cpu.py).

Part 1: every element of y, h_n, c_n, dx and the parameter gradients of every case, with NaN-filled outputs and 0xFF-filled
reserve / workspace (what the product's torch.empty may hold).  Part 2: the two-call backward.  Part 3: bit-exact
properties of the entry points (torch.equal between two device runs).

No bound here was tuned to a device result.  The step kernels (no mode flags: exact fp32) are held by hold()'s rule:
element-wise, relative to the float64 tensor's largest entry, 4 x the error torch.nn's float32 CPU layer makes on the same
case, never less than 4 ulp of fp32.  LR_RNN_RECUR_SPLIT and LR_RNN_PROJ_BF16X3 get the project's own figures for those
paths ADDED to that bound (rnn_layer_cases.allowance): 1e-4 of the largest entry element-wise and 2e-5 in relative norm;
1e-2 for dx under LR_RNN_INPUT_BF16_EXACT.

Measured on the MI355X: the device's element-wise error relative to the largest entry, its range over every tensor of the
path, then the path's worst tensor as (CPU fp32 figure, bound, device figure), then the worst relative norm against its
bound.  No bug came out of these cases: every tensor sits inside its bound, the exact path at 0.65 of it at the most.
  step kernels                  0 .. 4.9e-7      lstm20_b17 db_ih0      (1.08e-7, 4.77e-7, 3.1e-7)
  step kernels, saturated       9.6e-9 .. 2.1e-7 sat_lstm_step dw_ih0   (9.72e-8, 4.77e-7, 1.69e-7)
  clusters of 32-unit members   4.6e-7 .. 1.1e-5 split_gru40 dw_hh0     (1.93e-7, 1.01e-4, 1.08e-5)   norm 5.8e-6 of 2.1e-5
  clusters of 16-unit members   5.0e-7 .. 8.1e-6 split_lstm800 dw_hh0   (2.22e-7, 1.01e-4, 8.11e-6)   norm 5.7e-6 of 2.1e-5
  192-CU grid                   2.2e-7 .. 1.3e-5 grid_lstm1156 dw_hh1   (2.61e-7, 1.01e-4, 1.35e-5)   norm 6.4e-6 of 2.1e-5
  clusters, saturated           3.3e-7 .. 6.0e-6 sat_gru_split dw_ih1   (9.46e-8, 1.00e-4, 5.97e-6)   norm 4.9e-6 of 2.1e-5
  PROJ_BF16X3                   8.7e-7 .. 9.1e-6 x3_split dw_hh0        (2.26e-7, 1.01e-4, 9.13e-6)   norm 7.0e-6 of 2.1e-5
  ... | INPUT_BF16_EXACT        3.8e-7 .. 9.2e-6 besides dx; dx: x3exact_step (1.61e-7, 1.00e-2, 2.65e-3), norm 2.6e-3 of 1e-2"""
import pytest
import torch

from tests import rnn_layer_cases as C
from tests.test_gpu_transformer_fp64 import hold

pytestmark = pytest.mark.gpu

LR_ERR_UNSUPPORTED = -4


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _lib():
  from lipreading_amd import _C
  return _C.lib()


def one_launch(case):
  return C.SPLIT in case.flags


def before(case):
  """A one-launch case: the shape has its kernel on this device, and the fault words start clear."""
  if one_launch(case):
    assert _lib().lr_rnn_one_launch_status(C.mode_of(case), *C.dims_of(case)) == 0
    _lib().lr_rnn_pair_errors()


def after(case):
  if one_launch(case):
    assert _lib().lr_rnn_pair_errors() == 0      # no member of a cluster timed out


def where(got, want64, bound):
  """Where the elements outside the bound sit: up to 8 indices, for the assertion's message."""
  scale = max(float(want64.abs().max()), 1e-30)
  bad = ((got.double() - want64).abs() / scale > bound).nonzero()
  return "%d of %d elements, first at %s" % (len(bad), want64.numel(), bad[:8].tolist())


def hold_case(case, key, got, want64, cpu32):
  """hold() on the exact path; elsewhere its bound plus the path's own figures, element-wise and in relative norm."""
  what = "%s %s" % (case.name, key)
  assert got.shape == want64.shape, what
  if C.exact(case):
    try:
      hold(what, got, want64, cpu32)
    except AssertionError as e:
      cpu_err, _ = C.figures(cpu32, want64)
      raise AssertionError("%s: %s; %s" % (what, e, where(got, want64, C.bounds(case, key, cpu_err)[0])))
    return
  cpu_err, _ = C.figures(cpu32, want64)
  elem, norm = C.bounds(case, key, cpu_err)
  err, nerr = C.figures(got, want64)
  print("%-40s cpu fp32 %.2e  bound %.2e  device %.2e   norm: bound %.2e  device %.2e" % (what, cpu_err, elem, err, norm, nerr))
  assert torch.isfinite(got).all(), what
  assert err <= elem, (what, err, elem, where(got, want64, elem))
  assert nerr <= norm, (what, nerr, norm)


def same_bits(a, b, keys=None):
  for k in (keys if keys is not None else [k for k in a if k != "second"]):
    assert not torch.isnan(a[k]).any(), k
    assert torch.equal(a[k], b[k]), k


GRAD_KEYS = ("dw_ih", "dw_hh", "db_ih", "db_hh")


def grad_keys(case):
  return ["%s%d" % (k, d) for d in range(case.D) for k in GRAD_KEYS]


@pytest.fixture(scope="module")
def baseline(dev):
  """The plain run of a case (poisoned buffers, every pointer given, accumulate = 0): once per case, shared."""
  runs = {}

  def get(name):
    if name not in runs:
      case = C.CASES[name]
      before(case)
      runs[name] = C.run_layer(name, dev)
      after(case)
    return runs[name]
  return get


# ---- part 1: every element against float64 ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.CASES))
def test_layer_matches_float64(dev, baseline, name):
  """y, h_n, c_n, dx and the four parameter gradients per direction.  The saturated cases (bias_ih +-60) at the same
  bounds: fast_sigmoid / fast_tanh go through exp2 = inf and rcp(inf) there, and every output must be finite."""
  case = C.CASES[name]
  want64, cpu32 = C.reference(name)
  got = baseline(name)
  for k in C.tensor_names(case):
    hold_case(case, k, got[k], want64[k], cpu32[k])


# ---- part 2: the backward in two calls ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.PARTS_CASES)
def test_backward_parts_1_then_2_equal_parts_3(dev, baseline, name):
  """lr_rnn_layer_backward_parts: the data half, then the weight half from the dG it left in the SAME workspace."""
  case = C.CASES[name]
  before(case)
  halves = C.run_layer(name, dev, parts=(1, 2))
  whole = C.run_layer(name, dev, parts=(3,))
  # ... and as the product calls them: adding to gradients that are already there
  halves_acc = C.run_layer(name, dev, parts=(1, 2), accumulate=True)
  whole_acc = C.run_layer(name, dev, parts=(3,), accumulate=True)
  after(case)
  same_bits(halves, whole)
  same_bits(whole, baseline(name))
  same_bits(halves_acc, whole_acc)


@pytest.mark.parametrize("name", ["gru36_odd_i", "split_gru40"])
@pytest.mark.parametrize("parts", [1, 2])
def test_backward_parts_need_the_bf16x3_projection(dev, name, parts):
  case = C.CASES[name]
  before(case)
  assert C.run_layer(name, dev, parts=(parts,), raise_on_error=False) == {"status": LR_ERR_UNSUPPORTED}
  after(case)


# ---- part 3: properties, bit for bit --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.GRID_CASE])
def test_padded_frames_are_zero_in_y_and_dx(dev, baseline, name):
  got = baseline(name)
  pad = ~C.valid_mask(name)
  assert pad.any()
  for k in ("y", "dx"):
    assert torch.equal(got[k][pad.expand_as(got[k])], torch.zeros(int(pad.sum()) * got[k].shape[-1])), k


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.GRID_CASE])
def test_x_past_a_length_reaches_no_output(dev, baseline, name):
  """Seeded values of magnitude 1e3 in the frames of x past each length: not one bit of any output changes."""
  case = C.CASES[name]
  before(case)
  got = C.run_layer(name, dev, x=C.x_with_garbage(name))
  after(case)
  same_bits(got, baseline(name))


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.GRID_CASE])
def test_poisoned_buffers_change_nothing(dev, baseline, name):
  """NaN outputs, 0xFF reserve and workspace (the baseline) against zero-filled ones: no NaN, the same bits."""
  case = C.CASES[name]
  before(case)
  clean = C.run_layer(name, dev, poison=False)
  after(case)
  same_bits(baseline(name), clean)


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.LSTM_STEP_CASE])
def test_null_state_gradients_are_zero_tensors(dev, name):
  case = C.CASES[name]
  before(case)
  zeros = C.run_layer(name, dev, zero_state_grads=True)
  null = C.run_layer(name, dev, null_dh=True, null_dc=True)
  one = C.run_layer(name, dev, zero_state_grads=True, null_dc=True) if case.cell == "LSTM" else null
  after(case)
  same_bits(null, zeros)
  same_bits(one, zeros)


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.LSTM_STEP_CASE])
def test_null_dx_gives_the_same_weight_gradients(dev, baseline, name):
  case = C.CASES[name]
  before(case)
  got = C.run_layer(name, dev, null_dx=True)
  after(case)
  assert "dx" not in got
  same_bits(got, baseline(name), keys=["y", "h_n"] + grad_keys(case))


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.LSTM_STEP_CASE])
def test_null_h_n_gives_the_same_y_and_gradients(dev, baseline, name):
  case = C.CASES[name]
  before(case)
  got = C.run_layer(name, dev, null_hn=True)
  after(case)
  assert "h_n" not in got and "c_n" not in got
  same_bits(got, baseline(name), keys=["y", "dx"] + grad_keys(case))


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.GRID_CASE, C.LSTM_STEP_CASE])
def test_second_backward_over_one_reserve(dev, baseline, name):
  """retain_graph: the second lr_rnn_layer_backward over a forward's reserve re-packs W_hh with a launch of its own (the
  one-launch paths) and must give the first one's bits."""
  case = C.CASES[name]
  before(case)
  got = C.run_layer(name, dev, backwards=2)
  after(case)
  same_bits(got, baseline(name))
  same_bits(got["second"], baseline(name), keys=["dx"] + grad_keys(case))


@pytest.mark.parametrize("name", C.PROPERTY_CASES + [C.GRID_CASE, C.LSTM_STEP_CASE, "x3_split", "x3exact_step"])
def test_accumulate_adds_to_the_prefill(dev, baseline, name):
  """accumulate = 1 on seeded gradients: pre-fill + gradient within the case's bound; y, h_n, dx as without."""
  case, inp = C.CASES[name], C.inputs(name)
  want64, cpu32 = C.reference(name)
  before(case)
  got = C.run_layer(name, dev, accumulate=True)
  after(case)
  same_bits(got, baseline(name), keys=["y", "h_n", "dx"])
  for k in grad_keys(case):
    hold_case(case, k + "+=", got[k], inp.prefill[k].double() + want64[k], inp.prefill[k] + cpu32[k])
