"""tests/decoder_loop_cases.py is what tests/test_gpu_decoder_fp64.py takes it for (no GPU): every case sits on the
dispatch branches it names, the table reaches every branch of the loop, the float64 reference IS the oracle's
CharDecodingStep looped L times, the lengths are ragged, masked classes carry no mass, no draw of the reference sits on a
class boundary — and a reference that is deliberately wrong leaves the float64 result by more than 100 x the bound the GPU
test applies.

The float32 CPU loop's error against float64 per tensor, relative to the tensor's largest entry (the yardstick of which the
GPU test takes 4 x), measured over the table on an Intel host: log_probs' live classes 6.1e-8 .. 1.2e-7, its masked classes
4.4e-8 .. 9.4e-8, the states 5.7e-8 .. 2.6e-7, d_enc / dh0 / dc0 5.8e-8 .. 6.3e-7, the parameter gradients 2.8e-8 .. 3.7e-6
(the largest: attn_proj_layer1.bias of step_lstm36_concat_l2_drop, a sum over 70 frames of tanh' terms that nearly cancel;
next 1.0e-6).  The figures belong to the host's BLAS as much as to the loop: on the host of the MI355X the same tensor came out
at 4.9e-6 and dh0 of one_lstm1156_dot at 2.8e-6 instead of 5.5e-7.  The 2e-5 asked of it below leaves a factor of four there."""
import pytest
import torch

from oracle import torch_oracle as O
from tests import decoder_loop_cases as C

SMALL = [n for n, c in C.CASES.items() if not C.wide(c)]


# ---- the branches ----------------------------------------------------------------------------------------------------------

def _expected_branches(case):
  """lr_decoder_forward / lr_decoder_backward_parts / resolve_shape / lr_rnn_grid_shape, restated."""
  G, Hd = C.GATES[case.cell], case.Hd
  bwd = "step"                    # ws_layout's xch_bytes: G != 1 && lr_rnn_cluster_supported, nothing about the pattern
  if G != 1:
    c32, c16 = (Hd + 31) // 32, (Hd + 15) // 16
    c16 += c16 & 1
    if G == 4 and 1152 < Hd <= 1536:
      bwd = "grid"
    elif c32 <= (27 if G == 3 else 24):
      bwd = "cluster32:%d" % c32
    elif (56 if G == 3 else 50) <= c16 <= 72:
      bwd = "cluster16:%d" % c16
  recur = bwd if all(case.tf[1:]) else "step"       # lr_decoder_forward's one_launch
  wgrad = "fgemm" if G * Hd >= 1536 else "grouped"
  out_rows = 8
  while out_rows > 1 and out_rows * (Hd + case.V) * 4 > 60 * 1024:
    out_rows >>= 1
  return recur, bwd, wgrad, out_rows


@pytest.mark.parametrize("name", list(C.CASES))
def test_cases_sit_on_the_branches_they_name(name):
  case = C.CASES[name]
  # sizes_ok, and the 60 KiB rules that would answer LR_ERR_UNSUPPORTED
  assert case.Hd % 4 == 0 and 0 < case.V <= 1024 and 1 <= case.layers <= 8 and case.Cd > 0
  assert (case.attn == "concat") == (case.A > 0)
  assert case.out_rows * (case.Hd + case.V) * 4 <= 60 * 1024 and 2 * case.A * 4 <= 60 * 1024
  assert case.attn != "concat" or case.L * case.T * 4 <= 60 * 1024
  assert case.drop <= (case.layers > 1)
  assert (case.recur, case.bwd, case.wgrad, case.out_rows) == _expected_branches(case)
  assert set(C.tensor_names(case)) - {"log_probs", "h_n", "c_n", "d_enc", "dh0", "dc0"} == {"d_" + k for k in C.inputs(name).params}


def test_every_branch_has_a_case():
  cases = list(C.CASES.values())
  assert {c.attn for c in cases} == set(C.ATTN)
  assert {c.cell for c in cases} == set(C.GATES)
  assert {c.recur.split(":")[0] for c in cases} == {"step", "cluster32", "cluster16", "grid"}
  for attn in C.ATTN:      # every attention type on one launch, and so on the step kernels too (its hooked twin)
    assert any(c.attn == attn for c in cases if C.one_launch(c) and C.step_twin(c)), attn
  # a forward on the step kernels with the backward on the cluster recurrence, and one with the step kernels both ways
  assert any(c.recur == "step" and c.bwd != "step" for c in cases) and any(c.bwd == "step" for c in cases)
  assert {c.wgrad for c in cases} == {"grouped", "fgemm"} and {c.out_rows for c in cases} == {8, 4}
  # the first wide size with a single fgemm job; a GRU's two W_hh jobs plus an upper layer's W_ih
  assert any(C.GATES[c.cell] * c.Hd == 1536 and c.layers == 1 and c.cell == "LSTM" for c in cases)
  assert any(c.wgrad == "fgemm" and c.cell == "GRU" and c.layers > 1 for c in cases)
  # sizes the 64-class loops, the 16-byte loads and the tiles do not divide
  assert any(c.V % 64 and c.V % 4 for c in cases) and any(c.V > 64 and c.V % 64 for c in cases)
  assert any(c.V == 1024 for c in cases)
  assert any(c.Cd % 4 for c in cases) and any(c.A % 4 for c in cases) and any(c.A > 64 for c in cases)
  assert any(c.B > 16 for c in cases) and any(c.T > 64 and max(C.inputs(c.name).lens[:-1]) < 64 for c in cases)
  assert any(c.B == c.L == c.T == 1 for c in cases)
  # layers with and without a drop mask; mixed teacher forcing, a first step that is "not forced", the G = 1 cell
  assert any(c.layers >= 2 and c.drop for c in cases) and any(c.layers >= 3 and not c.drop for c in cases)
  assert any(c.tf[0] == 0 for c in cases) and any(0 in c.tf[1:] and 1 in c.tf[1:] for c in cases)
  assert any(c.cell == "RNN" and all(c.tf) and c.recur == "step" for c in cases)
  assert C.CASES[C.BIAS_CASE].bias == -25.0 and C.CASES[C.BIAS_CASE].attn == "1_layer_nn"
  kinds = [C.CASES[n] for n in C.PROPERTY_CASES]
  assert [k.recur.split(":")[0] for k in kinds] == ["step", "cluster32", "cluster32", "grid"]
  assert [C.wide(k) for k in kinds] == [False, False, True, True]
  assert all(k.attn != "none" and k.layers == 1 for k in kinds)
  none = C.CASES[C.NONE_CASE]
  assert none.attn == "none" and none.layers == 2
  for w in C.WRONG:
    assert any(C.applies(w, C.CASES[n]) for n in SMALL), w


@pytest.mark.parametrize("name", list(C.CASES))
def test_lengths_are_ragged(name):
  case, lens = C.CASES[name], C.inputs(name).lens.tolist()
  assert len(lens) == case.B and all(1 <= n <= case.T for n in lens)
  assert lens[case.B - 1] == case.T and lens.count(case.T) == 1 or case.T == 1      # the last sample is full, no other one
  if case.B >= 3:
    assert lens[1] == 1 and len(set(lens)) > 1
    pad = ~C.valid_mask(name).expand_as(C.inputs(name).enc)
    assert pad.any() and float(C.inputs(name).enc[pad].abs().max()) > 0
    assert float(C.enc_with_garbage(name)[pad].abs().min()) >= 1e3
    assert torch.equal(C.enc_with_garbage(name)[~pad], C.inputs(name).enc[~pad])
  assert int(C.inputs(name).tokens.min()) >= 2 and int(C.inputs(name).tokens.max()) < case.V
  if case.drop:
    assert set(C.inputs(name).drop.unique().tolist()) == {0.0, 2.0}


# ---- the reference ---------------------------------------------------------------------------------------------------------

def _oracle_loop(name, sampled):
  """OracleCharDecodingStep(...).double() stepped L times on the case, fed as the loop is fed."""
  c, inp = C.CASES[name], C.inputs(name)
  with torch.random.fork_rng():
    dec = O.OracleCharDecodingStep(c.Hd, c.cell, c.layers, c.Cd, c.V, O.default_char2idx(), attention_type=c.attn,
                                   attn_hidden_size=c.A if c.A else -1).double()
  names = {"emb": "embedding.weight", "w_c": "concat_layer.weight", "b_c": "concat_layer.bias", "w_o": "output_proj.weight",
           "b_o": "output_proj.bias"}
  for l in range(c.layers):
    for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
      names[k + (str(l) if l else "")] = "rnn.%s_%s_l%d" % ("weight" if k[0] == "w" else "bias", k[2:], l)
  layer = {"1_layer_nn": ("attn_proj_1_layer_nn",), "general": ("attn_proj_general",),
           "concat": ("attn_proj_layer1", "attn_proj_layer2")}.get(c.attn, ())
  for n, mod in enumerate(layer):
    names["attn_w%d" % (n + 1)], names["attn_b%d" % (n + 1)] = mod + ".weight", mod + ".bias"
  missing = dec.load_state_dict({names[k]: v.double() for k, v in inp.params.items()}, strict=False)
  assert not missing.unexpected_keys and set(missing.missing_keys) <= {"concat_layer.weight", "concat_layer.bias"}
  assert dec.output_mask.dtype == torch.float32          # log(mask + 1e-45) stays a float32 evaluation: -103.2789
  enc = inp.enc.double().requires_grad_(True)
  h0, c0 = inp.h0.double().requires_grad_(True), inp.c0.double().requires_grad_(True)
  state = (h0, c0) if c.cell == "LSTM" else h0
  rows = []
  for i in range(c.L):
    ids = inp.tokens[:, i] if (c.tf[i] or i == 0) else sampled[:, i - 1]
    lp, state = dec(ids, state, inp.lens, enc)
    rows.append(lp)
  lp = torch.stack(rows, 1)
  h_n, c_n = state if c.cell == "LSTM" else (state, None)
  loss = (lp * inp.d_lp.double()).sum() + (h_n * inp.dh_n.double()).sum()
  if c_n is not None:
    loss = loss + (c_n * inp.dc_n.double()).sum()
  loss.backward()
  res = {"log_probs": lp.detach(), "h_n": h_n.detach(), "d_enc": enc.grad if enc.grad is not None else torch.zeros_like(enc),
         "dh0": h0.grad}
  if c_n is not None:
    res["c_n"], res["dc0"] = c_n.detach(), c0.grad
  sd = dict(dec.named_parameters())
  for k in inp.params:
    res["d_" + k] = sd[names[k]].grad
  return res


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if not c.drop])
def test_float64_reference_is_the_oracle_step_looped(name):
  case = C.CASES[name]
  want64, _ = C.reference(name)
  oracle = _oracle_loop(name, want64["sampled"])
  for k in C.tensor_names(case):
    sk = C.scale_key(case, k)
    err, _ = C.figures(oracle[k], want64[k], want64[sk])
    assert err <= 1e-12, (k, err)


@pytest.mark.parametrize("name", list(C.CASES))
def test_references_are_finite_and_the_yardstick_is_tight(name):
  case = C.CASES[name]
  want64, cpu32 = C.reference(name)
  assert torch.equal(want64["sampled"], cpu32["sampled"])
  worst = 0.0
  for k in C.tensor_names(case):
    assert want64[k].dtype == torch.float64 and cpu32[k].dtype == torch.float32, k
    assert torch.isfinite(want64[k]).all() and torch.isfinite(cpu32[k]).all(), k
    for what, a, b, s in C.pieces(case, k, cpu32, want64):
      err, _ = C.figures(a, b, s)
      worst = max(worst, err)
      print("%-34s %-22s float32 CPU against float64 %.2e" % (name, what, err))
      # what keeps 4 x the figure a bound that a wrong element cannot hide under
      assert err <= 2e-5, (what, err)
  if case.attn == "none":
    assert not want64["d_enc"].any()
  pad = ~C.valid_mask(name).expand_as(want64["d_enc"])
  assert not want64["d_enc"][pad].any() and not cpu32["d_enc"][pad].any()      # padded frames: exactly zero
  print("%-34s worst %.2e" % (name, worst))


def test_the_bias_case_makes_the_1e13_and_the_bias_gradient_visible():
  case = C.CASES[C.BIAS_CASE]
  want64, _ = C.reference(C.BIAS_CASE)
  # the score bias has a real gradient on the scale of its sibling weight gradient ...
  assert float(want64["d_attn_b1"].abs().max()) > 1e-3 * float(want64["d_attn_w1"].abs().max())
  # ... where every other '1_layer_nn' / 'concat' case has a mathematically zero one
  for name, c in C.CASES.items():
    for k in C.grad_keys(c):
      if C.scale_key(c, k) != k and name != C.BIAS_CASE:
        w64, _ = C.reference(name)
        assert float(w64[k].abs().max()) < 1e-9 * float(w64[C.scale_key(c, k)].abs().max()), (name, k)


@pytest.mark.parametrize("name", list(C.CASES))
def test_masked_classes_carry_no_mass_and_no_draw_sits_on_a_boundary(name):
  """exp(lp) == 0 in float32 for PAD and BOS; with the float64 reference's own log_probs and the case's seed no (sample,
  step) row has u * total within DRAW_SLACK of a class boundary, so the reference needs none of the slack the GPU test
  grants — and its draws are live classes."""
  case = C.CASES[name]
  want64, cpu32 = C.reference(name)
  for r in (want64, cpu32):
    _, masked = C.split_log_probs(r["log_probs"])
    assert not masked.float().exp().any()
  pick, lo, hi, margin = C.draws(want64["log_probs"], case.seed)
  assert float(margin.min()) > C.DRAW_SLACK, (float(margin.min()), margin.argmin())
  assert torch.equal(pick, lo) and torch.equal(pick, hi)
  assert torch.equal(pick, want64["sampled"]) and int(pick.min()) >= 2 and int(pick.max()) < case.V
  # u depends on the step and on the sample
  us = {(b, i): C.hash_uniform(case.seed, i, b) for b in range(case.B) for i in range(case.L)}
  assert len(set(us.values())) == len(us) and all(0 <= u < 1 for u in us.values())


def test_hash_uniform_is_the_kernels():
  """Values worked out by hand from lr_decoder_dev.h's definition (splitmix64's finaliser on seed + golden * counter)."""
  def by_hand(seed, step, sample):
    m = (1 << 64) - 1
    x = (seed + 0x9E3779B97F4A7C15 * (step * 0x100000001B3 + sample + 1)) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return ((x ^ (x >> 31)) >> 40) * 2.0 ** -24
  for args in [(0, 0, 0), (11, 3, 7), ((1 << 64) - 1, 65535, 65534), (5, 1, 0), (5, 0, 1)]:
    assert C.hash_uniform(*args) == by_hand(*args)
  assert C.hash_uniform(5, 1, 0) != C.hash_uniform(5, 0, 1)
  # the rule: the first class whose cumulative mass exceeds u * total
  lp = torch.tensor([0.0, 0.25, 0.25, 0.5]).log().clamp(min=-110.0)
  assert [C.draw(lp, u)[0] for u in (0.0, 0.2499, 0.25, 0.4999, 0.5, 0.999)] == [1, 1, 2, 2, 3, 3]


# ---- wrong references --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrong", C.WRONG)
def test_a_wrong_reference_is_caught(wrong):
  """Each deliberately wrong loop leaves the float64 result by more than 100 x the exact bound (4 x the float32 CPU error,
  at least 4 ulp) on some tensor of some case: the cases can see the error."""
  caught = {}
  for name in SMALL:
    case = C.CASES[name]
    if not C.applies(wrong, case):
      continue
    want64, cpu32 = C.reference(name)
    bad64 = C.evaluate(name, torch.float64, want64["sampled"], wrong=wrong)
    for k in C.tensor_names(case):
      for (what, cpu, want, scale), (_, bad, _, _) in zip(C.pieces(case, k, cpu32, want64), C.pieces(case, k, bad64, want64)):
        cpu_err, _ = C.figures(cpu, want, scale)
        bound, _ = C.bounds(case, k, cpu_err, hooked=True)
        err, _ = C.figures(bad, want, scale)
        if err > 100 * bound:
          caught.setdefault(name, []).append((what, err / bound))
  print(wrong, {n: len(v) for n, v in caught.items()})
  assert caught, wrong
  assert any(k == "log_probs live" for v in caught.values() for k, _ in v)      # ... and in the forward already
