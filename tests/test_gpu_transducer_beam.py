"""GPU: lr_rnnt_beam_decode through lipreading_amd.transducer.rnnt_beam against the float64 restatement of
tests/transducer_beam_cases.py, against brute force and the device's own RNN-T loss, fed in chunks, at its edges, through
TransducerHead and through the driver's --transducer_beam.

Discrete outputs (ids, lens, frames, count, truncated) are equal to the restatement's; a score may differ by 8 x the
float32 restatement's own error on the case (tests/transducer_beam_cases.py FP32_ERROR), and a case is only used while
its smallest decision gap is 64 x that error."""
import numpy as np
import pytest
import torch

from lipreading_amd import transducer as TR
from tests import transducer_beam_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def case32(name):
  return K.make_case(name, torch.float32) if name in K.CASES else K.exhaustive_case(name, torch.float32)


def device_beam(c, dev, e=None, sizes=None, state=None, **kw):
  a = dict(beam_width=c["beam_width"], max_symbols=c["max_symbols"], max_out=c["max_out"])
  a.update(kw)
  if state is not None:
    a.pop("max_out")
  return TR.rnnt_beam((c["e"] if e is None else e).to(dev), (c["sizes"] if sizes is None else sizes).to(dev),
                      c["tables"].to(dev), c["W"].to(dev), c["b"].to(dev), c["mask"].to(dev), state=state, **a)


def host(out):
  return {k: out[k].cpu() for k in ("ids", "frames", "lens", "scores", "count", "truncated")}


def assert_matches(got, want, tol, what):
  for k in ("ids", "lens", "frames", "count", "truncated"):
    assert torch.equal(got[k], want[k]), (what, k, got[k], want[k])
  live = torch.isfinite(want["scores"])
  assert torch.equal(torch.isfinite(got["scores"]), live), what
  assert torch.all(got["scores"][~live] == float("-inf")), what
  err = float((got["scores"].double()[live] - want["scores"][live]).abs().max())
  print("%s: largest score error %.3g (tolerance %.3g)" % (what, err, tol))
  assert err <= tol, (what, err, tol)


def same_bits(a, b):
  return all(torch.equal(a[k], b[k]) for k in ("ids", "frames", "lens", "scores", "count", "truncated")) and \
      torch.equal(a["state"]["buffer"], b["state"]["buffer"]) and \
      torch.equal(a["state"]["frame_base"], b["state"]["frame_base"])


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_named_case_matches_float64(dev, name):
  assert K.margin_holds(name)                      # on the oracle alone
  c, _, stats, want = K.reference(name)
  if K.FP32_ERROR[name][3] > 0:
    assert stats["merges"] == K.FP32_ERROR[name][3] > 0
  out = device_beam(case32(name), dev)
  assert_matches(host(out), want, K.score_tolerance(name), name)
  assert int(out["state"]["status"].item()) == 0
  assert torch.equal(out["state"]["frame_base"].cpu(), c["sizes"])


@pytest.mark.parametrize("name", sorted(K.EXHAUSTIVE))
def test_exhaustive_inputs_give_every_prefix_with_the_brute_force_sum(dev, name):
  assert K.margin_holds(name)
  c, _, _, want = K.reference(name)
  c32 = case32(name)
  got = host(device_beam(c32, dev))
  tol = K.score_tolerance(name)
  assert_matches(got, want, tol, name)
  assert int(got["count"][0]) == c["nprefix"]
  T = c["e"].shape[1]
  prefixes = [tuple(int(k) for k in got["ids"][0, n, :int(got["lens"][0, n])]) for n in range(c["nprefix"])]
  assert len(set(prefixes)) == c["nprefix"]
  model = (c["tables"], c["W"], c["b"], c["mask"])
  for n, prefix in enumerate(prefixes):
    brute = K.brute_force_score(c["e"][0], T, *model, prefix, c["max_symbols"])
    assert abs(float(got["scores"][0, n]) - brute) <= tol, (prefix, float(got["scores"][0, n]), brute)
  nll = device_nll(c32, got, dev)
  for n, prefix in enumerate(prefixes):
    score = float(got["scores"][0, n])
    assert score <= -float(nll[0][n]) + tol
    if len(prefix) <= c["max_symbols"]:            # the cap binds nowhere: the loss's own sum
      assert abs(score + float(nll[0][n])) <= tol, (prefix, score, float(nll[0][n]))


def device_nll(c32, got, dev):
  """nll of every reported prefix under the device's RNN-T loss (no TransducerHead: the case's tables make p):
  a list per sample of float tensors, one entry per live hypothesis."""
  tables, out = c32["tables"].to(dev), []
  for i in range(got["ids"].shape[0]):
    n, Tb = int(got["count"][i]), int(c32["sizes"][i])
    if n == 0 or Tb == 0:
      out.append(torch.zeros(n))
      continue
    ids, lens = got["ids"][i, :n].to(dev), got["lens"][i, :n].to(dev)
    U = max(int(lens.max()), 1)
    y = torch.cat((ids.new_zeros((n, 2)), ids[:, :U]), dim=1).long()
    p = tables[0][y[:, 1:U + 2]]
    if tables.shape[0] == 2:
      p = p + tables[1][y[:, 0:U + 1]]
    e = c32["e"][i:i + 1, :Tb].to(dev).expand(n, Tb, -1).contiguous()
    _, _, info = TR.rnnt_loss(e, p, c32["W"].to(dev), c32["b"].to(dev), c32["mask"].to(dev), ids[:, :U].contiguous(),
                              torch.full((n,), Tb, dtype=torch.int32, device=dev), lens, "sum")
    assert int(info["sample_status"].abs().sum().item()) == 0
    out.append(info["nll"].cpu())
  return out


@pytest.mark.parametrize("name", ["vocab", "small_w32"])
def test_a_score_never_exceeds_the_loss_of_its_prefix(dev, name):
  c32 = case32(name)
  got = host(device_beam(c32, dev))
  tol = K.score_tolerance(name)
  nll = device_nll(c32, got, dev)
  for i in range(got["ids"].shape[0]):
    for n in range(int(got["count"][i])):
      assert float(got["scores"][i, n]) <= -float(nll[i][n]) + tol, (i, n)


# ---- resumption and reproducibility ------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 3, 5])
@pytest.mark.parametrize("name", ["ragged", "vocab"])
def test_chunks_give_the_one_shot_bits(dev, name, chunk):
  c = case32(name)
  whole = device_beam(c, dev)
  T = c["e"].shape[1]
  out = None
  for t0 in range(0, T, chunk):
    out = device_beam(c, dev, e=c["e"][:, t0:t0 + chunk], sizes=(c["sizes"] - t0).clamp(0, chunk),
                      state=None if out is None else out["state"])
  assert same_bits(out, whole)
  assert int(out["state"]["status"].item()) == 0


def test_two_runs_give_the_same_bits(dev):
  c = case32("workload")
  assert same_bits(device_beam(c, dev), device_beam(c, dev))


# ---- the edges ---------------------------------------------------------------------------------------------------------
def test_a_small_max_out_truncates_counts_and_leaves_neighbours_alone(dev):
  c64 = K.reference("odd")[0]
  stats = K.new_stats()
  want_state = K.run(c64, max_out=2, stats=stats)
  assert K.margin_holds("odd", stats)
  want = K.as_arrays(want_state, c64["beam_width"], 2)
  assert int(want["truncated"].sum()) > 0
  c = case32("odd")
  got = host(device_beam(c, dev, max_out=2))
  assert_matches(got, want, K.score_tolerance("odd"), "odd, max_out 2")
  assert int(got["lens"].max()) <= 2 and got["ids"].shape[2] == 2
  # sample 1 cut to two frames: sample 0 keeps its bits
  short = host(device_beam(c, dev, sizes=torch.tensor([int(c["sizes"][0]), 2], dtype=torch.int32), max_out=2))
  alone = host(device_beam(dict(c, e=c["e"][:1]), dev, sizes=c["sizes"][:1], max_out=2))
  for k in ("ids", "frames", "lens", "scores", "count", "truncated"):
    assert torch.equal(short[k][0], got[k][0]) and torch.equal(alone[k][0], got[k][0]), k


def test_a_sample_without_frames_answers_the_empty_prefix(dev):
  c = case32("ragged")
  got = host(device_beam(c, dev))
  assert int(c["sizes"][1]) == 0
  assert int(got["count"][1]) == 1 and int(got["lens"][1, 0]) == 0 and float(got["scores"][1, 0]) == 0.0
  assert torch.all(got["scores"][1, 1:] == float("-inf")) and int(got["lens"][1, 1:].abs().sum()) == 0
  assert int(got["ids"][1].abs().sum()) == 0 and int(got["truncated"][1]) == 0


def test_nbest_returns_the_first_rows(dev):
  c = case32("vocab")
  full, two = host(device_beam(c, dev)), host(device_beam(c, dev, nbest=2))
  assert two["scores"].shape == (4, 2) and two["ids"].shape[:2] == (4, 2)
  for k in ("ids", "frames", "lens", "scores"):
    assert torch.equal(two[k], full[k][:, :2]), k
  assert torch.equal(two["count"], full["count"].clamp(max=2)) and torch.equal(two["truncated"], full["truncated"])
  one = host(device_beam(case32("odd_w1"), dev, sizes=torch.tensor([1, 0], dtype=torch.int32)))
  assert one["scores"].shape == (2, 1) and torch.all(torch.isfinite(one["scores"]))
  # a beam that is not full yet: the empty slots are -inf with length 0
  first = host(device_beam(c, dev, e=c["e"][:, :1], sizes=torch.tensor([1, 1, 1, 0], dtype=torch.int32), max_symbols=1,
                           beam_width=32, nbest=32))
  assert int(first["count"][3]) == 1 and torch.all(first["scores"][3, 1:] == float("-inf"))
  n = int(first["count"][0])
  assert n == 32 or (torch.all(first["scores"][0, n:] == float("-inf")) and int(first["lens"][0, n:].sum()) == 0)


def test_rejections_raise_before_any_launch(dev):
  c = case32("ragged")
  for kw in (dict(beam_width=0), dict(beam_width=33), dict(max_symbols=0), dict(max_symbols=9), dict(nbest=0),
             dict(nbest=5), dict(max_out=0), dict(max_out=257)):
    with pytest.raises(ValueError):
      device_beam(c, dev, **kw)
  args = [c[k].to(dev) for k in ("tables", "W", "b", "mask")]
  e, sizes = c["e"].to(dev), c["sizes"].to(dev)
  with pytest.raises(ValueError):
    TR.rnnt_beam(e, sizes, torch.cat((args[0],) * 3), *args[1:])                       # context 3
  with pytest.raises(ValueError):
    TR.rnnt_beam(e, sizes, args[0], args[1][:, :-1], *args[2:])                        # joint_weight of another J
  with pytest.raises(ValueError):
    TR.rnnt_beam(torch.zeros((3, 1, 513), device=dev), None, torch.zeros((1, 5, 513), device=dev),
                 torch.zeros((5, 513), device=dev), args[2], args[3])                  # J past the limit
  with pytest.raises(ValueError):
    TR.rnnt_beam(e[:, :0], sizes, *args)                                                # T = 0
  L = TR._C.lib()
  assert L.lr_rnnt_beam_state_bytes(3, 33, 10) == 0 and L.lr_rnnt_beam_state_bytes(3, 4, 257) == 0
  assert L.lr_rnnt_beam_state_bytes(0, 4, 10) == 0 and L.lr_rnnt_beam_workspace_bytes(3, 5, 8, 4, 9) == 0
  assert L.lr_rnnt_beam_workspace_bytes(3, 257, 8, 4, 2) == 0 and L.lr_rnnt_beam_workspace_bytes(3, 5, 513, 4, 2) == 0
  assert L.lr_rnnt_beam_state_bytes(3, 4, 18) == 32 + 12 * 8 + 3 * 4 + 12 * 4 + 2 * 12 * 18 * 4


def test_a_state_of_another_geometry_is_refused(dev):
  c = case32("ragged")
  out = device_beam(c, dev)
  before = out["state"]["buffer"].clone()
  args = [c[k].to(dev) for k in ("e", "sizes", "tables", "W", "b", "mask")]
  for kw in (dict(beam_width=2), dict(beam_width=4, max_out=5), dict(beam_width=8)):
    with pytest.raises(ValueError, match="state"):
      TR.rnnt_beam(*args, max_symbols=2, state=out["state"], **kw)
  with pytest.raises(ValueError, match="state"):
    TR.rnnt_beam(args[0], args[1], torch.cat((args[2], args[2])), *args[3:], beam_width=4, max_symbols=2,
                 state=out["state"])                                                   # another context
  with pytest.raises(ValueError, match="state"):
    device_beam(dict(c, e=c["e"][:2]), dev, sizes=c["sizes"][:2], state=out["state"])   # another batch
  assert torch.equal(out["state"]["buffer"], before)
  # the same size but not a state: the host cannot tell, the device's status word does
  forged = dict(out["state"], buffer=torch.zeros_like(before), truncated=torch.full((3,), 7, dtype=torch.int32, device=dev))
  forged["status"] = forged["buffer"][:32].view(torch.int32)[5]
  got = device_beam(c, dev, state=forged)
  assert int(forged["status"].item()) == TR.BEAM_BAD_STATE
  assert int(got["count"].abs().sum()) == 0 and torch.all(got["scores"] == float("-inf"))
  assert int(got["truncated"].sum()) == 21 and int(forged["buffer"][32:].abs().sum()) == 0
  # a buffer of another size never reaches a launch
  with pytest.raises(ValueError, match="state"):
    device_beam(c, dev, state=dict(out["state"], buffer=before[:-8].clone()))


# ---- the head and the driver -------------------------------------------------------------------------------------------
def test_head_beam_and_decode_strings_match_the_restatement(dev):
  from lipreading_amd.data import EOS, default_char2idx
  from lipreading_amd.decoder import ctc_labels
  char2idx = default_char2idx()
  for seed in range(20, 40):   # a head whose restatement keeps the margin (decided on the oracle alone)
    torch.manual_seed(seed)
    head = TR.TransducerHead(24, len(char2idx), char2idx, joint_dim=40, embed_dim=8, context=2)
    hidden = torch.randn(2, 6, 24)
    sizes = torch.tensor([6, 4], dtype=torch.int32)
    with torch.no_grad():
      model = dict(tables=head.tables(), W=head.joint.weight, b=head.joint.bias, mask=head.output_mask)
      e = head.enc_proj(hidden)
      stats = K.new_stats()
      run = lambda dt, st=None: K.beam_search(e.to(dt), sizes, *(model[k].to(dt) for k in ("tables", "W", "b", "mask")),
                                              beam_width=4, max_symbols=3, stats=st)
      st64, st32 = run(torch.float64, stats), run(torch.float32)
    if [[h[0] for h in b] for b in st64["beams"]] != [[h[0] for h in b] for b in st32["beams"]]:
      continue
    err = max(abs(x[1] - y[1]) for b64, b32 in zip(st64["beams"], st32["beams"]) for x, y in zip(b64, b32))
    err = max(err, K.FP32_HALF_ULP * max(abs(h[1]) for b in st64["beams"] for h in b))
    if K.smallest_gap(stats) >= K.MARGIN_FACTOR * err:
      break
  else:
    raise AssertionError("no seed keeps the margin")
  want = K.as_arrays(st64, 4, 18)
  head = head.to(dev)
  out = head.beam(hidden.to(dev), sizes.to(dev), beam_width=4, max_symbols=3)
  assert out["ids"].shape == (2, 4, 18)
  assert_matches(host(out), want, K.TOL_FACTOR * err, "head")
  labels = ctc_labels(char2idx)
  strings = head.decode_strings(hidden.to(dev), sizes.to(dev), max_symbols=3, beam_width=4)
  assert strings == [''.join(labels[k] for k in b[0][0]).replace(EOS, '') for b in st64["beams"]]
  greedy = head.greedy(hidden.to(dev), sizes.to(dev), max_symbols=3)
  assert head.decode_strings(hidden.to(dev), sizes.to(dev), max_symbols=3) == \
      [''.join(labels[int(k)] for k in greedy["ids"][i, :int(greedy["lens"][i])].cpu()).replace(EOS, '') for i in range(2)]


def test_driver_reports_a_beam_search_cer(dev, tmp_path, capsys):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synthetic/nano", n_videos=6, captions_per_video=5, seed=11)
  flags = driver.parse_flags(["--data=synthetic/nano", "--batch_size=5", "--enable_ctc=True", "--ctc_only=True",
                              "--rnn_type=GRU", "--bidirectional=True", "--hidden_size=32", "--learning_rate=3e-4",
                              "--grad_norm=400", "--cuda=True", "--transducer=True", "--transducer_joint=64",
                              "--transducer_embed=16", "--encoder=rnn", "--num_layers=1", "--root=" + root,
                              "--max_epochs=1", "--transducer_beam=4", "--transducer_max_symbols=3"])
  out = driver.run(**flags)
  text = capsys.readouterr().out
  h = out["history"]
  assert len(h) == 1 and np.isfinite(h[0]["transducer_loss"]) and h[0]["transducer_loss"] > 0
  assert np.isfinite(h[0]["val_cer"]) and h[0]["val_cer"] >= 0.0
  assert "Transducer CER (val): " in text
