"""No GPU: the restatement of the transducer beam search (tests/transducer_beam_cases.py) against brute force, against the
loss's lattice and against itself fed in chunks; the named cases' margin condition; the driver's --transducer_beam."""
import pytest
import torch

from tests import transducer_beam_cases as K


def model(c):
  return c["tables"], c["W"], c["b"], c["mask"]


@pytest.mark.parametrize("name", sorted(K.EXHAUSTIVE))
def test_every_prefix_survives_with_the_brute_force_sum(name):
  c, st, stats, _ = K.reference(name)
  beam = st["beams"][0]
  T = c["e"].shape[1]
  assert len(beam) == c["nprefix"]                 # every string of at most T * max_symbols labels over two classes
  assert len(set(h[0] for h in beam)) == len(beam)
  assert all(k in (1, 2) for h in beam for k in h[0])
  assert stats["merges"] > 0
  for prefix, score, frames in beam:
    want = K.brute_force_score(c["e"][0], T, *model(c), prefix, c["max_symbols"])
    assert abs(score - want) <= 1e-12 * max(1.0, abs(want)), (prefix, score, want)
    assert len(frames) == len(prefix) and list(frames) == sorted(frames) and all(0 <= f < T for f in frames)
    assert all(frames.count(f) <= c["max_symbols"] for f in frames)
    if len(prefix) <= c["max_symbols"]:            # the cap binds nowhere: the loss's own sum
      lat = K.lattice_score(c["e"][0], T, *model(c), prefix)
      assert abs(score - lat) <= 1e-12 * max(1.0, abs(lat)), (prefix, score, lat)
    else:
      assert score <= K.lattice_score(c["e"][0], T, *model(c), prefix) + 1e-12


def test_brute_force_without_a_binding_cap_is_the_lattice():
  c = K.exhaustive_case("t3s1")
  for prefix in ((), (1,), (2, 1), (1, 2, 2)):
    full = K.brute_force_score(c["e"][0], 3, *model(c), prefix, max_symbols=3)
    assert abs(full - K.lattice_score(c["e"][0], 3, *model(c), prefix)) <= 1e-12 * abs(full)


@pytest.mark.parametrize("name", ["ragged", "odd", "small_w32"])
def test_a_pruned_score_never_exceeds_the_lattice(name):
  c, st, _, _ = K.reference(name)
  for i, beam in enumerate(st["beams"]):
    Tb = int(c["sizes"][i])
    for prefix, score, _ in beam:
      if Tb == 0:
        assert prefix == () and score == 0.0
      else:
        assert score <= K.lattice_score(c["e"][i], Tb, *model(c), prefix) + 1e-9


@pytest.mark.parametrize("chunk", [1, 3, 5])
@pytest.mark.parametrize("name", ["ragged", "vocab"])
def test_chunks_equal_the_one_shot_run(name, chunk):
  c, st, _, _ = K.reference(name)
  T = c["e"].shape[1]
  state = None
  for t0 in range(0, T, chunk):
    piece = dict(c, e=c["e"][:, t0:t0 + chunk], sizes=(c["sizes"] - t0).clamp(0, chunk))
    state = K.run(piece, state=state)
  assert state["beams"] == st["beams"] and state["truncated"] == st["truncated"]
  assert state["frame_base"] == [int(s) for s in c["sizes"]]


def test_a_small_max_out_truncates_and_counts():
  c, st, _, _ = K.reference("odd")
  short = K.run(c, max_out=2)
  assert all(len(h[0]) <= 2 for beam in short["beams"] for h in beam)
  assert sum(short["truncated"]) > 0 and st["truncated"] == [0, 0]


@pytest.mark.parametrize("name", sorted(K.FP32_ERROR))
def test_every_named_case_meets_the_margin_condition(name):
  assert set(K.FP32_ERROR) == set(K.CASES) | set(K.EXHAUSTIVE)
  assert K.margin_holds(name), (name, K.smallest_gap(K.reference(name)[2]), K.FP32_ERROR[name])


def test_the_cases_cover_what_they_must():
  widths = {K.CASES[n][2] for n in K.CASES}
  assert {1, 4, 32} <= widths
  contexts = {K.make_case(n)["tables"].shape[0] for n in ("ragged", "odd")}
  assert contexts == {1, 2}
  odd = K.make_case("odd")
  assert odd["W"].shape == (37, 45)
  assert 0 in K.CASES["ragged"][1]
  for name in ("ragged", "vocab", "small_w32", "workload"):
    assert K.FP32_ERROR[name][3] > 0                                     # the tabled merges ...
  assert K.reference("ragged")[2]["merges"] == K.FP32_ERROR["ragged"][3]   # ... are the oracle's


def test_driver_flag_checks():
  from lipreading_amd import driver
  base = ["--enable_ctc=True", "--ctc_only=True", "--transducer=True"]
  assert driver.parse_flags(base)["transducer_beam"] == 0 and driver.parse_flags([])["transducer_beam"] == 0
  assert driver.parse_flags(base + ["--transducer_beam=4"])["transducer_beam"] == 4
  assert driver.parse_flags(base + ["--transducer_beam=32", "--transducer_max_symbols=8"])["transducer_beam"] == 32
  assert driver.parse_flags(base + ["--transducer_max_symbols=9"])["transducer_max_symbols"] == 9   # greedy: no cap
  for flags in (["--transducer_beam=4"], ["--enable_ctc=True", "--ctc_only=True", "--transducer_beam=4"],
                base + ["--transducer_beam=33"], base + ["--transducer_beam=-1"],
                base + ["--transducer_beam=4", "--transducer_max_symbols=9"]):
    with pytest.raises(ValueError, match="transducer_beam"):
      driver.parse_flags(flags)
