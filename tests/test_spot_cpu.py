"""CPU: the restatement of lr_ctc_spot (tests/spot_cases.py) against brute-force enumeration, its tie, suppression,
threshold and status rules, and the host-side checks around the spotter.  No GPU."""
import math

import numpy as np
import pytest

from tests import spot_cases as S

f32 = np.float32


def tiny_cases():
  """60 cases: n <= 6, C = 3 (blank 0), L <= 3, integer log-probabilities (every sum exact), doubled letters among
  them."""
  rng = np.random.RandomState(20)
  for i in range(60):
    n = int(rng.randint(1, 7))
    L = int(rng.randint(1, 4))
    y = S.random_target(rng, L, 3, 0, doubled=i % 3 == 2)
    lp = S.integers(rng, (n, 3))
    yield lp, y


def test_the_restatement_equals_enumeration_on_tiny_cases():
  finite = 0
  for lp, y in tiny_cases():
    d = S.ratios(lp)
    score, start = S.trace(d, y, 0)
    brute = S.best_by_enumeration(d, y, 0)
    for t, (best, starts) in enumerate(brute):
      if best is None:
        assert score[t] == -np.inf and start[t] == -1, (lp, y, t)
      else:
        assert float(score[t]) == best, (lp, y, t)
        assert int(start[t]) in starts, (lp, y, t, start[t], starts)
        finite += 1
  assert finite > 50       # (the comparison is not vacuous)


def test_the_batched_restatement_equals_the_one_keyword_restatement():
  rng = np.random.RandomState(11)
  for name, family in S.FAMILIES:
    d = S.ratios(family(rng, (40, 9)))
    d[5, 3] = -np.inf
    kw, ln = S.keyword_batch(rng, [1, 2, 7, 8, 9, 16, 17, 3, 3], 9, 0, stride=20)
    score, start = S.trace_batch(d, kw, ln, 0)
    for k in range(len(ln)):
      one_score, one_start = S.trace(d, [int(c) for c in kw[k, :ln[k]]], 0)
      assert np.array_equal(score[k], one_score) and np.array_equal(start[k], one_start), (name, k)


def test_finite_scores_are_not_positive_and_reachability():
  """end_score[t] is finite exactly when t + 1 >= L + #{i: y[i] == y[i-1]}."""
  rng = np.random.RandomState(3)
  for name, family in S.FAMILIES:
    for L in (1, 2, 5, 9):
      for doubled in (False, True):
        y = S.random_target(rng, L, 7, 0, doubled)
        score, start = S.trace(S.ratios(family(rng, (14, 7))), y, 0)
        need = L + S.repeats(y)
        for t in range(14):
          assert np.isfinite(score[t]) == (t + 1 >= need), (name, y, t)
          assert (start[t] >= 0) == bool(np.isfinite(score[t]))
          if np.isfinite(score[t]):
            assert score[t] <= 0 and 0 <= start[t] <= t + 1 - need


def test_ratios_are_zero_at_the_argmax_and_take_minus_infinity():
  lp = np.array([[-1.0, -np.inf, -3.0], [-2.0, -2.0, -5.0]], f32)
  d = S.ratios(lp)
  assert d.dtype == np.float32 and d.tolist() == [[0.0, -np.inf, -2.0], [0.0, 0.0, -3.0]]
  score, start = S.trace(d, [1], 0)
  assert score.tolist() == [-np.inf, 0.0] and start.tolist() == [-1, 1]


def test_an_all_zero_run_of_the_first_token_keeps_the_earlier_start():
  """y[0] is the arg-max on frames 1..4: the fresh start (0, t) never beats the stay at 0, so the start stays 1."""
  lp = np.full((6, 3), -4.0, f32)
  lp[1:5, 1] = 0.0
  lp[0, 0] = lp[5, 0] = 0.0
  score, start = S.trace(S.ratios(lp), [1], 0)
  assert score.tolist() == [-4.0, 0.0, 0.0, 0.0, 0.0, -4.0]
  assert start.tolist() == [0, 1, 1, 1, 1, 1]        # (frame 5: the stay at 0 is not beaten by a fresh 0 either)
  # two tokens: the second inherits the first one's earliest start
  lp[4, 1], lp[4, 2] = -4.0, 0.0
  score, start = S.trace(S.ratios(lp), [1, 2], 0)
  assert score[4] == 0.0 and start[4] == 1


def test_equal_score_hits_come_out_by_smallest_end_and_never_overlap():
  score = np.array([-np.inf, -1.0, -1.0, -2.0, -1.0, -1.0, -3.0], f32)
  start = np.array([-1, 0, 1, 3, 3, 5, 6], np.int32)
  got = S.hits(score, start, None, 4)
  # t = 1 ([0, 2)) first; t = 2 ([1, 3)) overlaps it; t = 4 ([3, 5)); t = 5 ([5, 6)); then t = 6 ([6, 7))
  assert [(float(s), a, e) for s, a, e in got] == [(-1.0, 0, 2), (-1.0, 3, 5), (-1.0, 5, 6), (-3.0, 6, 7)]
  assert S.hits(score, start, None, 2) == got[:2]
  rng = np.random.RandomState(8)
  for _ in range(20):
    y = S.random_target(rng, int(rng.randint(1, 4)), 5, 0)
    sc, st = S.trace(S.ratios(S.integers(rng, (30, 5))), y, 0)
    got = S.hits(sc, st, None, 16)
    spans = [(a, e) for _, a, e in got]
    for i, (a, e) in enumerate(spans):
      assert all(not (a < e2 and a2 < e) for a2, e2 in spans[:i])
    assert [float(s) for s, _, _ in got] == sorted((float(s) for s, _, _ in got), reverse=True)
    # a candidate that was not reported overlaps a reported span (or the list is full)
    if len(got) < 16:
      for t in range(30):
        if np.isfinite(sc[t]) and (int(st[t]), t + 1) not in spans:
          assert any(int(st[t]) < e and a < t + 1 for a, e in spans)


def test_min_scores_filter_with_greater_or_equal():
  score = np.array([-2.0, -1.5, -2.0, -0.5], f32)
  start = np.array([0, 1, 2, 3], np.int32)
  assert [e for _, _, e in S.hits(score, start, f32(-1.5), 4)] == [4, 2]
  assert [e for _, _, e in S.hits(score, start, np.nextafter(f32(-1.5), f32(0)), 4)] == [4]
  assert S.hits(score, start, f32(0.0), 4) == []


def test_status_rules():
  rng = np.random.RandomState(4)
  lp = S.log_softmax(rng, (3, 9, 5))
  kw = np.array([[1, 2, 3], [1, 0, 2], [4, 5, 1], [2, -1, 1], [3, 99, 99], [1, 1, 1], [1, 1, 1]], np.int32)
  lens = np.array([3, 3, 2, 2, 1, 0, 4], np.int32)
  sizes = np.array([9, 0, 10], np.int32)
  want = S.expected(lp, sizes, kw, lens, 0, None, 2)
  assert want["status"][0].tolist() == [0, S.BAD_ID, S.BAD_ID, S.BAD_ID, 0, S.BAD_LENGTH, S.BAD_LENGTH]
  assert (want["status"][1:] == S.BAD_LENGTH).all()
  bad = want["status"] != 0
  assert (want["n_hits"][bad] == 0).all() and (want["hit_score"][bad] == -np.inf).all()
  assert (want["hit_start"][bad] == -1).all() and (want["hit_end"][bad] == -1).all()
  assert (want["end_score"][bad] == -np.inf).all() and (want["end_start"][bad] == -1).all()
  assert want["n_hits"][0, 0] >= 1 and want["n_hits"][0, 4] == 2


def test_the_spotter_checks_its_arguments_on_the_host():
  import torch
  from lipreading_amd import _C
  from lipreading_amd.spot import KeywordSpotter
  labels = ['_'] + list("abc ")
  sp = KeywordSpotter(labels, ["ab", "c", "a b", "abcab"], min_confidence=0.5, max_hits=3)
  assert sp.ids.tolist() == [[1, 2, 0, 0, 0], [3, 0, 0, 0, 0], [1, 4, 2, 0, 0], [1, 2, 3, 1, 2]]
  assert sp.lengths.tolist() == [2, 1, 3, 5]
  assert sp.min_scores.dtype == np.float32
  assert sp.min_scores.tolist() == [float(f32(L * math.log(0.5))) for L in (2, 1, 3, 5)]
  assert sp._order.tolist() == [1, 0, 2, 3]
  assert sp.seconds(2997) == 100.0
  assert KeywordSpotter(labels, ["a"]).min_scores is None
  with pytest.raises(KeyError):
    KeywordSpotter(labels, ["abd"])
  with pytest.raises(KeyError):
    KeywordSpotter(labels, ["a_"])          # the blank's label is no character
  for bad in ([""], ["a" * 33], []):
    with pytest.raises(ValueError):
      KeywordSpotter(labels, bad)
  KeywordSpotter(labels, ["a" * 32])
  for kw in (dict(max_hits=0), dict(max_hits=17), dict(min_confidence=0.0), dict(min_confidence=1.5)):
    with pytest.raises(ValueError):
      KeywordSpotter(labels, ["a"], **kw)
  with pytest.raises(_C.LipReadingHipError):
    sp.spot_ids(torch.zeros(1, 4, 5))
  with pytest.raises(_C.LipReadingHipError):
    sp.spot(torch.zeros(1, 4, 5))


def test_the_library_decides_limits_and_null_pointers_on_the_host():
  import ctypes
  from lipreading_amd import _C
  lib = _C.lib()
  ws = lib.lr_ctc_spot_workspace_bytes
  assert ws(32, 75, 65, 100, 10, 4) == 16
  assert ws(8, 2048, 65, 100, 10, 4) == 8 * 100 * 2048 * 8
  for args in ((1, 2049, 65, 1, 4, 4), (1, 75, 65, 1, 33, 4), (1, 75, 65, 1, 4, 17), (1, 75, 65, 0, 4, 4),
               (1, 75, 65, 1, 0, 4), (1, 75, 65, 1, 4, 0), (0, 75, 65, 1, 4, 4)):
    assert ws(*args) == 0, args
  plan = (ctypes.c_int32 * 11)()
  assert lib.lr_ctc_spot_plan(1, 2049, 65, 1, 4, 4, ctypes.addressof(plan)) == _C.LR_ERR_UNSUPPORTED
  assert lib.lr_ctc_spot_plan(1, 75, 65, 1, 33, 4, ctypes.addressof(plan)) == _C.LR_ERR_UNSUPPORTED
  assert lib.lr_ctc_spot_plan(1, 75, 65, 1, 4, 17, ctypes.addressof(plan)) == _C.LR_ERR_UNSUPPORTED
  assert lib.lr_ctc_spot_plan(1, 75, 65, 1, 4, 4, None) == _C.LR_ERR_INVALID_ARG
  assert lib.lr_ctc_spot_plan(32, 75, 65, 100, 10, 4, ctypes.addressof(plan)) == 0
  seg, threads, side_by_side, groups, rows_lds, trace_at, lds_bytes, per_wg, len16, len32, wgs = list(plan)
  assert (seg, threads, side_by_side, rows_lds, trace_at) == (32, 256, 2, 1, 0)
  assert (len16, len32) == (8, 16) and (groups, per_wg) == (4, 16) and wgs == 32 * -(-100 // per_wg)
  assert lds_bytes == -(-75 * 65 * 4 // 16) * 16 + 16 * 75 * 8 and lds_bytes <= 65536   # rows (to 16 bytes) + traces
  for L, want in ((1, 16), (8, 16), (9, 32), (16, 32), (17, 64), (32, 64)):
    assert lib.lr_ctc_spot_plan(1, 75, 65, 1, L, 4, ctypes.addressof(plan)) == 0 and plan[0] == want
  # null required pointers: no device call (this test runs without a device)
  assert lib.lr_ctc_spot(None, 0, 0, None, None, 4, None, None, 0, 4, None, None, None, None, None, None, None, None, 0,
                         1, 75, 65, 1, None) == _C.LR_ERR_INVALID_ARG


def test_driver_flag_checks():
  from lipreading_amd import driver
  base = ["--enable_ctc=True", "--ctc_only=True"]
  f = driver.parse_flags(base + ["--spot=out.jsonl", "--keywords=the,of", "--spot_confidence=0.25", "--spot_max_hits=2"])
  assert (f["spot"], f["keywords"], f["spot_confidence"], f["spot_max_hits"]) == ("out.jsonl", "the,of", 0.25, 2)
  assert driver.parse_flags(base)["spot"] == ""
  with pytest.raises(ValueError, match="keywords"):
    driver.parse_flags(base + ["--spot=out.jsonl"])
  with pytest.raises(ValueError, match="CTC head"):
    driver.parse_flags(["--spot=out.jsonl", "--keywords=the"])
  with pytest.raises(ValueError):
    driver.parse_flags(base + ["--spot=out.jsonl", "--keywords=the", "--spot_confidence=2"])
  with pytest.raises(ValueError):
    driver.parse_flags(base + ["--spot=out.jsonl", "--keywords=the", "--spot_max_hits=17"])
  with pytest.raises(ValueError, match="keywords"):
    driver.run(root=".", data="none", spot="x.jsonl", enable_ctc=True, max_epochs=0)


def test_keywords_come_from_a_list_or_a_file(tmp_path):
  from lipreading_amd import driver
  assert driver.read_keywords("the,of,good morning") == ["the", "of", "good morning"]
  assert driver.read_keywords(" the, of ,good morning,,") == ["the", "of", "good morning"]   # blanks around, not inside
  p = tmp_path / "kw.txt"
  p.write_text("the\ngood morning\n\nof\n")
  assert driver.read_keywords(str(p)) == ["the", "good morning", "of"]
  p.write_text(" the \r\ngood morning\n")
  assert driver.read_keywords(str(p)) == ["the", "good morning"]
  assert driver.read_keywords(str(p) + ",of") == [str(p), "of"]       # with a comma it is a list, whatever it names
  assert driver.read_keywords(str(tmp_path / "absent")) == [str(tmp_path / "absent")]
  with pytest.raises(ValueError):
    driver.read_keywords(",")


def test_keyword_report_counts_at_word_boundaries():
  from lipreading_amd.analysis import caption_contains, keyword_counts
  assert caption_contains("the cat sat", "cat") and caption_contains("cat", "cat")
  assert caption_contains("the cat", "cat") and caption_contains("cat sat", "cat")
  assert not caption_contains("concatenate", "cat") and not caption_contains("cats", "cat")
  assert not caption_contains("tomcat sat", "cat")
  assert caption_contains("tomcat cat", "cat")                 # a later occurrence at a boundary counts
  assert caption_contains("say good morning all", "good morning")
  assert not caption_contains("say good mornings", "good morning")
  captions = ["the cat sat", "concatenate", "a cat", "dog"]
  hit = lambda k: dict(index=k, keyword="", start=0, end=1, score=0.0, confidence=1.0)
  hits = [[hit(0)], [hit(0), hit(0)], [], [hit(1), hit(0)]]
  got = keyword_counts(captions, hits, ["cat", "dog"])
  assert got == [dict(keyword="cat", utterances=2, hit=1, false_hits=3),
                 dict(keyword="dog", utterances=1, hit=1, false_hits=0)]
