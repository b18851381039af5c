"""CPU: the yardstick of the forced aligner (tests/align_cases.py) against brute force and against itself at double
precision, the structure of its paths, word grouping against str.split(), and the argument checks of the C entry
points and the host layer that need no device."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from lipreading_amd import _C, driver, lm
from lipreading_amd.data import EOS, UNK, default_char2idx
from lipreading_amd.decoder import ctc_labels
from tests import align_cases as A

LABELS = ctc_labels(default_char2idx())
ROLES = lm.class_roles(LABELS, 0)

# (T, L) of the exactness cases: the one-wave and multi-wave limits, odd sizes, up to the kernel's limits
QUANT_SHAPES = ((1, 0), (2, 1), (17, 5), (75, 31), (76, 32), (130, 33), (200, 75), (300, 128), (400, 200), (512, 256))


def test_restatement_equals_enumeration():
  rng = np.random.RandomState(0)
  C, blank = 3, 0
  feasible = infeasible = 0
  for T in range(1, 7):
    for L in range(0, 4):
      for y in itertools.product((1, 2), repeat=L):
        for _ in range(3):
          lp = A.integers(rng, (T, C))
          total, path = A.viterbi(lp, list(y), blank)
          want = A.best_by_enumeration(lp, y, blank)
          assert (path is None) == (want is None) == (T < L + A.repeats(y)), (T, y)
          if want is None:
            assert total == -np.inf
            infeasible += 1
          else:
            assert float(total) == want, (T, y, total, want)
            assert float(sum(lp[t, 0 if s % 2 == 0 else y[s // 2]] for t, s in enumerate(path))) == want
            feasible += 1
  assert feasible > 100 and infeasible > 20


def quant_cases():
  rng = np.random.RandomState(1)
  C = 65
  for T, L in QUANT_SHAPES + ((2048, 256),):
    for k in range(1 if T == 2048 else 3):
      yield T, L, A.quantised(rng, (T, C)), A.random_target(rng, L, C, 0, doubled=k == 1)


@pytest.fixture(scope="module")
def quant_paths():
  out = []
  for T, L, lp, y in quant_cases():
    out.append((lp, y, A.viterbi(lp, y, 0, np.float32), A.viterbi(lp, y, 0, np.float64)))
  return out


def test_yardstick_is_exact_on_quantised_values(quant_paths):
  """Multiples of 1/64 in (-16, 0]: partial sums need at most 21 bits, so float32 loses nothing — scores bit-equal,
  paths equal."""
  aligned = 0
  for lp, y, (t32, p32), (t64, p64) in quant_paths:
    assert t32.dtype == np.float32 and t64.dtype == np.float64
    assert float(t32) == float(t64)
    assert p32 == p64
    aligned += p32 is not None
  assert aligned >= 25


def test_structure_of_the_restated_path(quant_paths):
  for lp, y, (total, path), _ in quant_paths:
    if path is None:
      assert len(lp) < len(y) + A.repeats(y)
      continue
    classes = [0 if s % 2 == 0 else y[s // 2] for s in path]
    assert A.collapse(classes, 0) == y
    r = A.align_one(lp, y, 0, ROLES)
    prev_end = 0
    for s, e, _ in r["tok"]:
      assert prev_end <= s < e <= len(lp)      # ordered, disjoint, non-empty
      prev_end = e
    for i, (s, e, _) in enumerate(r["tok"]):
      assert r["frame_token"][s:e] == [i] * (e - s)   # contiguous
    blanks = np.float32(0)
    for t, ft in enumerate(r["frame_token"]):
      if ft < 0:
        blanks = np.float32(blanks + lp[t, 0])
    # (every partial sum is exact on these values, so the order of summation does not matter)
    assert float(sum(float(p) for _, _, p in r["tok"]) + float(blanks)) == float(total)
    for f, c, s, e, p in r["words"]:
      assert (s, e) == (r["tok"][f][0], r["tok"][f + c - 1][1])
      assert float(p) == sum(float(r["tok"][i][2]) for i in range(f, f + c))


def test_word_grouping_equals_str_split():
  at = {l: i for i, l in enumerate(LABELS)}
  for text in ("hello world", " leading", "trailing ", "two  spaces", "  a  b  ", "", " ", "x"):
    y = [at[ch] for ch in text] + [at[EOS]]
    words = A.words_of(y, ROLES)
    assert [''.join(LABELS[y[i]] for i in range(f, f + c)) for f, c in words] == text.split()
    assert all(f + c <= len(text) for f, c in words)     # '<EOS>' belongs to no word
  # '<UNK>' inside a word ends it
  y = [at[ch] for ch in "ab"] + [at[UNK]] + [at[ch] for ch in "cd e"] + [at[EOS]]
  assert A.words_of(y, ROLES) == [(0, 2), (3, 2), (6, 1)]


def _align_call(lib, T=75, max_label_len=30, null=None, C=65, target_stride=None, ws_bytes=1 << 20):
  """lr_ctc_align with host buffers for every pointer (never dereferenced: each of these calls returns before any
  launch); `null`: the index of the pointer argument to pass as NULL."""
  buf = ctypes.create_string_buffer(64)
  p = [ctypes.addressof(buf)] * 18   # log_probs sizes targets target_lens roles | 12 outputs | workspace
  if null is not None:
    p[null] = None
  ts = max_label_len if target_stride is None else target_stride
  return lib.lr_ctc_align(p[0], T * C, C, p[1], p[2], ts, p[3], p[4], 0, *p[5:17], p[17], ws_bytes, 2, T, C,
                          max_label_len, None)


def test_entry_points_check_their_arguments_without_a_device():
  lib = _C.lib()
  required = (0, 2, 3, 5, 6, 7, 8, 15, 16, 17)    # log_probs targets target_lens frame_token tok_* total status workspace
  for k in required:
    assert _align_call(lib, null=k) == _C.LR_ERR_INVALID_ARG, k
  for k in range(9, 15):                          # the word outputs and n_words are required with class_roles
    assert _align_call(lib, null=k) == _C.LR_ERR_INVALID_ARG, k
  assert _align_call(lib, T=2049) == _C.LR_ERR_UNSUPPORTED
  assert _align_call(lib, max_label_len=257) == _C.LR_ERR_UNSUPPORTED
  assert _align_call(lib, target_stride=31) == _C.LR_ERR_INVALID_ARG       # wider than max_label_len
  assert _align_call(lib, T=2048, max_label_len=256, ws_bytes=16) == _C.LR_ERR_WORKSPACE
  assert lib.lr_ctc_align_workspace_bytes(1, 2049, 65, 30) == 0
  assert lib.lr_ctc_align_workspace_bytes(1, 75, 65, 257) == 0
  assert lib.lr_ctc_align_workspace_bytes(0, 75, 65, 30) == 0
  assert lib.lr_ctc_align_workspace_bytes(32, 75, 65, 30) == 16            # rows and table in LDS
  assert lib.lr_ctc_align_workspace_bytes(3, 2048, 65, 256) == 3 * 128 * 576 * 4
  # the plan query: kernel, threads, rows in LDS, table in LDS, dynamic LDS bytes — and it agrees with the workspace query
  plan = (ctypes.c_int32 * 5)()
  at = ctypes.addressof(plan)
  assert lib.lr_ctc_align_plan(32, 75, 65, 30, None) == _C.LR_ERR_INVALID_ARG
  assert lib.lr_ctc_align_plan(32, 2049, 65, 30, at) == _C.LR_ERR_UNSUPPORTED
  for (T, L), want in (((75, 30), [1, 256, 1, 1]), ((75, 31), [1, 256, 1, 1]), ((75, 32), [0, 128, 1, 1]),
                       ((1000, 31), [1, 64, 0, 1]), ((300, 128), [0, 320, 0, 1]), ((2048, 256), [0, 576, 0, 0])):
    assert lib.lr_ctc_align_plan(4, T, 65, L, at) == 0
    assert list(plan)[:4] == want, (T, L, list(plan))
    assert 0 < plan[4] <= 65536 - 512
    assert (lib.lr_ctc_align_workspace_bytes(4, T, 65, L) == 16) == bool(plan[3])


def test_driver_flag_and_host_layer():
  assert driver.DEFAULTS["align"] == "" and driver.parse_flags([])["align"] == ""
  f = driver.parse_flags(["--align=/tmp/out/val.jsonl", "--enable_ctc=True"])
  assert f["align"] == "/tmp/out/val.jsonl"
  assert driver.parse_flags(["--align=a.jsonl", "--frontend=conv3d"])["align"] == "a.jsonl"   # a CTC-only regime
  with pytest.raises(ValueError):
    driver.parse_flags(["--align=a.jsonl"])
  from lipreading_amd.align import CTCAligner
  al = CTCAligner(LABELS)
  assert al.roles == ROLES and al.seconds(2997) == 100.0
  assert CTCAligner(['_', 'a', 'b']).roles is None
  tg, tl = al.encode(["ab c", ""])
  assert tg.tolist() == [[LABELS.index(ch) for ch in "ab c"], [0, 0, 0, 0]] and tl.tolist() == [4, 0]
  for bad in ("a_b", "café"):
    with pytest.raises(KeyError):
      al.encode([bad])
  lp = torch.zeros(2, 5, 65)
  with pytest.raises(_C.LipReadingHipError):
    al.align_ids(lp, torch.tensor([5, 5]), torch.ones(2, 3, dtype=torch.int32), torch.tensor([3, 3]))
