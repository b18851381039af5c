"""CPU: the semantics lr_edit_distance implements, restated in plain Python and checked against the
host code it must equal — Decoder.cer, Decoder.wer, the oracle's edit_distance — plus the scorer's tables, the driver
flag and the C entry points' argument checks (no device call).

The restatement lives here (tests/test_gpu_edit.py imports it): expansion of class ids through the spelling table,
the two units, and the alignment's walk back with its order of preference.  Everything is integer-exact."""
import random

import pytest
import torch

from lipreading_amd import _C
from lipreading_amd.data import EOS, UNK, default_char2idx
from lipreading_amd.decoder import Decoder, ctc_labels
from lipreading_amd.scoring import EditScorer, spelling_table


# ---- the restatement ---------------------------------------------------------------------------------------------
def expand(ids, labels, drop=(EOS,)):
  """Class ids -> the concatenation of their spellings (a dropped class spells '')."""
  return ''.join('' if labels[i] in drop else labels[i] for i in ids)


def table(h, r):
  """D[i][j] = Levenshtein distance between the first i items of h and the first j of r."""
  n, m = len(h), len(r)
  D = [[0] * (m + 1) for _ in range(n + 1)]
  for i in range(n + 1):
    D[i][0] = i
  for j in range(m + 1):
    D[0][j] = j
  for i in range(1, n + 1):
    for j in range(1, m + 1):
      D[i][j] = min(D[i - 1][j - 1] + (h[i - 1] != r[j - 1]), D[i][j - 1] + 1, D[i - 1][j] + 1)
  return D


def align(h, r, D=None):
  """The walk back from (n, m): the diagonal if it explains D[i][j], else a deletion (the reference character is
  absent from the hypothesis), else an insertion.  Returns (distance, hits, sub, ins, dele, steps) with steps a list of
  (reference character or None, hypothesis character or None).  `D`: table(h, r) if the caller has it already."""
  D = table(h, r) if D is None else D
  i, j = len(h), len(r)
  hits = sub = ins = dele = 0
  steps = []
  while i > 0 or j > 0:
    if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (h[i - 1] != r[j - 1]):
      if h[i - 1] == r[j - 1]:
        hits += 1
      else:
        sub += 1
      steps.append((r[j - 1], h[i - 1]))
      i, j = i - 1, j - 1
    elif j > 0 and D[i][j] == D[i][j - 1] + 1:
      dele += 1
      steps.append((r[j - 1], None))
      j -= 1
    else:
      assert i > 0 and D[i][j] == D[i - 1][j] + 1   # rule 3 is always a legal step when 1 and 2 are not
      ins += 1
      steps.append((None, h[i - 1]))
      i -= 1
  return D[len(h)][len(r)], hits, sub, ins, dele, steps


def score_ref(hyp_ids, ref_ids, labels, unit='char', drop=(EOS,)):
  """What one pair's row of lr_edit_distance's `out` must hold: dict(distance, ref_len, hyp_len, hits, sub, ins, dele)
  and the alignment's steps (character unit)."""
  h, r = expand(hyp_ids, labels, drop), expand(ref_ids, labels, drop)
  if unit == 'word':
    h, r = [w for w in h.split(' ') if w], [w for w in r.split(' ') if w]
    return dict(distance=table(h, r)[len(h)][len(r)], ref_len=len(r), hyp_len=len(h)), []
  h, r = h.replace(' ', ''), r.replace(' ', '')
  d, hits, sub, ins, dele, steps = align(h, r)
  return dict(distance=d, ref_len=len(r), hyp_len=len(h), hits=hits, sub=sub, ins=ins, dele=dele), steps


def confusion_ref(steps_list, symbols):
  """conf[(K+1)][(K+1)] of the listed alignments over the sorted alphabet; index K is "nothing"."""
  K = len(symbols)
  at = {ch: i for i, ch in enumerate(symbols)}
  conf = [[0] * (K + 1) for _ in range(K + 1)]
  for steps in steps_list:
    for r, h in steps:
      conf[K if r is None else at[r]][K if h is None else at[h]] += 1
  return conf


def random_ids(rng, n_classes, length, special=()):
  """Ids with runs of spaces and the marker classes over-represented."""
  out = []
  while len(out) < length:
    u = rng.random()
    if u < 0.15 and special:
      out += [rng.choice(special)] * rng.randint(1, 3)
    else:
      out.append(rng.randrange(n_classes))
  return out[:length]


LABELS = ctc_labels(default_char2idx())


def special_classes(labels):
  return [labels.index(' '), labels.index(EOS), labels.index(UNK)]


# ---- the restatement against the host code ------------------------------------------------------------------------
def test_restatement_equals_the_host_code_on_random_ids():
  from oracle import torch_oracle as O
  rng = random.Random(20240917)
  dec = Decoder(LABELS)
  sp = special_classes(LABELS)
  cases = [([], []), ([], [5, 6]), ([7], []), ([sp[0]] * 4, [sp[0]] * 2), ([sp[0]] * 3, [9, sp[0], 10]),
           ([sp[1]] * 2, [sp[1]]), ([sp[2]], [sp[2], sp[2]])]
  for _ in range(300):
    cases.append((random_ids(rng, len(LABELS), rng.randint(0, 45), sp), random_ids(rng, len(LABELS), rng.randint(0, 45), sp)))
  for hyp, ref in cases:
    hs = ''.join(LABELS[i] for i in hyp).replace(EOS, '')
    rs = ''.join(LABELS[i] for i in ref).replace(EOS, '')
    assert expand(hyp, LABELS) == hs and expand(ref, LABELS) == rs
    c, steps = score_ref(hyp, ref, LABELS, 'char')
    w, _ = score_ref(hyp, ref, LABELS, 'word')
    assert c["distance"] == dec.cer(hs, rs) == O.edit_distance(hs.replace(' ', ''), rs.replace(' ', ''))
    assert w["distance"] == dec.wer(hs, rs)
    assert c["ref_len"] == len(rs.replace(' ', '')) and c["hyp_len"] == len(hs.replace(' ', ''))
    assert w["ref_len"] == len(rs.split()) and w["hyp_len"] == len(hs.split())
    assert c["sub"] + c["ins"] + c["dele"] == c["distance"]
    assert c["hits"] + c["sub"] + c["dele"] == c["ref_len"]
    assert c["hits"] + c["sub"] + c["ins"] == c["hyp_len"]
    assert len(steps) == c["hits"] + c["sub"] + c["ins"] + c["dele"]


def test_unk_expands_to_five_characters_and_eos_to_none():
  unk, eos, a = LABELS.index(UNK), LABELS.index(EOS), LABELS.index('a')
  assert expand([a, unk, eos, a], LABELS) == 'a<UNK>a'
  assert score_ref([unk], [], LABELS)[0]["distance"] == 5
  assert score_ref([eos, eos], [], LABELS)[0]["distance"] == 0


def test_hand_worked_cases():
  assert table("kitten", "sitting")[6][7] == 3
  # "ac" against the reference "abc": c/c hit, then at (1, 2) the diagonal would cost 2, D[1][1] + 1 = 1 explains the
  # cell: 'b' is deleted; then a/a hit
  assert align("ac", "abc") == (1, 2, 0, 0, 1, [('c', 'c'), ('b', None), ('a', 'a')])
  # "ab" against "ba": D = [[0,1,2],[1,1,1],[2,1,2]].  At (2, 2) all three moves give 2: the diagonal is preferred, a
  # substitution (reference 'a', hypothesis 'b'); at (1, 1) the diagonal again (reference 'b', hypothesis 'a').  The
  # equally short "delete b, hit a, insert b" is NOT what the rule order yields.
  assert table("ab", "ba") == [[0, 1, 2], [1, 1, 1], [2, 1, 2]]
  assert align("ab", "ba") == (2, 0, 2, 0, 0, [('a', 'b'), ('b', 'a')])
  # an insertion: "xa" against "a": a/a hit, then only the hypothesis side is left
  assert align("xa", "a") == (1, 1, 0, 1, 0, [('a', 'a'), (None, 'x')])
  conf = confusion_ref([align("ac", "abc")[5], align("ab", "ba")[5]], ['a', 'b', 'c'])
  assert conf == [[1, 1, 0, 0],    # reference a: hit, read as b once
                  [1, 0, 0, 1],    # reference b: read as a once, deleted once
                  [0, 0, 1, 0],    # reference c: hit
                  [0, 0, 0, 0]]    # no insertions


# ---- the scorer's tables ------------------------------------------------------------------------------------------
def test_spelling_table_and_alphabet_of_the_default_ctc_labels():
  symbols, off, sym, space, longest = spelling_table(LABELS)
  assert symbols == sorted(set(''.join(l for l in LABELS if l != EOS)))
  assert len(off) == len(LABELS) + 1 and off[0] == 0 and off[-1] == len(sym)
  assert longest == 5 and symbols[space] == ' '
  for c, label in enumerate(LABELS):
    assert ''.join(symbols[s] for s in sym[off[c]:off[c + 1]]) == ('' if label == EOS else label)
  sc = EditScorer(LABELS)
  assert sc.K == len(symbols) and sc.symbols == symbols and sc.max_spelling == 5
  assert Decoder(LABELS).scorer().symbols == symbols
  # no ' ' among the labels: nothing is a space
  assert spelling_table(['_', 'a', 'b'])[3] == -1


def test_labels_that_can_spell_a_dropped_marker_are_refused():
  with pytest.raises(ValueError):
    EditScorer(['_', '<', 'E', 'O', 'S', '>', EOS, 'a'])
  with pytest.raises(ValueError):
    EditScorer(['_', '<EO', 'S>', EOS])
  EditScorer(['_', '<', 'O', 'S', '>', EOS, 'a'])   # no 'E' anywhere else: accepted


def test_score_flag():
  from lipreading_amd.driver import parse_flags
  assert parse_flags([])["score"] == "host"
  assert parse_flags(["--score=device"])["score"] == "device"
  assert parse_flags(["--score=host"])["score"] == "host"
  with pytest.raises(SystemExit):
    parse_flags(["--score=gpu"])


# ---- the C entry points, no device ---------------------------------------------------------------------------------
def test_workspace_query():
  lib = _C.lib()
  q = lib.lr_edit_workspace_bytes
  for bad in ((0, 8, 8, 1, 0), (1, 0, 8, 1, 0), (1, 8, 0, 1, 0), (1, 8, 8, 0, 0), (1, 8, 8, 1, 3), (1, 8, 8, 1, -1),
              (1, 4097, 8, 1, 0), (1, 8, 4097, 1, 1), (1, 820, 8, 5, 0), (1, 2049, 8, 1, 2), (1, 8, 2049, 1, 2)):
    assert q(*bad) == 0, bad
  # the distance modes keep everything in LDS: a 16-byte placeholder, so that 0 always means "rejected"
  assert q(32, 75, 30, 5, 0) == 16 and q(1000, 4096, 4096, 1, 0) == 16 and q(7, 4096, 4096, 1, 1) == 16
  # alignment: 2 bits per cell, rows padded to 4 cells; in LDS while it fits beside the sequences ...
  assert q(32, 75, 30, 5, 2) == 16
  # ... else B * align4(capH * ceil(capR / 4)) bytes of workspace
  assert q(3, 256, 256, 5, 2) == 3 * 1280 * 320
  assert q(1, 2048, 2048, 1, 2) == 2048 * 512
  assert q(2, 2047, 2047, 1, 2) == 2 * 2047 * 512


def test_null_arguments_are_rejected_without_a_device():
  lib = _C.lib()
  assert lib.lr_edit_distance(None, 0, None, 0, None, 0, None, 0, None, None, 65, 5, 4, 0, None, None, None, 60, None,
                              None, 0, 1, 8, 8, None) == -1


def test_cpu_tensors_raise():
  sc = EditScorer(LABELS)
  ids = torch.zeros((2, 4), dtype=torch.int32)
  lens = torch.tensor([4, 4], dtype=torch.int32)
  with pytest.raises(_C.LipReadingHipError):
    sc.score(ids, lens, ids, lens)
  with pytest.raises(_C.LipReadingHipError):
    sc.result()
