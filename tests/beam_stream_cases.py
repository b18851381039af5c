"""Helpers for the session tests (tests/test_beam_stream_cpu.py, tests/test_gpu_beam_stream.py; not collected): the
parity inputs, the chunkings, and stream_ref, the restatement of a session (lr_ctc_beam_stream_*,
lipreading_amd/csrc/lr_ctc_beam.hip) in terms of the float64 restatements of the one-shot searches: the state after t
frames is the one-shot restatement run on the first t frames."""
import numpy as np

from tests import beam_bias_cases as K
from tests.test_beam_cpu import beam_ref
from tests.test_beam_lm_cpu import beam_lm_ref

LABELS = K.TRAP_LABELS + ["<EOS>"]   # _, ' ', a..z, <EOS>
TEXTS = ["the cat sat on", "a dog ran", "hello there you", "we go", "pan the channel", "one two three"]
B, T, C = len(TEXTS), 40, len(LABELS)

# how T = 40 frames are cut; every slot gets the whole chunk
CHUNKINGS = {"whole": [40], "frames": [1] * 40, "mixed": [7, 1, 0, 13, 19]}
# ragged: the chunks' lengths, and per chunk how many of its frames each slot consumes; the slots' totals differ
RAGGED_T = [10, 12, 8, 10]
RAGGED_SIZES = [[10, 10, 10, 0, 0, 10],
                [12, 12, 0, 1, 0, 12],
                [8, 8, 7, 0, 0, 8],
                [10, 3, 0, 0, 0, 10]]
RAGGED_TOTALS = [40, 33, 17, 1, 0, 40]

HOT = [("pan", 10.0), ("channel", 6.0), ("an", 2.5), ("the cat", 8.0), ("a", 0.5), ("three", 4.0)]
LM_WORDS = sorted({w for t in TEXTS for w in t.split()} | {"cat", "can", "than", "tree", "on", "an"})


def parity_frames():
  """The six utterances, clean and sharply peaked: (B, T, C) float32 probabilities."""
  from tests.test_gpu_beam_lm import spoken_frames
  return spoken_frames(np.random.default_rng(0), TEXTS, T, C, LABELS, noise=0.0, strength=(8.0, 11.0))


def lm_sentences():
  """A seeded corpus over the texts' words for tests.test_beam_lm_cpu.write_arpa."""
  rng = np.random.default_rng(5)
  sents = [t.split() for t in TEXTS] * 20
  sents += [[LM_WORDS[int(i)] for i in rng.integers(0, len(LM_WORDS), int(rng.integers(2, 5)))] for _ in range(120)]
  return sents


def hot_phrases(labels=LABELS):
  return [(K.spell_ids(text, labels), w) for text, w in HOT]


def common_prefix(hyps):
  """Length of the longest common prefix of the id tuples."""
  if not hyps:
    return 0
  n = min(len(h) for h in hyps)
  for d in range(n):
    if any(h[d] != hyps[0][d] for h in hyps):
      return d
  return n


def one_shot_ref(v, size, W, n, cutoff_prob=1.0, blank=0, log_input=False, lm=None, dic=None, alpha=0.0, beta=0.0,
                 bias=None):
  """The one-shot restatement of the variant: [(ids, offsets, score)], best first."""
  if bias is not None:
    return K.beam_bias_ref(v, size, W, n, bias, cutoff_prob, blank, log_input, lm, dic, alpha, beta)
  if lm is not None:
    return beam_lm_ref(v, size, W, n, lm, dic, alpha, beta, cutoff_prob, blank, log_input)
  return beam_ref(v, size, W, n, cutoff_prob, blank, log_input)


def stream_ref(v, chunks, W, n, **kw):
  """One slot fed `chunks` frames at a time from v (T, C): per chunk border (frames consumed, the hypotheses the
  one-shot restatement holds after that many frames, stable = the common prefix of all of them)."""
  out, t = [], 0
  for c in chunks:
    t += c
    hyps = one_shot_ref(v, t, W, n, **kw)
    out.append((t, hyps, common_prefix([h[0] for h in hyps])))
  return out


def ragged_chunks(p):
  """RAGGED_* applied to p (B, T, C): per chunk (tensor (B, chunk_T, C), sizes): slot b's consumed frames are its next
  ones, the rest of its rows another slot's frames, which must not be read."""
  cur = [0] * B
  out = []
  for ct, sizes in zip(RAGGED_T, RAGGED_SIZES):
    x = np.empty((B, ct, C), np.float32)
    for b in range(B):
      x[b] = p[(b + 1) % B, :ct]
      x[b, :sizes[b]] = p[b, cur[b]:cur[b] + sizes[b]]
      cur[b] += sizes[b]
    out.append((x, np.asarray(sizes, np.int32)))
  assert cur == RAGGED_TOTALS
  return out
