"""train.py's evaluation-loop helpers on device="cpu" with stand-ins: the scoring arithmetic of the one host CER loop
(ctc_cer / attention_cer), the context manager that switches an encoder to the per-step kernels, and the retry helper,
which on a CPU device neither rolls nor reads the fault words."""
import pytest
import torch

from lipreading_amd import train as T
from lipreading_amd.data import BOS, EOS, default_char2idx
from lipreading_amd.decoder import Decoder, ctc_labels

C2I = default_char2idx()
V = len(C2I)
REFS = [["ab cd", "hello"], ["x y"]]
HYPS = [["ab cd" + EOS, "hallo"], ["xx y"]]
# space-free distances 0 + 1 + 1 over space-free reference lengths 4 + 5 + 2
WANT = 2 / 11


def ids_of(text):
  out, i = [], 0
  while i < len(text):
    if text.startswith(EOS, i):
      out.append(C2I[EOS])
      i += len(EOS)
    else:
      out.append(C2I[text[i]])
      i += 1
  return out


def make_loader():
  loader = []
  for refs in REFS:
    rows = [[C2I[BOS]] + ids_of(r) + [C2I[EOS]] for r in refs]
    width = max(len(r) for r in rows)
    chars = torch.zeros(len(rows), width, dtype=torch.long)
    for b, r in enumerate(rows):
      chars[b, :len(r)] = torch.tensor(r)
    n = len(rows)
    loader.append((torch.zeros(n, 6, 68, 3), torch.full((n,), 6), chars, torch.tensor([len(r) for r in rows])))
  return loader


class StubEncoder(object):
  enable_ctc = True

  def eval(self):
    return self

  def forward(self, frames, lens, max_len=None):
    B = frames.shape[0]
    return torch.zeros(B, max_len, V + 1), torch.zeros(B, max_len, 3), None

  __call__ = forward


class StubCTCDecoder(Decoder):
  def __init__(self):
    super(StubCTCDecoder, self).__init__(ctc_labels(C2I), blank_index=0)
    self.batches = iter(HYPS)

  def decode(self, probs, sizes=None):
    assert probs.shape[2] == V + 1 and probs.shape[0] == len(sizes)
    return [[h] for h in next(self.batches)], None


class StubDecodingStep(object):
  def __init__(self):
    self.batches, self.seen = iter(HYPS), []

  def eval(self):
    return self

  def beam_search(self, hidden, frame_lens, state, beam_width, max_label_len, **joint):
    self.seen.append(joint)
    rows = [ids_of(h if h.endswith(EOS) else h + EOS) for h in next(self.batches)]
    ids = torch.zeros(len(rows), beam_width, max(len(r) for r in rows), dtype=torch.int32)
    lens = torch.zeros(len(rows), beam_width, dtype=torch.int32)
    for b, r in enumerate(rows):
      ids[b, 0, :len(r)] = torch.tensor(r, dtype=torch.int32)
      lens[b, 0] = len(r)
    return ids, lens, torch.zeros(len(rows), beam_width)


def test_ctc_cer_scores_space_free_distance_over_space_free_length():
  assert T.ctc_cer(StubEncoder(), make_loader(), "cpu", C2I, StubCTCDecoder()) == WANT
  assert T.ctc_cer(StubEncoder(), [], "cpu", C2I, StubCTCDecoder()) == 0.0
  assert T.greedy_cer(StubEncoder(), [], "cpu", C2I) == 0.0


@pytest.mark.parametrize("ctc_weight", [0.0, 0.3])
def test_attention_cer_scores_the_same_and_passes_joint_keywords_only_when_joint(ctc_weight):
  step = StubDecodingStep()
  got = T.attention_cer(StubEncoder(), step, make_loader(), "cpu", C2I, beam_width=3, max_label_len=20,
                        ctc_weight=ctc_weight, pre_beam=7)
  assert got == WANT
  assert len(step.seen) == len(REFS)
  for joint in step.seen:
    if ctc_weight == 0.0:
      assert joint == {}
    else:
      assert sorted(joint) == ["ctc_log_probs", "ctc_weight", "pre_beam"]
      assert joint["ctc_weight"] == ctc_weight and joint["pre_beam"] == 7
      assert joint["ctc_log_probs"].shape[1:] == (6, V + 1)
  assert T.attention_cer(StubEncoder(), StubDecodingStep(), [], "cpu", C2I, ctc_weight=ctc_weight) == 0.0


class Plain(object):
  pass


def recurrent():
  enc = Plain()
  enc.recurrence = 'auto'
  return enc


def wrapped():
  outer = Plain()
  outer.encoder = recurrent()
  return outer


@pytest.mark.parametrize("make,inner_of", [(recurrent, lambda e: e), (wrapped, lambda e: e.encoder)],
                         ids=["bare", "wrapped"])
def test_step_kernels_switches_and_restores(make, inner_of):
  enc = make()
  with T._step_kernels(enc):
    assert inner_of(enc).recurrence == 'f32'
  assert inner_of(enc).recurrence == 'auto'
  with pytest.raises(KeyError):
    with T._step_kernels(enc):
      assert inner_of(enc).recurrence == 'f32'
      raise KeyError("inside")
  assert inner_of(enc).recurrence == 'auto'
  if inner_of(enc) is not enc:
    assert not hasattr(enc, "recurrence")


def test_step_kernels_leaves_an_encoder_without_the_attribute_alone():
  enc = Plain()
  with T._step_kernels(enc):
    assert not hasattr(enc, "recurrence")
  with pytest.raises(KeyError):
    with T._step_kernels(enc):
      raise KeyError("inside")
  assert vars(enc) == {}


def test_retried_on_cpu_runs_once_and_touches_no_fault_word(monkeypatch):
  def boom(*a, **k):
    raise AssertionError("the fault words are device state: not on a CPU device")

  monkeypatch.setattr(T, "_roll_faults", boom)
  monkeypatch.setattr(T, "_fault_keep", boom)
  calls = []
  enc = recurrent()
  assert T._retried(enc, None, lambda: calls.append(enc.recurrence) or "out") == "out"
  assert calls == ['auto'] and enc.recurrence == 'auto'
  # and through a whole loop
  assert T.ctc_cer(StubEncoder(), make_loader(), "cpu", C2I, StubCTCDecoder()) == WANT
