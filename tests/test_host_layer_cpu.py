"""CPU: the host call layer of the inference entry points (lipreading_amd/_host.py) on CPU tensors and fakes, and
BeamCTCDecoder's one owner of its packed language model.  tests/test_gpu_host_layer.py holds the entry points that use
it on the device."""
import contextlib

import pytest
import torch

from lipreading_amd import _C, _host
from tests.test_beam_lm_cpu import TOY


def test_device_key_equates_cpu_spellings_and_is_hashable():
  assert _host.device_key("cpu") == _host.device_key(torch.device("cpu")) == ("cpu", None)
  assert _host.device_key("cuda:1") == _host.device_key(torch.device("cuda", 1)) == ("cuda", 1)
  assert len({_host.device_key("cpu"), _host.device_key(torch.device("cpu"))}) == 1


def test_device_key_resolves_a_bare_cuda_to_the_current_device(monkeypatch):
  monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
  assert _host.device_key("cuda") == _host.device_key(torch.device("cuda:3")) == ("cuda", 3)


def test_per_device_makes_once_per_key():
  made = []

  def make(dev):
    made.append(dev)
    return object()

  cache = _host.PerDevice()
  a = cache.get("cpu", make)
  assert cache.get(torch.device("cpu"), make) is a and made == ["cpu"]
  b = cache.get("cuda:1", make)
  assert b is not a and cache.get(torch.device("cuda", 1), make) is b and made == ["cpu", "cuda:1"]
  assert list(cache.values()) == [a, b]


def test_log_probs_3d_returns_an_acceptable_tensor_itself():
  x = torch.randn(2, 12, 6)
  assert _host.log_probs_3d(x, 6, "log_probs") is x
  assert _host.log_probs_3d(x, 9, "probs") is x


def test_log_probs_3d_takes_the_transposed_view_as_it_is():
  v = torch.randn(12, 2, 6).transpose(0, 1)
  assert not v.is_contiguous()
  assert _host.log_probs_3d(v, 6, "log_probs") is v


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_log_probs_3d_converts_to_fp32(dtype):
  x = torch.randn(2, 12, 6).to(dtype)
  got = _host.log_probs_3d(x, 6, "log_probs")
  assert got.dtype == torch.float32 and torch.equal(got, x.float())
  v = x.transpose(0, 1)   # (the conversion alone leaves the class stride at 1)
  assert _host.log_probs_3d(v, 6, "log_probs").stride(2) == 1


def test_log_probs_3d_makes_a_class_strided_view_contiguous():
  v = torch.randn(2, 12, 12)[:, :, ::2]
  got = _host.log_probs_3d(v, 6, "log_probs")
  assert got is not v and got.is_contiguous() and torch.equal(got, v)
  w = torch.randn(2, 6, 12).transpose(1, 2)   # classes along the slow dimension
  got = _host.log_probs_3d(w, 12, "log_probs")
  assert got.stride(2) == 1 and torch.equal(got, w)


@pytest.mark.parametrize("what", ["log_probs", "probs"])
def test_log_probs_3d_rejects_a_tensor_that_is_not_3d(what):
  with pytest.raises(ValueError, match=r"^%s must be \(batch, frames, classes\), got \(12, 6\)$" % what):
    _host.log_probs_3d(torch.zeros(12, 6), 6, what)


@pytest.mark.parametrize("what", ["log_probs", "probs"])
def test_log_probs_3d_rejects_more_classes_than_labels(what):
  with pytest.raises(KeyError, match="^'%s has 6 classes but only 5 labels'$" % what):
    _host.log_probs_3d(torch.zeros(2, 12, 6), 5, what)


def test_int32_vector():
  assert _host.int32_vector(None, 2, "sizes") is None
  t = torch.tensor([12, 9], dtype=torch.int32)
  assert _host.int32_vector(t, 2, "sizes") is t
  assert _host.int32_vector(t, 2, "sizes", device=torch.device("cpu")) is t
  got = _host.int32_vector(torch.tensor([12, 9]), 2, "sizes")
  assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == [12, 9]
  col = torch.tensor([[12, 1], [9, 2]], dtype=torch.int32)[:, 0]
  got = _host.int32_vector(col, 2, "sizes")
  assert got.is_contiguous() and got.tolist() == [12, 9]
  assert _host.int32_vector(col, 2, "hyp_lens", strided=True) is col   # (the scorer hands the kernel the stride)


@pytest.mark.parametrize("bad", [torch.zeros(3, dtype=torch.int32), torch.zeros((2, 1), dtype=torch.int32),
                                 torch.tensor(2)])
def test_int32_vector_rejects_a_wrong_shape(bad):
  with pytest.raises(ValueError, match=r"^target_lens must be \(2,\), got "):
    _host.int32_vector(bad, 2, "target_lens")


def test_growing_workspace_grows_only():
  ws = _host.GrowingWorkspace()
  a = ws.get("cpu", 64)
  assert a.dtype == torch.uint8 and a.numel() == 64
  assert ws.get(torch.device("cpu"), 16) is a and ws.get("cpu", 64) is a
  b = ws.get("cpu", 65)
  assert b is not a and b.numel() == 65
  assert ws.get("cpu", 1) is b


def test_char_classes_skips_the_blank_and_the_first_class_wins():
  assert _host.char_classes(["_", "a", "<EOS>", " ", "a", "b"], 0) == {"a": 1, " ": 3, "b": 5}
  assert _host.char_classes(["a", "b", "a"], 0) == {"b": 1, "a": 2}   # the blank's label is no character
  assert _host.char_classes(["_", "a"], 1) == {"_": 0}


def test_launch_enters_the_device_and_passes_the_stream_last(monkeypatch):
  events = []

  @contextlib.contextmanager
  def device(dev):
    events.append(("enter", dev))
    try:
      yield
    finally:
      events.append(("exit", dev))

  def fn(*args):
    events.append(("call", args))
    return status[0]

  monkeypatch.setattr(torch.cuda, "device", device)
  monkeypatch.setattr(_C, "stream_handle", lambda: 0)
  dev = torch.device("cuda:1")
  status = [0]
  assert _host.launch(dev, "lr_fake", fn, 7, None, 2.5) is None
  assert events == [("enter", dev), ("call", (7, None, 2.5, 0)), ("exit", dev)]
  status[0] = _C.LR_ERR_UNSUPPORTED
  with pytest.raises(_C.LipReadingHipError, match="^lr_fake failed: .*%d" % _C.LR_ERR_UNSUPPORTED):
    _host.launch(dev, "lr_fake", fn)
  assert events[-1] == ("exit", dev)


def test_beam_decoder_holds_one_word_lm(tmp_path):
  from lipreading_amd.decoder import BeamCTCDecoder
  from lipreading_amd.lm import ArpaModel, WordLM
  path = tmp_path / "toy.arpa"
  path.write_text(TOY)
  labels = ["_", " ", "a", "b"]
  dec = BeamCTCDecoder(labels, lm_path=str(path), alpha=0.5, beta=1.0)
  assert isinstance(dec._word_lm, WordLM) and dec.lm is dec._word_lm.model and isinstance(dec.lm, ArpaModel)
  assert dec.lm.order == 3 and dec.lm.counts == [6, 5, 2]
  assert (dec.alpha, dec.beta) == (0.5, 1.0) == (dec._word_lm.alpha, dec._word_lm.beta)
  assert dec._word_lm.labels == labels and dec._word_lm.blank_index == 0
  for gone in ("_lm_blob", "_lm_roles", "_lm_dev", "_lm_tensors"):
    assert not hasattr(dec, gone)
  plain = BeamCTCDecoder(labels)
  assert plain.lm is None and plain._word_lm is None
