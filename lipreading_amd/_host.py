"""The host call layer the inference entry points share (decoder.py, align.py, spot.py, scoring.py, lm.py and
CharDecodingStep.beam_search): what stands between a caller's tensors and one call into the C ABI.  A new entry point's
front door starts from these.  Nothing here asks for a GPU tensor, so all of it is tested on the CPU
(tests/test_host_layer_cpu.py); the entry points call _C.require_cuda themselves.
"""
import torch

from . import _C


def device_key(dev):
  """(type, index) of a torch.device or a string, a bare 'cuda' resolved to the current device: the one key of every
  per-device cache."""
  if isinstance(dev, str):
    dev = torch.device(dev)
  kind, index = dev.type, dev.index
  if index is None and kind == "cuda":
    index = torch.cuda.current_device()
  return (kind, index)


class PerDevice(object):
  """What an object uploads or allocates once per device: get(dev, make) calls make(dev) the first time."""

  def __init__(self):
    self._made = {}

  def get(self, dev, make):
    key = device_key(dev)
    if key not in self._made:
      self._made[key] = make(dev)
    return self._made[key]

  def values(self):
    return self._made.values()


class GrowingWorkspace(object):
  """One uint8 buffer per device, grown to the largest size asked for.  Two streams calling concurrently on a device
  would share it: its owner is called from one stream at a time."""

  def __init__(self):
    self._buf = {}

  def get(self, dev, nbytes):
    key = device_key(dev)
    ws = self._buf.get(key)
    if ws is None or ws.numel() < nbytes:
      ws = self._buf[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def log_probs_3d(x, n_labels, what):
  """The (B, T, C) tensor the CTC kernels take: fp32 with unit class stride, batch and time strided as they come (the
  transposed view of a (T, B, C) tensor goes in as it is).  `x` itself when it already is one: no copy."""
  if x.dim() != 3:
    raise ValueError("%s must be (batch, frames, classes), got %s" % (what, tuple(x.shape)))
  if x.shape[2] > n_labels:
    raise KeyError("%s has %d classes but only %d labels" % (what, x.shape[2], n_labels))
  if x.dtype != torch.float32:
    x = x.float()
  if x.stride(2) != 1 or x.stride(0) < 0 or x.stride(1) < 0:
    x = x.contiguous()
  return x


def int32_vector(t, n, what, device=None, strided=False):
  """The (n,) int32 vector a kernel takes (sizes, target_lens, the scorer's lengths), None passed through: converted
  (and moved to `device`, if given) only when it differs, `t` itself otherwise.  Contiguous, unless the caller hands
  the kernel the stride (`strided`)."""
  if t is None:
    return None
  if t.dim() != 1 or t.shape[0] != n:
    raise ValueError("%s must be (%d,), got %s" % (what, n, tuple(t.shape)))
  if t.dtype != torch.int32 or (device is not None and t.device != device):
    t = t.to(device=t.device if device is None else device, dtype=torch.int32)
  return t if strided else t.contiguous()


def char_classes(labels, blank_index):
  """character -> class over the one-character labels: the blank's label is no character, and of two classes with the
  same label the first wins."""
  class_of = {}
  for i, l in enumerate(labels):
    if len(l) == 1 and i != blank_index:
      class_of.setdefault(l, i)
  return class_of


def launch(dev, what, fn, *args):
  """fn(*args, stream) on `dev`: under torch.cuda.device(dev), so that the stream is the current one of the device the
  tensors live on, whichever device is current for the caller.  A non-zero status raises LipReadingHipError naming
  `what`."""
  with torch.cuda.device(dev):
    _C.check(fn(*args, _C.stream_handle()), what)
