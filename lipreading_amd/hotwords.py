"""Hotwords (contextual biasing) for BeamCTCDecoder: phrases spelled in the decoder's one-character labels, packed
once into the automaton blob lr_ctc_beam_bias_decode / lr_ctc_beam_lm_bias_decode read.  The blob's layout and the
specification are owned by lipreading_amd/csrc/lr_ctc_beam.hip."""
import ctypes
import math

import numpy as np
import torch

from . import _host


def normalise(hotwords, default_weight):
  """[(string, weight)] from a list of strings or (string, weight) pairs.  ValueError for an empty string or a weight
  that is not finite and positive."""
  out = []
  for h in hotwords:
    text, w = (h, default_weight) if isinstance(h, str) else h
    w = float(w)
    if not isinstance(text, str) or not text:
      raise ValueError("a hotword must be a non-empty string, got %r" % (text,))
    if not (math.isfinite(w) and w > 0):
      raise ValueError("the weight of hotword %r must be finite and > 0, got %r" % (text, w))
    out.append((text, w))
  return out


def spell(phrases, labels, blank_index):
  """Each phrase's class ids over the one-character labels.  ValueError for a character without a class."""
  class_of = _host.char_classes(labels, blank_index)
  ids = []
  for text, _ in phrases:
    for ch in text:
      if ch not in class_of:
        raise ValueError("hotword %r: no label spells %r" % (text, ch))
    ids.append([class_of[ch] for ch in text])
  return ids


def pack(ids, weights, anchor, n_classes):
  """The device blob (numpy uint8) of lr_ctc_beam_bias_pack for phrases given as class ids."""
  from . import _C
  L = _C.lib()
  off = np.zeros(len(ids) + 1, np.int64)
  off[1:] = np.cumsum([len(p) for p in ids])
  cls = np.asarray([c for p in ids for c in p], np.int32)
  w = np.asarray(weights, np.float32)
  vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
  nbytes = L.lr_ctc_beam_bias_pack_bytes(len(ids), vp(off), vp(cls), anchor, n_classes)
  out = np.empty(max(nbytes, 1), np.uint8)
  # the packer itself tells a bad argument from a set that is too large
  _C.check(L.lr_ctc_beam_bias_pack(vp(out), nbytes, len(ids), vp(off), vp(cls), vp(w), anchor, n_classes),
           "lr_ctc_beam_bias_pack (%d hotwords, %d characters)" % (len(ids), len(cls)))
  return out


class Hotwords(object):
  """Phrases checked, spelled and packed once for a label list; the blob is uploaded once per device."""

  def __init__(self, hotwords, labels, weight=10.0, anchor=True, blank_index=0):
    self.phrases = normalise(hotwords, weight)
    class_of = _host.char_classes(labels, blank_index)
    if anchor and " " not in class_of:
      raise ValueError("hotword_anchor=True needs a ' ' label to find the start of a word; pass hotword_anchor=False")
    self.anchor = class_of[" "] if anchor else -1
    self.ids = spell(self.phrases, labels, blank_index)
    self.blob = pack(self.ids, [w for _, w in self.phrases], self.anchor, len(labels))
    self._dev = _host.PerDevice()

  def unreachable_under(self, model):
    """The phrases with a word that is not a unigram of the ARPA `model`: the dictionary keeps them out of the beam."""
    return [text for text, _ in self.phrases if any(w not in model.word_id for w in text.split())]

  def tensor(self, dev):
    """The packed automaton on `dev`: one host->device copy, the first time."""
    return self._dev.get(dev, lambda d: torch.from_numpy(self.blob).to(d))
