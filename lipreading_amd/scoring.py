"""Edit-distance scoring of decoded class ids on the device — `src/models/lipreader/decoder.py:44-73` (Decoder.wer /
Decoder.cer) without the strings.

The host path joins label strings per utterance and runs a pure-Python Levenshtein loop on them.  EditScorer keeps
the ids where the decoders leave them: one lr_edit_distance launch per batch scores every (hypothesis, reference)
pair and adds to device-resident totals (and, with `align=True`, to a character confusion matrix); `result()` is the
one device->host read.  The semantics are those of the host code:

  * a spelling table maps each class to its label, classes in `drop` (the '<EOS>' marker) to ''; ids expand to the
    concatenation of their spellings — `''.join(labels[i] ...)` followed by `.replace(EOS, '')`;
  * unit 'char': spaces deleted from both sides, Levenshtein over characters (Decoder.cer);
  * unit 'word': both sides split at runs of spaces, Levenshtein over words (Decoder.wer);
  * `align=True` (characters): hits / substitutions / insertions / deletions of the walk back that prefers the
    diagonal, then a deletion (reference character absent), then an insertion, and the confusion matrix
    conf[r][h] over the sorted alphabet, index K = "nothing".

There is no host fall-back: CPU tensors raise LipReadingHipError, a shape past the kernel's limits raises too.
"""
import torch

from . import _C
from . import _host
from .data import EOS

CHARS, WORDS, CHARS_ALIGN = _C.LR_EDIT_CHARS, _C.LR_EDIT_WORDS, _C.LR_EDIT_CHARS_ALIGN
OUT_FIELDS = ("status", "distance", "ref_len", "hyp_len", "hits", "sub", "ins", "dele")
TOTAL_FIELDS = ("distance", "ref_len", "hyp_len", "hits", "sub", "ins", "dele", "pairs")


def spelling_table(labels, drop=(EOS,)):
  """(symbols, spell_off, spell_sym, space_sym, max_spelling): the sorted alphabet of all spellings, each class's
  spelling as indices into it (class c: spell_sym[spell_off[c]:spell_off[c+1]]), the index of ' ' (-1 if none) and
  the longest spelling.  Raises ValueError for a label set that could spell a dropped marker out of other labels —
  there, dropping tokens and the host's string `.replace` would differ."""
  labels, drop = list(labels), tuple(drop)
  others = set(''.join(l for l in labels if l not in drop))
  for d in drop:
    if d and all(ch in others for ch in d):
      raise ValueError("every character of the dropped marker %r also occurs in another label: the labels could spell "
                       "it, and scoring ids would then differ from scoring strings" % d)
  spell = ['' if l in drop else l for l in labels]
  symbols = sorted(set(''.join(spell)))
  if not symbols:
    raise ValueError("the labels spell nothing")
  index = {ch: i for i, ch in enumerate(symbols)}
  off, sym = [0], []
  for s in spell:
    sym += [index[ch] for ch in s]
    off.append(len(sym))
  return symbols, off, sym, index.get(' ', -1), max(1, max(len(s) for s in spell))


class EditScorer(object):
  """Scores (hypothesis ids, reference ids) pairs of ONE class layout (`labels[i]` = class i's string) on the GPU."""

  def __init__(self, labels, drop=(EOS,)):
    self.labels, self.drop = list(labels), tuple(drop)
    self.symbols, self._off, self._sym, self.space_sym, self.max_spelling = spelling_table(self.labels, self.drop)
    self.K = len(self.symbols)
    self._dev = _host.PerDevice()   # (spell_off, spell_sym, totals, conf), uploaded / allocated once per device
    self._last = None               # the state of the device that scored last

  def _make_state(self, dev):
    return (torch.tensor(self._off, dtype=torch.int32, device=dev),
            torch.tensor(self._sym or [0], dtype=torch.int32, device=dev),
            torch.zeros(16, dtype=torch.int64, device=dev),
            torch.zeros((self.K + 1, self.K + 1), dtype=torch.int64, device=dev))

  def _state(self, dev):
    self._last = self._dev.get(dev, self._make_state)
    return self._last

  @staticmethod
  def _rows(ids, what):
    if ids.dim() != 2 or ids.shape[0] < 1:
      raise ValueError("%s must be (B, width) with B >= 1, got %s" % (what, tuple(ids.shape)))
    if ids.dtype != torch.int32:
      ids = ids.to(torch.int32)
    if ids.shape[1] == 0:
      ids = ids.new_zeros((ids.shape[0], 1))
    if ids.stride(1) != 1 or ids.stride(0) < 0:
      ids = ids.contiguous()
    return ids

  def score(self, hyp_ids, hyp_lens, ref_ids, ref_lens, unit='char', align=False, gate=None):
    """One launch: hyp_ids (B, Wh) / ref_ids (B, Wr) integer class ids on the GPU (any row stride: `ids[:, 0]` of a
    beam search's (B, W, T) goes in as it is), hyp_lens / ref_lens (B,).  Returns a dict of (B,) int32 device tensors
    (OUT_FIELDS; `status` is negative for a pair with an id outside the labels or a length outside its row) and adds
    the batch to the scorer's totals — unless `gate` (an int32 device tensor) holds a non-zero first element, which
    leaves totals and confusion matrix untouched.  Nothing is read back."""
    if unit not in ('char', 'word'):
      raise ValueError("unit must be 'char' or 'word', got %r" % (unit,))
    if align and unit != 'char':
      raise ValueError("the alignment is defined for unit='char' only")
    _C.require_cuda(hyp_ids, hyp_lens, ref_ids, ref_lens, gate)
    L = _C.lib()
    mode = WORDS if unit == 'word' else (CHARS_ALIGN if align else CHARS)
    hyp, ref = self._rows(hyp_ids, "hyp_ids"), self._rows(ref_ids, "ref_ids")
    B = hyp.shape[0]
    if ref.shape[0] != B:
      raise ValueError("%d hypotheses against %d references" % (B, ref.shape[0]))
    # (the kernel takes the lengths' strides: `lens[:, 0]` of a beam search goes in as it is)
    hl = _host.int32_vector(hyp_lens, B, "hyp_lens", strided=True)
    rl = _host.int32_vector(ref_lens, B, "ref_lens", strided=True)
    if gate is not None and (gate.dtype != torch.int32 or gate.numel() < 1):
      raise ValueError("gate must be an int32 tensor with at least one element")
    dev = hyp.device
    Wh, Wr = hyp.shape[1], ref.shape[1]
    nbytes = L.lr_edit_workspace_bytes(B, Wh, Wr, self.max_spelling, mode)
    if nbytes == 0:
      raise _C.LipReadingHipError(
          "lr_edit_distance: unsupported shape B=%d hyp_width=%d ref_width=%d longest spelling=%d unit=%s align=%s "
          "(at most %d expanded characters per side%s)" % (B, Wh, Wr, self.max_spelling, unit, bool(align),
                                                            2048 if align else 4096, " with the alignment" if align else ""))
    off, sym, totals, conf = self._state(dev)
    out = torch.empty((B, len(OUT_FIELDS)), dtype=torch.int32, device=dev)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _host.launch(dev, "lr_edit_distance", L.lr_edit_distance, hyp.data_ptr(), hyp.stride(0), hl.data_ptr(),
                 hl.stride(0), ref.data_ptr(), ref.stride(0), rl.data_ptr(), rl.stride(0), off.data_ptr(),
                 sym.data_ptr(), len(self.labels), self.max_spelling, self.space_sym, mode, out.data_ptr(),
                 totals.data_ptr(), conf.data_ptr(), self.K, _C.ptr(gate), ws.data_ptr(), nbytes, B, Wh, Wr)
    return {name: out[:, i] for i, name in enumerate(OUT_FIELDS)}

  def _scored(self):
    if self._last is None:
      raise _C.LipReadingHipError("EditScorer: nothing was scored yet (the totals live on the GPU that scored)")
    return self._last

  def read(self, extra=None):
    """The one device->host read: (result dict, `extra` on the host) — `extra`, an optional int64 device vector,
    rides on the same copy."""
    _, _, totals, _ = self._scored()
    host = (totals if extra is None else torch.cat((totals, extra.to(torch.int64).reshape(-1)))).cpu()
    t = host[:16].tolist()
    c, w = dict(zip(TOTAL_FIELDS, t[:8])), dict(zip(TOTAL_FIELDS, t[8:]))
    res = dict(c)
    res["cer"] = c["distance"] / max(c["ref_len"], 1)
    res["wer"] = w["distance"] / max(w["ref_len"], 1)
    res.update(("word_" + k, v) for k, v in w.items() if k in ("distance", "ref_len", "hyp_len", "pairs"))
    return res, (None if extra is None else host[16:])

  def result(self):
    """Totals since the last reset(): cer, wer, and for the character unit distance, ref_len, hyp_len, hits, sub, ins,
    dele (the last four from align=True calls only), pairs; word_distance, word_ref_len, word_hyp_len, word_pairs."""
    return self.read()[0]

  def confusion(self):
    """((K+1, K+1) int64 device tensor, symbols): conf[r][h] counts reference symbol r aligned to hypothesis symbol h
    (hits on the diagonal), conf[r][K] deletions, conf[K][h] insertions, accumulated by the align=True calls."""
    return self._scored()[3].clone(), list(self.symbols)

  def reset(self):
    for _, _, totals, conf in self._dev.values():
      totals.zero_()
      conf.zero_()
