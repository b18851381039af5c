"""ARPA n-gram language models for BeamCTCDecoder (the reference's `lm_path`, handed to ctcdecode's KenLM scorer) and,
as WordLM, for the attention decoder's beam searches (CharDecodingStep.beam_search(lm=...)).

KenLM is not part of this build.  Its `lmplz` writes ARPA text by default, so this module reads ARPA (plain or
gzip) into the arrays lr_ctc_beam_lm_pack takes; the device blob's layout is owned by lr_ctc_beam.hip.  KenLM's
binary formats are not read.
"""
import ctypes
import gzip
import math

import numpy as np
import torch

from . import _host

MAX_ORDER = 6                   # KenLM's default maximum; lr_ctc_beam_lm_pack's limit
KENLM_MAGIC = b"mmap lm "       # the start of every KenLM binary file (lm/binary_format.cc)
SPECIAL = ("<s>", "</s>", "<unk>")   # never in the dictionary


def is_arpa_path(path):
  return str(path).endswith((".arpa", ".arpa.gz"))


def kenlm_binary_error(path):
  return NotImplementedError("BeamCTCDecoder: lm_path=%r is not an ARPA file; KenLM's binary formats are not "
                             "supported (no KenLM here).  Pass the ARPA file instead (lmplz writes ARPA; "
                             "'.arpa' or '.arpa.gz')" % (path,))


class ArpaModel(object):
  """order; vocab (unigram strings, word id = row); counts[k-1] n-grams of order k; words (sum counts * k,) int32,
  order 1 first; log10_prob / log10_backoff (sum counts,) float64 (an absent backoff is 0)."""

  def __init__(self, order, vocab, counts, words, log10_prob, log10_backoff):
    self.order, self.vocab, self.counts = order, vocab, counts
    self.words, self.log10_prob, self.log10_backoff = words, log10_prob, log10_backoff
    self.word_id = {w: i for i, w in enumerate(vocab)}


def _open(path):
  with open(path, "rb") as f:
    head = f.read(len(KENLM_MAGIC))
  if head == KENLM_MAGIC:
    raise kenlm_binary_error(path)
  if head[:2] == b"\x1f\x8b":
    return gzip.open(path, "rt", encoding="utf-8")
  return open(path, "rt", encoding="utf-8")


def read_arpa(path):
  """Parse an ARPA file.  ValueError, naming the line, for: no \\data\\ or \\end\\; a section whose entry count
  differs from its header; a duplicate n-gram; an n-gram whose (k-1)-gram context is not listed; a word of a
  higher order that is no unigram; order > 6; malformed lines."""
  def bad(lineno, msg):
    return ValueError("%s:%d: %s" % (path, lineno, msg))

  with _open(path) as f:
    lines = f.read().split("\n")
  i, n = 0, len(lines)
  while i < n and lines[i].strip() != "\\data\\":
    i += 1
  if i == n:
    raise bad(n, "no \\data\\ section")
  i += 1
  declared = {}
  while i < n and lines[i].strip().startswith("ngram "):
    text = lines[i].strip()[6:]
    try:
      k, cnt = (int(x) for x in text.split("="))
    except ValueError:
      raise bad(i + 1, "malformed count line %r" % lines[i])
    if k > MAX_ORDER:
      raise bad(i + 1, "order %d > %d is not supported" % (k, MAX_ORDER))
    if k != len(declared) + 1 or cnt < 0:
      raise bad(i + 1, "count lines must list orders 1, 2, ... with counts >= 0")
    declared[k] = cnt
    i += 1
  if not declared:
    raise bad(i + 1, "\\data\\ lists no ngram counts")
  order = len(declared)
  seen = {}            # n-gram tuple of word ids -> row
  vocab, word_id = [], {}
  words, lp, bow = [], [], []
  ended = False
  k = 0
  while i < n:
    s = lines[i].strip()
    if not s:
      i += 1
      continue
    if s == "\\end\\":
      ended = True
      break
    if not (s.startswith("\\") and s.endswith("-grams:")):
      raise bad(i + 1, "expected a section header, got %r" % s)
    try:
      kk = int(s[1:-7])
    except ValueError:
      raise bad(i + 1, "malformed section header %r" % s)
    if kk != k + 1 or kk > order:
      raise bad(i + 1, "section %r out of order" % s)
    k = kk
    i += 1
    got = 0
    while i < n:
      s = lines[i].strip()
      if s.startswith("\\"):
        break
      if not s:
        i += 1
        continue
      parts = s.split()
      if len(parts) not in (k + 1, k + 2):
        raise bad(i + 1, "a %d-gram line needs %d or %d fields" % (k, k + 1, k + 2))
      try:
        p = float(parts[0])
        b = float(parts[k + 1]) if len(parts) == k + 2 else 0.0
      except ValueError:
        raise bad(i + 1, "malformed number in %r" % s)
      toks = parts[1:k + 1]
      if k == 1:
        if toks[0] in word_id:
          raise bad(i + 1, "duplicate 1-gram %r" % toks[0])
        word_id[toks[0]] = len(vocab)
        vocab.append(toks[0])
        ids = (word_id[toks[0]],)
      else:
        try:
          ids = tuple(word_id[t] for t in toks)
        except KeyError as e:
          raise bad(i + 1, "word %s of a %d-gram is not a unigram" % (e, k))
        if ids in seen:
          raise bad(i + 1, "duplicate %d-gram %r" % (k, " ".join(toks)))
        if ids[:-1] not in seen:
          raise bad(i + 1, "the context %r of this %d-gram is not listed" % (" ".join(toks[:-1]), k))
      seen[ids] = len(lp)
      words.extend(ids)
      lp.append(p)
      bow.append(b)
      got += 1
      i += 1
    if got != declared[k]:
      raise bad(i + 1 if i < n else n, "\\%d-grams: holds %d entries, \\data\\ declares %d" % (k, got, declared[k]))
  if not ended:
    raise bad(n, "no \\end\\")
  if k != order:
    raise bad(i + 1, "\\data\\ declares order %d but the file has sections up to %d" % (order, k))
  counts = [declared[q] for q in range(1, order + 1)]
  return ArpaModel(order, vocab, counts, np.asarray(words, np.int32), np.asarray(lp, np.float64),
                   np.asarray(bow, np.float64))


def class_roles(labels, blank_index):
  """Roles of lr_ctc_beam_lm_decode: 2 for the ' ' label, 1 for every other one-character label but the blank,
  0 (transparent) for the rest.  ValueError without a ' ' label or with two identical one-character labels."""
  singles = [l for l in labels if len(l) == 1]
  if " " not in labels:
    raise ValueError("a language model needs a ' ' label to separate words")
  if len(set(singles)) != len(singles):
    raise ValueError("a language model needs distinct one-character labels: %r" % labels)
  roles = []
  for i, l in enumerate(labels):
    roles.append(2 if l == " " else (1 if len(l) == 1 and i != blank_index else 0))
  return roles


def dictionary(model, labels, roles):
  """(dict_word, dict_off, dict_cls): the vocabulary words whose every character is a word-character label, spelled
  in class ids.  ValueError if no word can be reached."""
  cls_of = {l: i for i, l in enumerate(labels) if roles[i] == 1}
  dw, off, cl = [], [0], []
  for wid, w in enumerate(model.vocab):
    if w in SPECIAL:
      continue
    try:
      spell = [cls_of[ch] for ch in w]
    except KeyError:
      continue
    dw.append(wid)
    cl.extend(spell)
    off.append(len(cl))
  if not dw:
    raise ValueError("no word of the language model can be spelled with these labels (upper- vs lower-case?)")
  return np.asarray(dw, np.int32), np.asarray(off, np.int64), np.asarray(cl, np.int32)


def pack(model, labels, blank_index):
  """The device blob (numpy uint8) and the class roles for lr_ctc_beam_lm_decode."""
  from . import _C
  roles = class_roles(labels, blank_index)
  dw, off, cl = dictionary(model, labels, roles)
  L = _C.lib()
  counts = np.asarray(model.counts, np.int64)
  cp = counts.ctypes.data_as(ctypes.c_void_p)
  nbytes = L.lr_ctc_beam_lm_pack_bytes(model.order, cp, int(off[-1]))
  if nbytes == 0:
    raise _C.LipReadingHipError("lr_ctc_beam_lm_pack: unsupported model (order %d, %d words)"
                                % (model.order, len(model.vocab)))
  out = np.empty(nbytes, np.uint8)
  vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
  bos = model.word_id.get("<s>", -1)
  _C.check(L.lr_ctc_beam_lm_pack(vp(out), nbytes, model.order, cp, vp(model.words), vp(model.log10_prob),
                                 vp(model.log10_backoff), bos, len(dw), vp(dw), vp(off), vp(cl), len(labels)),
           "lr_ctc_beam_lm_pack")
  return out, roles


class WordLM(object):
  """An ARPA word model read, checked and packed once for a label list, for CharDecodingStep.beam_search(lm=...):
  `labels` are the CTC classes' (decoder.ctc_labels(char2idx): the decoder's token v is class v + 1, so one packed
  model serves BeamCTCDecoder and the attention searches), `alpha` weighs the model's log-probabilities and `beta` is
  added per word, as in BeamCTCDecoder.  ValueError for labels without a ' ' or with repeated one-character labels, or
  for non-finite weights; NotImplementedError for a path that is not ARPA."""

  def __init__(self, path, labels, alpha=0.0, beta=0.0, blank_index=0):
    if not is_arpa_path(path):
      raise kenlm_binary_error(path)
    alpha, beta = float(alpha), float(beta)
    if not (math.isfinite(alpha) and math.isfinite(beta)):
      raise ValueError("alpha and beta must be finite")
    self.labels, self.blank_index = list(labels), int(blank_index)
    if not 0 <= self.blank_index < len(self.labels):
      raise ValueError("blank_index %d outside the %d labels" % (blank_index, len(self.labels)))
    class_roles(self.labels, self.blank_index)   # the label checks come before the file is read
    self.alpha, self.beta = alpha, beta
    self.model = read_arpa(path)
    self.blob, self.roles = pack(self.model, self.labels, self.blank_index)
    self._dev = _host.PerDevice()   # (blob, roles) tensors, uploaded once per device

  def tensors(self, dev):
    """The packed model and the class roles on `dev`: one host->device copy each, the first time."""
    return self._dev.get(dev, lambda d: (torch.from_numpy(self.blob).to(d),
                                         torch.tensor(self.roles, dtype=torch.int32, device=d)))
