"""CTC decoders — drop-in for `src/models/lipreader/decoder.py` (Decoder :23, BeamCTCDecoder :90,
GreedyDecoder :146).

GreedyDecoder.decode keeps the reference's contract — `(strings, offsets)` with
`strings[b] == [str]` and `offsets[b] == [IntTensor]` — but the per-frame Python loop with one
`.item()` per element (decoder.py:168-169) becomes one kernel (argmax + collapse + ordered
compaction) and a single device->host copy of the kept ids.

BeamCTCDecoder keeps the reference's constructor and `(strings, offsets)` contract, but the
search ctcdecode runs on CPU threads after `probs.cpu()` (decoder.py:139) runs on the GPU
(lr_ctc_beam_decode: prefix beam search) with one device->host copy.  An ARPA `lm_path` adds ctcdecode's word
language model (lr_ctc_beam_lm_decode; the reader is lipreading_amd/lm.py); `hotwords` tell either search which
words to expect (lr_ctc_beam_bias_decode, lr_ctc_beam_lm_bias_decode; lipreading_amd/hotwords.py).
BeamCTCDecoder.stream() is the same search fed chunk by chunk (BeamStream on lr_ctc_beam_stream_*): partial
transcripts with the characters that are already final, and at the end decode's answer bit for bit.
"""
import warnings

import torch

from . import _C
from . import _host
from . import hotwords as hw
from . import lm


def _edit_distance(a, b):
  """Levenshtein distance; the reference delegates to the `Levenshtein` package (decoder.py:18)."""
  prev = list(range(len(b) + 1))
  for i, ca in enumerate(a, 1):
    cur = [i]
    for j, cb in enumerate(b, 1):
      cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
    prev = cur
  return prev[-1]


class Decoder(object):
  """decoder.py:23-88: label bookkeeping plus WER/CER helpers."""

  def __init__(self, labels, blank_index=0):
    self.labels = labels
    self.int_to_char = dict([(i, c) for (i, c) in enumerate(labels)])
    self.blank_index = blank_index
    space_index = len(labels)  # out-of-bounds sentinel when there is no ' ' (decoder.py:38)
    if ' ' in labels:
      space_index = labels.index(' ')
    self.space_index = space_index

  def wer(self, s1, s2):
    """Word-level edit distance (decoder.py:44-62)."""
    b = set(s1.split() + s2.split())
    word2char = dict(zip(b, range(len(b))))
    w1 = [chr(word2char[w]) for w in s1.split()]
    w2 = [chr(word2char[w]) for w in s2.split()]
    return _edit_distance(''.join(w1), ''.join(w2))

  def cer(self, s1, s2):
    """Character-level edit distance with spaces removed (decoder.py:64-73)."""
    s1, s2 = s1.replace(' ', ''), s2.replace(' ', '')
    return _edit_distance(s1, s2)

  def decode(self, probs, sizes=None):
    raise NotImplementedError

  def scorer(self):
    """An EditScorer over this decoder's labels: decode_ids' output -> CER / WER on the device, no strings
    (lipreading_amd/scoring.py)."""
    from .scoring import EditScorer
    return EditScorer(self.labels)


class BeamCTCDecoder(Decoder):
  """decoder.py:90-143 on lr_ctc_beam_decode.  `log_probs_input` is ctcdecode's later keyword: True when
  `probs` holds log-probabilities (VideoEncoder's output).  Classes are compared by index, as ctcdecode does:
  no canonical-label mapping.  `num_processes`, and `alpha`/`beta` without a language model, are accepted and
  ignored, as ctcdecode ignores them.

  `lm_path` ending in '.arpa' or '.arpa.gz' loads an ARPA n-gram word model (lipreading_amd/lm.py); `alpha` weighs
  its log-probabilities and `beta` is added per word, as in ctcdecode (the specification is lr_ctc_beam.hip's).
  Any other path, or a KenLM binary file, raises NotImplementedError.  The labels then need a ' ' and distinct
  one-character labels (ValueError otherwise).

  `hotwords` (strings, or (string, weight) pairs; `hotword_weight` for the bare strings) raise the score of
  hypotheses that spell them while the search runs, a half-spelled one in proportion (lr_ctc_beam_bias_decode,
  DESIGN.md §13.2).  They are spelled in the one-character labels (ValueError for a character without one);
  `hotword_anchor` lets them match only at the start of a word and needs a ' ' label.  With a language model the
  dictionary still holds: hotwords with a word the model does not list cannot be reached, and are named in a
  warning.  None or [] is the search without hotwords."""

  def __init__(self, labels, lm_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0, beam_width=100,
               num_processes=4, blank_index=0, log_probs_input=False, hotwords=None, hotword_weight=10.0,
               hotword_anchor=True):
    super(BeamCTCDecoder, self).__init__(labels, blank_index)
    if lm_path is not None and not lm.is_arpa_path(lm_path):
      # decided by the name, before the file is opened
      raise lm.kenlm_binary_error(lm_path)
    if not 0 <= blank_index < len(labels):
      raise ValueError("blank_index %d outside the %d labels" % (blank_index, len(labels)))
    if beam_width < 1 or cutoff_top_n < 1:
      raise ValueError("beam_width and cutoff_top_n must be >= 1")
    self.cutoff_top_n = int(cutoff_top_n)
    self.cutoff_prob = float(cutoff_prob)
    self.beam_width = int(beam_width)
    self.log_probs_input = bool(log_probs_input)
    self.lm = self._word_lm = None
    if lm_path is not None:
      # WordLM checks the weights, then the labels, then reads, packs and (once per device) uploads the file
      self._word_lm = lm.WordLM(lm_path, labels, alpha=alpha, beta=beta, blank_index=blank_index)
      self.lm, self.alpha, self.beta = self._word_lm.model, self._word_lm.alpha, self._word_lm.beta
    self._hotwords = None
    if hotwords:
      self._hotwords = hw.Hotwords(hotwords, labels, weight=hotword_weight, anchor=hotword_anchor,
                                   blank_index=blank_index)
      lost = self._hotwords.unreachable_under(self.lm) if self.lm is not None else []
      if lost:
        warnings.warn("hotwords with a word the language model does not list cannot be decoded: %s"
                      % ", ".join(repr(t) for t in lost))

  def decode_ids(self, probs, sizes=None):
    """Device part: probs (B,T,C) -> (ids (B,W,T) int32, offsets (B,W,T) int32, lens (B,W) int32,
    scores (B,W) fp32 = -log P, ascending) on the GPU.  Entries past lens are -1."""
    _C.require_cuda(probs, sizes)
    L = _C.lib()
    probs = _host.log_probs_3d(probs, len(self.labels), "probs")
    B, T, C = probs.shape
    W, n = self.beam_width, self.cutoff_top_n
    dev = probs.device
    ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
    off = torch.empty((B, W, T), dtype=torch.int32, device=dev)
    lens = torch.empty((B, W), dtype=torch.int32, device=dev)
    scores = torch.empty((B, W), dtype=torch.float32, device=dev)
    sz = _host.int32_vector(sizes, B, "sizes", device=dev)
    nbytes = L.lr_ctc_beam_workspace_bytes(B, T, C, W, n)
    if nbytes == 0:
      raise _C.LipReadingHipError("lr_ctc_beam_decode: unsupported shape B=%d T=%d C=%d beam_width=%d "
                                  "cutoff_top_n=%d" % (B, T, C, W, n))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    head = (probs.data_ptr(), probs.stride(0), probs.stride(1), _C.ptr(sz), int(self.log_probs_input), n,
            self.cutoff_prob, W, self.blank_index)
    tail = (ids.data_ptr(), off.data_ptr(), lens.data_ptr(), scores.data_ptr(), ws.data_ptr(), nbytes, B, T, C)
    bias = None if self._hotwords is None else self._hotwords.tensor(dev)
    if self._word_lm is not None and bias is not None:
      blob, roles = self._word_lm.tensors(dev)
      _host.launch(dev, "lr_ctc_beam_lm_bias_decode", L.lr_ctc_beam_lm_bias_decode,
                   *head, blob.data_ptr(), roles.data_ptr(), self.alpha, self.beta, bias.data_ptr(), *tail)
    elif bias is not None:
      _host.launch(dev, "lr_ctc_beam_bias_decode", L.lr_ctc_beam_bias_decode, *head, bias.data_ptr(), *tail)
    elif self._word_lm is not None:
      blob, roles = self._word_lm.tensors(dev)
      _host.launch(dev, "lr_ctc_beam_lm_decode", L.lr_ctc_beam_lm_decode,
                   *head, blob.data_ptr(), roles.data_ptr(), self.alpha, self.beta, *tail)
    else:
      _host.launch(dev, "lr_ctc_beam_decode", L.lr_ctc_beam_decode, *head, *tail)
    return ids, off, lens, scores

  def stream(self, batch, max_frames, device):
    """A BeamStream: this decoder's search over `batch` utterance slots fed chunk by chunk, up to `max_frames`
    frames per slot (the trie's tables are sized for them; there is no compaction).  It keeps the decoder's
    parameters, language model and hotwords; fed all frames it answers what decode answers, bit for bit."""
    return BeamStream(self, batch, max_frames, device)

  def _strings(self, ids, off, lens):
    """decode's (strings, offsets) from device (B,W,T) ids / offsets and (B,W) lens: one device->host copy."""
    B, W, T = ids.shape
    host = torch.cat((ids.view(B, -1), off.view(B, -1), lens), dim=1).cpu()   # the one device->host copy
    off = host[:, W * T:2 * W * T].view(B, W, T)
    ids, lens = host[:, :W * T].view(B, W, T).tolist(), host[:, 2 * W * T:].tolist()
    chars = self.int_to_char
    strings, offsets = [], []
    for b in range(B):
      strings.append([''.join([chars[i] for i in ids[b][p][:n]]) for p, n in enumerate(lens[b])])
      offsets.append([off[b, p, :n].clone() if n > 0 else torch.tensor([], dtype=torch.int)
                      for p, n in enumerate(lens[b])])
    return strings, offsets

  def decode(self, probs, sizes=None):
    """decoder.py:128-143: probs (B,T,C) -> (strings, offsets); strings[b] holds beam_width strings, best
    first ('' for empty beam slots), offsets[b] the matching IntTensors of frame indices."""
    ids, off, lens, _ = self.decode_ids(probs, sizes)
    return self._strings(ids, off, lens)


class BeamStream(object):
  """A resumable search of a BeamCTCDecoder (lr_ctc_beam_stream_*): `batch` independent slots, each
  fed its utterance in chunks of any lengths.  The state lives in one device tensor; feed() is two launches, every
  read one, and a read changes nothing.  Use BeamCTCDecoder.stream()."""

  def __init__(self, decoder, batch, max_frames, device):
    device = torch.device(device)
    if device.type != "cuda":
      raise _C.LipReadingHipError(
          "lipreading_amd ops run on the MI355X only; got device %s (no CPU fallback)" % device)
    if int(batch) < 1 or int(max_frames) < 1:
      raise ValueError("batch and max_frames must be >= 1, got %d and %d" % (batch, max_frames))
    self.decoder, self.batch, self.max_frames = decoder, int(batch), int(max_frames)
    d = decoder
    L = _C.lib()
    self._lm = d._word_lm is not None
    self._bias = d._hotwords is not None
    nbytes = L.lr_ctc_beam_stream_state_bytes(self.batch, self.max_frames, d.beam_width, int(self._lm),
                                              int(self._bias))
    if nbytes == 0:
      raise _C.LipReadingHipError("lr_ctc_beam_stream_reset: unsupported shape B=%d max_frames=%d beam_width=%d"
                                  % (self.batch, self.max_frames, d.beam_width))
    self.device = torch.device(device.type, _host.device_key(device)[1])
    # zeroed, so that the bytes the search never writes are equal from session to session
    self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
    self._ws = _host.GrowingWorkspace()
    self._blob = self._roles = self._biasblob = None
    if self._lm:
      self._blob, self._roles = d._word_lm.tensors(self.device)
    if self._bias:
      self._biasblob = d._hotwords.tensor(self.device)
    self.reset()

  def reset(self, mask=None):
    """Slots with a non-zero `mask` entry ((batch,) on the device; None: all) restart from the empty prefix with
    0 frames; the others keep every bit."""
    _C.require_cuda(mask)
    m = _host.int32_vector(mask if mask is None or mask.dtype != torch.bool else mask.int(), self.batch, "mask",
                           device=self.device)
    L = _C.lib()
    _host.launch(self.device, "lr_ctc_beam_stream_reset", L.lr_ctc_beam_stream_reset, self.state.data_ptr(),
                 self.state.numel(), _C.ptr(m), self.batch, self.max_frames, self.decoder.beam_width, int(self._lm),
                 int(self._bias), _C.ptr(self._blob), _C.ptr(self._biasblob))

  def feed(self, probs, sizes=None):
    """One advance: probs (batch, chunk_T, C), slot b consuming its first sizes[b] frames (None: all).  Strided
    views such as all_probs[:, t0:t1] go in without a copy."""
    _C.require_cuda(probs, sizes)
    d = self.decoder
    L = _C.lib()
    probs = _host.log_probs_3d(probs, len(d.labels), "probs")
    B, T, C = probs.shape
    if B != self.batch:
      raise ValueError("probs holds %d utterances, the session %d" % (B, self.batch))
    if C != len(d.labels):
      raise ValueError("probs has %d classes, the decoder %d labels" % (C, len(d.labels)))
    sz = _host.int32_vector(sizes, B, "sizes", device=self.device)
    if T == 0:
      return self
    W, n = d.beam_width, d.cutoff_top_n
    nbytes = L.lr_ctc_beam_stream_workspace_bytes(B, T, C, W, n)
    if nbytes == 0:
      raise _C.LipReadingHipError("lr_ctc_beam_stream_advance: unsupported shape B=%d chunk_T=%d C=%d beam_width=%d "
                                  "cutoff_top_n=%d" % (B, T, C, W, n))
    ws = self._ws.get(self.device, nbytes)
    alpha, beta = (d.alpha, d.beta) if self._lm else (0.0, 0.0)
    _host.launch(self.device, "lr_ctc_beam_stream_advance", L.lr_ctc_beam_stream_advance, probs.data_ptr(),
                 probs.stride(0), probs.stride(1), _C.ptr(sz), int(d.log_probs_input), n, d.cutoff_prob, W,
                 d.blank_index, _C.ptr(self._blob), _C.ptr(self._roles), alpha, beta, _C.ptr(self._biasblob),
                 self.state.data_ptr(), self.state.numel(), self.max_frames, ws.data_ptr(), ws.numel(), B, T, C)
    return self

  def read_ids(self, n_out=1, width=None):
    """What decode_ids would answer if the stream ended now, on the device: (ids (B,n_out,width) int32, offsets
    likewise, lens (B,n_out) the true lengths, scores (B,n_out), stable (B,), frames (B,), status (B,)).  `width`
    None is max_frames.  The first stable[b] ids of slot b's best hypothesis are final.  The status bits
    (_C.LR_BEAM_STREAM_OVERFLOW, _C.LR_BEAM_STREAM_MISMATCH) are the caller's to look at."""
    d = self.decoder
    n_out = int(n_out)
    width = self.max_frames if width is None else int(width)
    if not 1 <= n_out <= d.beam_width:
      raise ValueError("n_out must be in [1, beam_width = %d], got %d" % (d.beam_width, n_out))
    if width < 1:
      raise ValueError("width must be >= 1, got %d" % width)
    B, dev = self.batch, self.device
    ids = torch.empty((B, n_out, width), dtype=torch.int32, device=dev)
    off = torch.empty((B, n_out, width), dtype=torch.int32, device=dev)
    lens = torch.empty((B, n_out), dtype=torch.int32, device=dev)
    scores = torch.empty((B, n_out), dtype=torch.float32, device=dev)
    meta = torch.empty((3, B), dtype=torch.int32, device=dev)
    self._read_into(n_out, width, ids, off, lens, scores, meta[0], meta[1], meta[2])
    return ids, off, lens, scores, meta[0], meta[1], meta[2]

  def _read_into(self, n_out, width, ids, off, lens, scores, stable, frames, status):
    d = self.decoder
    alpha, beta = (d.alpha, d.beta) if self._lm else (0.0, 0.0)
    L = _C.lib()
    _host.launch(self.device, "lr_ctc_beam_stream_read", L.lr_ctc_beam_stream_read, self.state.data_ptr(),
                 self.state.numel(), _C.ptr(self._blob), alpha, beta, _C.ptr(self._biasblob), n_out, width,
                 ids.data_ptr(), off.data_ptr(), lens.data_ptr(), scores.data_ptr(), stable.data_ptr(),
                 frames.data_ptr(), status.data_ptr(), self.batch)

  def _raise_for(self, status):
    for b, s in enumerate(status):
      names = [name for name, bit in (("overflow: frames past max_frames = %d were offered" % self.max_frames,
                                       _C.LR_BEAM_STREAM_OVERFLOW),
                                      ("mismatch: a call's configuration is not the session's",
                                       _C.LR_BEAM_STREAM_MISMATCH)) if s & bit]
      if names:
        raise _C.LipReadingHipError("lr_ctc_beam_stream: slot %d has status %d (%s)" % (b, s, "; ".join(names)))

  def partial(self):
    """Per slot (best string so far, how many of its leading characters are final), one device->host copy.  A
    status bit raises LipReadingHipError naming the slot."""
    ids, _, lens, _, stable, _, status = self.read_ids(1, self.max_frames)
    host = torch.cat((ids[:, 0], lens, stable[:, None], status[:, None]), dim=1).cpu().tolist()
    T = self.max_frames
    self._raise_for([row[T + 2] for row in host])
    chars = self.decoder.int_to_char
    return [(''.join(chars[i] for i in row[:row[T]]), row[T + 1]) for row in host]

  def result(self):
    """(strings, offsets) in BeamCTCDecoder.decode's contract, all beam_width hypotheses, as if the stream ended
    now; the width is the most frames any slot consumed (at least 1).  A status bit raises LipReadingHipError."""
    frames, status = self.read_ids(1, 1)[5:]
    fs = torch.stack((frames, status)).cpu().tolist()
    self._raise_for(fs[1])
    ids, off, lens = self.read_ids(self.decoder.beam_width, max(1, max(fs[0])))[:3]
    return self.decoder._strings(ids, off, lens)


class ChunkedBeamDecoder(object):
  """A BeamCTCDecoder's decode / decode_ids run through a session in chunks of `chunk` frames, one read per chunk: by
  construction the same answers, plus the record of what a live caller would have seen.  commit_delay() turns the
  record into analysis.commit_delay_stats' dict and clears it.  What the driver's --stream_chunk evaluates with."""

  def __init__(self, decoder, chunk):
    if int(chunk) < 1:
      raise ValueError("chunk must be >= 1, got %d" % chunk)
    self.decoder, self.chunk = decoder, int(chunk)
    self._seen = []   # per batch, on the device: reads (R, 2, B), the best hypothesis's offsets (B, T) and length (B,)

  def __getattr__(self, name):   # labels, scorer(), cer() ...: the decoder's
    return getattr(self.decoder, name)

  def decode_ids(self, probs, sizes=None):
    _C.require_cuda(probs, sizes)
    B, T = probs.shape[0], probs.shape[1]
    st = self.decoder.stream(B, max(T, 1), probs.device)
    sz = _host.int32_vector(sizes, B, "sizes", device=probs.device)
    reads = []
    for t0 in range(0, T, self.chunk):
      t1 = min(T, t0 + self.chunk)
      st.feed(probs[:, t0:t1], None if sz is None else (sz - t0).clamp_(0, t1 - t0))
      got = st.read_ids(1, 1)
      reads.append(torch.stack((got[5], got[4])))
    ids, off, lens, scores = st.read_ids(self.decoder.beam_width, max(T, 1))[:4]
    total = sz if sz is not None else torch.full((B,), T, dtype=torch.int32, device=probs.device)
    if reads:
      self._seen.append((torch.stack(reads), off[:, 0], lens[:, 0], total.clamp(0, T)))
    return ids, off, lens, scores

  def decode(self, probs, sizes=None):
    ids, off, lens, _ = self.decode_ids(probs, sizes)
    return self.decoder._strings(ids, off, lens)

  def commit_delay(self):
    from .analysis import commit_delay, commit_delay_stats
    per = []
    for reads, off, lens, total in self._seen:
      reads, off, lens, total = reads.cpu().tolist(), off.cpu().tolist(), lens.cpu().tolist(), total.cpu().tolist()
      for b, n in enumerate(lens):
        per.append(commit_delay([(r[0][b], r[1][b]) for r in reads], off[b][:n], total[b]))
    self._seen = []
    return commit_delay_stats(per)


class GreedyDecoder(Decoder):
  def __init__(self, labels, blank_index=0):
    super(GreedyDecoder, self).__init__(labels, blank_index)
    # the reference compares characters, not indices (decoder.py:167-171): classes that share
    # a label string collapse together.  canonical index = first class with that string.
    first = {}
    canon = [first.setdefault(c, i) for i, c in enumerate(labels)]
    self._canon = canon if canon != list(range(len(labels))) else None
    self._canon_dev = _host.PerDevice()   # the map, uploaded once per device

  def decode_ids(self, probs, sizes=None):
    """Device part: returns (ids (B,T) int32, offsets (B,T) int32, lens (B,) int32) on the GPU."""
    _C.require_cuda(probs, sizes)
    L = _C.lib()
    probs = _host.log_probs_3d(probs, len(self.labels), "probs")
    B, T, C = probs.shape
    dev = probs.device
    ids = torch.empty((B, T), dtype=torch.int32, device=dev)
    off = torch.empty((B, T), dtype=torch.int32, device=dev)
    lens = torch.empty((B,), dtype=torch.int32, device=dev)
    sz = _host.int32_vector(sizes, B, "sizes", device=dev)
    cmap = None
    if self._canon is not None:
      cmap = self._canon_dev.get(dev, lambda d: torch.tensor(self._canon, dtype=torch.int32, device=d))
    blank = self.blank_index if self._canon is None else self._canon[self.blank_index]
    _host.launch(dev, "lr_ctc_greedy_decode", L.lr_ctc_greedy_decode, probs.data_ptr(), probs.stride(0),
                 probs.stride(1), _C.ptr(sz), _C.ptr(cmap), ids.data_ptr(), off.data_ptr(), lens.data_ptr(), B, T, C,
                 blank)
    return ids, off, lens

  def decode(self, probs, sizes=None):
    """decoder.py:182-197: probs (B,T,C) -> ([[str]], [[IntTensor offsets]])."""
    ids, off, lens = self.decode_ids(probs, sizes)
    ids, off, lens = ids.cpu(), off.cpu(), lens.cpu().tolist()
    strings, offsets = [], []
    for b, n in enumerate(lens):
      chars = [self.int_to_char[i] for i in ids[b, :n].tolist()]
      if chars and self.space_index >= len(self.labels):
        # decoder.py:174 indexes labels[space_index] for every kept character
        raise IndexError("list index out of range")
      strings.append([''.join(chars)])
      offsets.append([off[b, :n].clone().to(torch.int)])
    return strings, offsets


def ctc_labels(char2idx):
  """Label list for the live model's V'=V+1 class layout (better_model.py:38,43-45): index 0 is
  the CTC blank '_', index i+1 the character with id i.  The reference defines none because its
  greedy decoder has no live caller."""
  inv = {v: k for k, v in char2idx.items()}
  return ['_'] + [inv[i] for i in range(len(inv))]
