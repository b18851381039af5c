"""CTC keyword spotting on the device: is a keyword spoken anywhere in a clip, where, and how well (BUILD-DEFINED,
DESIGN.md §20; the reference has no spotter).

The decoders say what a clip says and CTCAligner says when a KNOWN caption is spoken.  KeywordSpotter answers for a
fixed list of keywords and every clip of a batch: one lr_ctc_spot launch runs, per (clip, keyword), a dynamic programme
with a free start and a free end over the keyword's 2L-1 states (its tokens and the blanks between them), scored in
frame ratios lp[t][c] - max_c lp[t][c] — the log-ratio of the keyword's path to the greedy path on the same frames, 0
where the greedy decoder reads exactly this keyword — and picks up to `max_hits` non-overlapping spans, best first:

  * hit_score (B, K, H) fp32, hit_start / hit_end (B, K, H) int32: the span [start, end) in frames, padded with
    -inf / -1 / -1; n_hits (B, K); status (B, K): 0, BAD_ID, BAD_LENGTH;
  * with trace=True also end_score / end_start (B, K, T): the score and start of the best span ENDING on each frame.

Everything the kernel computes is a sum of fp32 ratios.  The per-character mean score / L, confidence =
exp(score / L) and seconds are made here on the host after the read.  There is no host fall-back: CPU tensors raise
LipReadingHipError.
"""
import math

import numpy as np
import torch

from . import _C
from . import _host

BAD_ID, BAD_LENGTH = _C.LR_SPOT_BAD_ID, _C.LR_SPOT_BAD_LENGTH
MAX_T, MAX_KW_LEN, MAX_HITS = _C.LR_SPOT_MAX_T, _C.LR_SPOT_MAX_KW_LEN, _C.LR_SPOT_MAX_HITS


class KeywordSpotter(object):
  """Spots `keywords` (strings over `labels`; a phrase with ' ' is an ordinary keyword) in clips of ONE class layout
  (`labels[i]` = class i's string, blank at `blank_index`).  `min_confidence` = p in (0, 1] keeps the spans whose mean
  per-character ratio is at least log p: min_scores[k] = float32(L_k * log p).  `fps` turns frames into seconds."""

  def __init__(self, labels, keywords, blank_index=0, fps=29.97, max_hits=4, min_confidence=None):
    self.labels = list(labels)
    if not 0 <= blank_index < len(self.labels):
      raise ValueError("blank_index %d outside the %d labels" % (blank_index, len(self.labels)))
    if not 1 <= int(max_hits) <= MAX_HITS:
      raise ValueError("max_hits must be in [1, %d], got %r" % (MAX_HITS, max_hits))
    if min_confidence is not None and not 0.0 < float(min_confidence) <= 1.0:
      raise ValueError("min_confidence must be in (0, 1], got %r" % (min_confidence,))
    self.blank_index, self.fps, self.max_hits = int(blank_index), float(fps), int(max_hits)
    self.min_confidence = None if min_confidence is None else float(min_confidence)
    class_of = _host.char_classes(self.labels, self.blank_index)
    self.keywords = list(keywords)
    if not self.keywords:
      raise ValueError("at least one keyword")
    rows = []
    for s in self.keywords:
      if not isinstance(s, str) or not 1 <= len(s) <= MAX_KW_LEN:
        raise ValueError("a keyword has 1 to %d characters, got %r" % (MAX_KW_LEN, s))
      try:
        rows.append([class_of[ch] for ch in s])
      except KeyError as e:
        raise KeyError("character %r of keyword %r has no class" % (e.args[0], s))
    K = len(rows)
    self.lengths = np.array([len(r) for r in rows], np.int32)
    self.ids = np.zeros((K, int(self.lengths.max())), np.int32)
    for k, r in enumerate(rows):
      self.ids[k, :len(r)] = r
    self.min_scores = None
    if self.min_confidence is not None:
      self.min_scores = np.array([np.float32(int(L) * math.log(self.min_confidence)) for L in self.lengths], np.float32)
    # the kernel packs keywords of similar length side by side in a wave: hand them over sorted by length and put the
    # outputs back into the caller's order
    self._order = np.argsort(self.lengths, kind="stable")
    self._sorted = bool((self._order == np.arange(K)).all())
    self._dev = _host.PerDevice()   # (ids, lengths, min_scores, inverse order), uploaded once per device
    self._ws = _host.GrowingWorkspace()

  def seconds(self, frame):
    return frame / self.fps

  def _upload(self, dev):
    o = self._order
    inv = np.empty_like(o)
    inv[o] = np.arange(len(o))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (up(self.ids[o]), up(self.lengths[o]), None if self.min_scores is None else up(self.min_scores[o]),
            None if self._sorted else up(inv.astype(np.int64)))

  def spot_ids(self, log_probs, sizes=None, trace=False):
    """One launch, nothing read back: log_probs (B, T, C) fp32 on the GPU (any batch / time strides with unit class
    stride: the transposed view of a (T, B, C) tensor goes in as it is), sizes (B,) or None (= T).  Returns a dict of
    device tensors indexed by the keyword's position in `keywords`: hit_score (B, K, H) fp32, hit_start, hit_end
    (B, K, H) int32, n_hits, status (B, K) int32, and with trace=True end_score (B, K, T) fp32, end_start (B, K, T)
    int32.  ValueError for a shape past the kernel's limits.  The spotter keeps one workspace per device: call it from
    one stream at a time."""
    _C.require_cuda(log_probs, sizes)
    L = _C.lib()
    lp = _host.log_probs_3d(log_probs, len(self.labels), "log_probs")
    B, T, C = lp.shape
    sz = _host.int32_vector(sizes, B, "sizes")
    K, W = self.ids.shape
    H = self.max_hits
    nbytes = L.lr_ctc_spot_workspace_bytes(B, T, C, K, W, H) if B > 0 and self.blank_index < C else 0
    if nbytes == 0:
      raise ValueError("lr_ctc_spot: unsupported shape B=%d T=%d C=%d keywords=%d longest=%d max_hits=%d blank=%d (at "
                       "most %d frames, %d tokens a keyword and %d hits; at least one sample, two classes and the "
                       "blank among them)" % (B, T, C, K, W, H, self.blank_index, MAX_T, MAX_KW_LEN, MAX_HITS))
    dev = lp.device
    ids, lens, thr, inv = self._dev.get(dev, self._upload)
    # (the trace goes straight into end_score / end_start)
    ws = self._ws.get(dev, 16 if trace else nbytes)
    # one int32 buffer per shape, so that putting the keywords back in order is one gather each: the scores ride along
    # bit for bit
    hit = torch.empty((3, B, K, H), dtype=torch.int32, device=dev)     # score bits, start, end
    per = torch.empty((2, B, K), dtype=torch.int32, device=dev)        # n_hits, status
    end = torch.empty((2, B, K, T), dtype=torch.int32, device=dev) if trace else None
    _host.launch(dev, "lr_ctc_spot", L.lr_ctc_spot, lp.data_ptr(), lp.stride(0), lp.stride(1), _C.ptr(sz),
                 ids.data_ptr(), W, lens.data_ptr(), _C.ptr(thr), self.blank_index, H, hit[0].data_ptr(),
                 hit[1].data_ptr(), hit[2].data_ptr(), per[0].data_ptr(), per[1].data_ptr(),
                 end[0].data_ptr() if trace else None, end[1].data_ptr() if trace else None, ws.data_ptr(), ws.numel(),
                 B, T, C, K)
    if inv is not None:
      hit, per = hit.index_select(2, inv), per.index_select(2, inv)
      if trace:
        end = end.index_select(2, inv)
    out = dict(hit_score=hit[0].view(torch.float32), hit_start=hit[1], hit_end=hit[2], n_hits=per[0], status=per[1])
    if trace:
      out.update(end_score=end[0].view(torch.float32), end_start=end[1])
    return out

  def records(self, out):
    """spot_ids' dict -> per sample a list of dict(keyword, index, start, end, score, confidence), ordered by keyword
    and then by pick order (the ONE device->host read; frames as ints, confidence = exp(score / L))."""
    B, K, H = out["hit_start"].shape
    host = torch.cat([out["hit_score"].view(torch.int32), out["hit_start"], out["hit_end"],
                      out["n_hits"].reshape(B, K, 1)], dim=2).cpu()
    score = host[:, :, :H].contiguous().view(torch.float32).tolist()
    start, end = host[:, :, H:2 * H].tolist(), host[:, :, 2 * H:3 * H].tolist()
    n_hits = host[:, :, 3 * H].tolist()
    recs = []
    for b in range(B):
      found = []
      for k in range(K):
        L = int(self.lengths[k])
        for h in range(n_hits[b][k]):
          sc = score[b][k][h]
          found.append(dict(keyword=self.keywords[k], index=k, start=start[b][k][h], end=end[b][k][h], score=sc,
                            confidence=math.exp(sc / L)))
      recs.append(found)
    return recs

  def spot(self, log_probs, sizes=None):
    """log_probs (B, T, C) on the GPU, sizes (B,) or None -> one list of hits per sample (see records()).  One launch,
    one device->host read."""
    return self.records(self.spot_ids(log_probs, sizes))
