"""CTC segmentation on the device: given a WHOLE video's log-probabilities and its whole caption track, where does each
caption really start and end (BUILD-DEFINED, DESIGN.md §24, after Kuerzinger et al. 2020; the reference has no
segmenter).

CTCAligner times one clip against one caption, pinned to the clip's first and last frame, up to 2048 frames and 256
tokens.  CTCSegmenter runs the same Viterbi recursion over one lattice for the whole stream — up to 65536 frames
against 16384 tokens, the lattice spread over many workgroups and many launches — with the path free to start and end
anywhere (`free_start`, `free_end`), and reads off

  * span (B, 2): the frames [first, one past the last) the path covers;
  * frame_token (B, T): the token a frame belongs to, -1 on blank frames, outside the span and past the stream's length;
  * tok_start / tok_end / tok_logp (B, W): each token's contiguous frames and the sum of its log-probabilities;
  * utt_start / utt_end / utt_frames / utt_logp / utt_worst (B, U): the same per utterance — a token range of the target,
    one caption — with the number of frames its tokens hold and its least likely token;
  * total (B,): the path's log-probability; status (B,): 0, INFEASIBLE, BAD_ID, BAD_LENGTH, BAD_UTTERANCE.

There is no host fall-back: CPU tensors raise LipReadingHipError.
"""
import ctypes
import math

import torch

from . import _C
from . import _host

INFEASIBLE, BAD_ID, BAD_LENGTH = _C.LR_SEG_INFEASIBLE, _C.LR_SEG_BAD_ID, _C.LR_SEG_BAD_LENGTH
BAD_UTTERANCE = _C.LR_SEG_BAD_UTTERANCE
FREE_START, FREE_END = _C.LR_SEG_FREE_START, _C.LR_SEG_FREE_END
MAX_T, MAX_TOKENS = _C.LR_SEG_MAX_T, _C.LR_SEG_MAX_TOKENS
TOO_LONG, NO_CLIPS = 2, 3   # train.segment_videos' own: a video past the limits, a video that keeps no clip


def within_limits(frames, tokens):
  """Whether a stream of `frames` frames and `tokens` target tokens is one lr_ctc_segment takes."""
  return 1 <= frames <= MAX_T and 0 <= tokens <= MAX_TOKENS


class CTCSegmenter(object):
  """Segments streams of ONE class layout (`labels[i]` = class i's string, blank at `blank_index`) on the GPU.  `fps`
  turns frames into seconds; the default is the reference's fixed frame rate (src/data/video.py:55-56)."""

  def __init__(self, labels, blank_index=0, fps=29.97):
    self.labels = list(labels)
    if not 0 <= blank_index < len(self.labels):
      raise ValueError("blank_index %d outside the %d labels" % (blank_index, len(self.labels)))
    self.blank_index, self.fps = int(blank_index), float(fps)
    self._class_of = _host.char_classes(self.labels, self.blank_index)
    self._ws = _host.GrowingWorkspace()

  def seconds(self, frame):
    return frame / self.fps

  def segment_ids(self, log_probs, sizes, targets, target_lens, utt_first=None, utt_count=None, n_utts=None,
                  free_start=True, free_end=True):
    """Nothing read back: log_probs (B, T, C) fp32 on the GPU (any batch / time strides with unit class stride), sizes
    (B,) or None (= T), targets (B, W) integer class ids (blank excluded), target_lens (B,); utt_first, utt_count (B, U)
    and n_utts (B,) the utterances' token ranges, or all None.  Returns a dict of device tensors: span (B, 2),
    frame_token (B, T), tok_start, tok_end (B, W) int32, tok_logp (B, W) fp32, with utterances also utt_start, utt_end,
    utt_frames, utt_worst (B, U) int32 and utt_logp (B, U) fp32; total (B,) fp32; status (B,) int32.  ValueError for a
    shape past the kernels' limits.  The segmenter keeps one workspace per device: call it from one stream at a time."""
    return self._segment_ids(log_probs, sizes, targets, target_lens, utt_first, utt_count, n_utts, free_start, free_end)

  def _segment_ids(self, log_probs, sizes, targets, target_lens, utt_first, utt_count, n_utts, free_start, free_end,
                   phase_ms=None):
    """segment_ids; with phase_ms (tools/bench_segment.py alone: a ctypes float array of 3) through
    lr_ctc_segment_phases, which writes the milliseconds of the forward launches, the walk back and the span launches
    there and waits for the device."""
    _C.require_cuda(log_probs, sizes, targets, target_lens, utt_first, utt_count, n_utts)
    L = _C.lib()
    lp = _host.log_probs_3d(log_probs, len(self.labels), "log_probs")
    B, T, C = lp.shape
    if targets.dim() != 2 or targets.shape[0] != B or target_lens.dim() != 1 or target_lens.shape[0] != B:
      raise ValueError("targets must be (%d, width) and target_lens (%d,), got %s and %s"
                       % (B, B, tuple(targets.shape), tuple(target_lens.shape)))
    with_utts = n_utts is not None
    if with_utts and (utt_first is None or utt_count is None or utt_first.dim() != 2 or utt_first.shape[0] != B
                      or utt_count.shape != utt_first.shape):
      raise ValueError("utt_first and utt_count must both be (%d, utterances) beside n_utts" % B)
    sz = _host.int32_vector(sizes, B, "sizes")
    tl = _host.int32_vector(target_lens, B, "target_lens")
    nu = _host.int32_vector(n_utts, B, "n_utts")
    dev = lp.device

    def table(t):   # (B, width) int32, contiguous, at least one column
      t = t if t.dtype == torch.int32 else t.to(torch.int32)
      if t.shape[1] == 0:
        t = t.new_zeros((B, 1))
      return t.contiguous()

    tg = table(targets)
    W = tg.shape[1]
    nbytes = L.lr_ctc_segment_workspace_bytes(B, T, C, W) if B > 0 and self.blank_index < C else 0
    if nbytes == 0:
      raise ValueError("lr_ctc_segment: unsupported shape B=%d T=%d C=%d target width=%d blank=%d (at most %d frames "
                       "and %d target tokens, at least one sample, two classes and the blank among them)"
                       % (B, T, C, W, self.blank_index, MAX_T, MAX_TOKENS))
    # One workspace per device, grown to the largest shape seen: the back-pointer table, the value rows between the
    # forward launches and the end records.  Calls on ONE stream at a time.
    ws = self._ws.get(dev, nbytes)
    flags = (FREE_START if free_start else 0) | (FREE_END if free_end else 0)
    ints = torch.empty((2, B, W), dtype=torch.int32, device=dev).unbind(0)
    tok_logp = torch.empty((B, W), dtype=torch.float32, device=dev)
    frame_token = torch.empty((B, T), dtype=torch.int32, device=dev)
    span = torch.empty((B, 2), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    out = dict(span=span, frame_token=frame_token, tok_start=ints[0], tok_end=ints[1], tok_logp=tok_logp, total=total,
               status=status)
    U, uf, uc, up = 0, None, None, [None] * 5
    if with_utts:
      uf, uc = table(utt_first), table(utt_count)
      U = uf.shape[1]
      ui = torch.empty((4, B, U), dtype=torch.int32, device=dev).unbind(0)
      utt_logp = torch.empty((B, U), dtype=torch.float32, device=dev)
      out.update(utt_start=ui[0], utt_end=ui[1], utt_frames=ui[2], utt_logp=utt_logp, utt_worst=ui[3])
      up = [ui[0].data_ptr(), ui[1].data_ptr(), ui[2].data_ptr(), utt_logp.data_ptr(), ui[3].data_ptr()]
    timed = () if phase_ms is None else (ctypes.addressof(phase_ms),)
    entry = L.lr_ctc_segment_phases if timed else L.lr_ctc_segment
    _host.launch(dev, "lr_ctc_segment", entry, lp.data_ptr(), lp.stride(0), lp.stride(1), _C.ptr(sz), tg.data_ptr(), W,
                 tl.data_ptr(), _C.ptr(uf), _C.ptr(uc), U, _C.ptr(nu), self.blank_index, flags, frame_token.data_ptr(),
                 ints[0].data_ptr(), ints[1].data_ptr(), tok_logp.data_ptr(), *up, span.data_ptr(), total.data_ptr(),
                 status.data_ptr(), ws.data_ptr(), nbytes, B, T, C, W, *timed)
    return out

  def encode(self, utterance_lists, tail=None):
    """One list of strings per sample -> (targets (B, W), target_lens (B,), utt_first (B, U), utt_count (B, U), n_utts
    (B,)) int32 host tensors: a sample's utterances one after the other in its target.  `tail` is one label, such as
    '<EOS>', appended to every utterance as one token.  KeyError for a character, or a tail, that has no class."""
    tail_id = None
    if tail is not None:
      if tail not in self.labels or self.labels.index(tail) == self.blank_index:
        raise KeyError("tail %r has no class" % (tail,))
      tail_id = self.labels.index(tail)
    rows, ranges = [], []
    for utts in utterance_lists:
      row, rng = [], []
      for s in utts:
        try:
          ids = [self._class_of[ch] for ch in s]
        except KeyError as e:
          raise KeyError("character %r of utterance %r has no class" % (e.args[0], s))
        if tail_id is not None:
          ids.append(tail_id)
        rng.append((len(row), len(ids)))
        row += ids
      rows.append(row)
      ranges.append(rng)
    B = len(rows)
    W = max([len(r) for r in rows] + [1])
    U = max([len(r) for r in ranges] + [1])
    tg = torch.zeros((B, W), dtype=torch.int32)
    uf, uc = torch.zeros((B, U), dtype=torch.int32), torch.zeros((B, U), dtype=torch.int32)
    for b in range(B):
      tg[b, :len(rows[b])] = torch.tensor(rows[b], dtype=torch.int32)
      if ranges[b]:
        r = torch.tensor(ranges[b], dtype=torch.int32)
        uf[b, :len(ranges[b])], uc[b, :len(ranges[b])] = r[:, 0], r[:, 1]
    return (tg, torch.tensor([len(r) for r in rows], dtype=torch.int32), uf, uc,
            torch.tensor([len(r) for r in ranges], dtype=torch.int32))

  def records(self, out, utterance_lists, targets):
    """segment_ids' dict -> one host record per sample (the ONE device->host read): dict(status, total, span,
    utterances=[dict(text, start, end, start_s, end_s, logp, frames, confidence, worst)]) with frames as ints, seconds
    by `fps`, confidence = exp(logp / frames) in float64 (None with 0 frames) and worst the label of the utterance's least
    likely token.  A sample that was not segmented (status != 0) has an empty list."""
    B, U = out["utt_start"].shape
    dev = out["status"].device
    worst = out["utt_worst"].long()
    worst_id = torch.gather(targets.to(device=dev, dtype=torch.int32), 1,
                            worst.clamp(min=0).clamp(max=targets.shape[1] - 1))
    ints = [out[k] for k in ("utt_start", "utt_end", "utt_frames", "utt_worst")] + [worst_id, out["span"],
                                                                                   out["status"].reshape(B, 1)]
    fl = [out["utt_logp"], out["total"].reshape(B, 1)]
    # (floats ride on the same copy as the integers, bit for bit)
    host = torch.cat([t.reshape(B, -1) for t in ints] + [t.reshape(B, -1).view(torch.int32) for t in fl], dim=1).cpu()
    iv = [host[:, k * U:(k + 1) * U].tolist() for k in range(5)]
    at = 5 * U
    span = host[:, at:at + 2].tolist()
    status = host[:, at + 2].tolist()
    fv = host[:, at + 3:].contiguous().view(torch.float32)
    logp, tot = fv[:, :U].tolist(), fv[:, U].tolist()
    recs = []
    for b in range(B):
      rec = dict(status=status[b], total=tot[b], span=tuple(span[b]), utterances=[])
      if status[b] == 0:
        for u, text in enumerate(utterance_lists[b]):
          s, e, fr = iv[0][b][u], iv[1][b][u], iv[2][b][u]
          rec["utterances"].append(dict(
              text=text, start=s, end=e, start_s=self.seconds(s) if s >= 0 else None,
              end_s=self.seconds(e) if e >= 0 else None, logp=logp[b][u], frames=fr,
              confidence=math.exp(logp[b][u] / fr) if fr > 0 else None,
              worst=self.labels[iv[4][b][u]] if iv[3][b][u] >= 0 else None))
      recs.append(rec)
    return recs

  def segment(self, log_probs, sizes, utterance_lists, tail=None, free_start=True, free_end=True):
    """log_probs (B, T, C) on the GPU, sizes (B,) or None, utterance_lists one list of strings per sample -> one record
    per sample (see records()).  One device->host read."""
    _C.require_cuda(log_probs, sizes)
    if len(utterance_lists) != log_probs.shape[0]:
      raise ValueError("%d utterance lists for %d samples" % (len(utterance_lists), log_probs.shape[0]))
    tg, tl, uf, uc, nu = (t.to(log_probs.device) for t in self.encode(utterance_lists, tail))
    out = self.segment_ids(log_probs, sizes, tg, tl, uf, uc, nu, free_start, free_end)
    return self.records(out, utterance_lists, tg)
