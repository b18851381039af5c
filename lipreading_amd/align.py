"""CTC forced alignment on the device: given the clip's log-probabilities AND its known transcript, when is each
character and each word spoken (BUILD-DEFINED; the reference has no aligner).

The decoders answer "what was said" and the greedy decoder's `offsets` time the model's OWN transcript.  CTCAligner
answers the converse for a given caption: one lr_ctc_align launch per batch runs the Viterbi recursion over the CTC
lattice of every sample (the 2L+1 states of the loss, maximum in place of log-sum-exp, a fixed tie-break) and walks
the best path back into

  * frame_token (B, T): the token a frame belongs to, -1 on blank frames and past the clip's length;
  * tok_start / tok_end / tok_logp (B, W): each token's contiguous frames [start, end) and the sum of its
    log-probabilities over them;
  * word_first / word_count / word_start / word_end / word_logp (B, W) and n_words (B,): the same per word — a maximal
    run of tokens whose class is a word character (lm.class_roles: ' ' separates, markers such as '<EOS>' take a span
    of their own but belong to no word);
  * total (B,): the path's log-probability; status (B,): 0, INFEASIBLE (the clip is too short to spell the target),
    BAD_ID, BAD_LENGTH.

There is no host fall-back: CPU tensors raise LipReadingHipError.
"""
import torch

from . import _C
from . import _host
from . import lm

INFEASIBLE, BAD_ID, BAD_LENGTH = _C.LR_ALIGN_INFEASIBLE, _C.LR_ALIGN_BAD_ID, _C.LR_ALIGN_BAD_LENGTH
MAX_T, MAX_LABEL_LEN = _C.LR_ALIGN_MAX_T, 256   # 256: the label limit of lr_ctc_nll (the header names no constant)


class CTCAligner(object):
  """Aligns targets of ONE class layout (`labels[i]` = class i's string, blank at `blank_index`) on the GPU.  `fps`
  turns frames into seconds; the default is the reference's fixed frame rate (src/data/video.py:55-56)."""

  def __init__(self, labels, blank_index=0, fps=29.97):
    self.labels = list(labels)
    if not 0 <= blank_index < len(self.labels):
      raise ValueError("blank_index %d outside the %d labels" % (blank_index, len(self.labels)))
    self.blank_index, self.fps = int(blank_index), float(fps)
    # without a ' ' label nothing separates words: no word outputs
    self.roles = lm.class_roles(self.labels, self.blank_index) if ' ' in self.labels else None
    self._class_of = _host.char_classes(self.labels, self.blank_index)
    self._roles_dev = _host.PerDevice()     # the roles tensor, uploaded once per device
    self._ws = _host.GrowingWorkspace()

  def seconds(self, frame):
    return frame / self.fps

  def _roles(self, dev):
    if self.roles is None:
      return None
    return self._roles_dev.get(dev, lambda d: torch.tensor(self.roles, dtype=torch.int32, device=d))

  def align_ids(self, log_probs, sizes, targets, target_lens):
    """One launch, nothing read back: log_probs (B, T, C) fp32 on the GPU (any batch / time strides with unit class
    stride: the transposed view of a (T, B, C) tensor goes in as it is), sizes (B,) or None (= T), targets (B, W)
    integer class ids in this aligner's class layout (blank excluded), target_lens (B,).  Returns a dict of device
    tensors: frame_token (B, T) int32; tok_start, tok_end (B, W) int32, tok_logp (B, W) fp32; with a ' ' label also
    word_first, word_count, word_start, word_end (B, W) int32, word_logp (B, W) fp32, n_words (B,) int32; total (B,)
    fp32; status (B,) int32.  ValueError for a shape past the kernel's limits.  The aligner keeps one workspace per
    device: call it from one stream at a time."""
    _C.require_cuda(log_probs, sizes, targets, target_lens)
    L = _C.lib()
    lp = _host.log_probs_3d(log_probs, len(self.labels), "log_probs")
    B, T, C = lp.shape
    if targets.dim() != 2 or targets.shape[0] != B or target_lens.dim() != 1 or target_lens.shape[0] != B:
      raise ValueError("targets must be (%d, width) and target_lens (%d,), got %s and %s"
                       % (B, B, tuple(targets.shape), tuple(target_lens.shape)))
    sz = _host.int32_vector(sizes, B, "sizes")
    tl = _host.int32_vector(target_lens, B, "target_lens")
    dev = lp.device
    tg = targets if targets.dtype == torch.int32 else targets.to(torch.int32)
    if tg.shape[1] == 0:
      tg = tg.new_zeros((B, 1))
    tg = tg.contiguous()
    W = tg.shape[1]
    nbytes = L.lr_ctc_align_workspace_bytes(B, T, C, W) if B > 0 and self.blank_index < C else 0
    if nbytes == 0:
      raise ValueError("lr_ctc_align: unsupported shape B=%d T=%d C=%d target width=%d blank=%d (at most %d frames and "
                       "%d target tokens, at least one sample, two classes and the blank among them)"
                       % (B, T, C, W, self.blank_index, MAX_T, MAX_LABEL_LEN))
    # One workspace per device, grown to the largest shape seen (the back-pointer table when it does not fit in LDS).
    # Calls on ONE stream at a time: two streams aligning concurrently on a device would share the table.
    ws = self._ws.get(dev, nbytes)
    roles = self._roles(dev)
    # (each output's view is made once: its pointer goes to the kernel and the view itself into the dict)
    ints = torch.empty((6 if roles is not None else 2, B, W), dtype=torch.int32, device=dev).unbind(0)
    flts = torch.empty((2, B, W), dtype=torch.float32, device=dev).unbind(0)
    frame_token = torch.empty((B, T), dtype=torch.int32, device=dev)
    per = torch.empty((2, B), dtype=torch.int32, device=dev).unbind(0)   # status, n_words
    total = torch.empty((B,), dtype=torch.float32, device=dev)
    wp = [t.data_ptr() for t in ints[2:] + (flts[1], per[1])] if roles is not None else [None] * 6
    _host.launch(dev, "lr_ctc_align", L.lr_ctc_align, lp.data_ptr(), lp.stride(0), lp.stride(1), _C.ptr(sz),
                 tg.data_ptr(), W, tl.data_ptr(), _C.ptr(roles), self.blank_index, frame_token.data_ptr(),
                 ints[0].data_ptr(), ints[1].data_ptr(), flts[0].data_ptr(), *wp, total.data_ptr(), per[0].data_ptr(),
                 ws.data_ptr(), nbytes, B, T, C, W)
    out = dict(frame_token=frame_token, tok_start=ints[0], tok_end=ints[1], tok_logp=flts[0], total=total,
               status=per[0])
    if roles is not None:
      out.update(word_first=ints[2], word_count=ints[3], word_start=ints[4], word_end=ints[5], word_logp=flts[1],
                 n_words=per[1])
    return out

  def encode(self, transcripts):
    """Strings -> (targets (B, W) int32, target_lens (B,) int32) host tensors; KeyError for a character that has no
    class (the blank's label is no character)."""
    rows = []
    for s in transcripts:
      try:
        rows.append([self._class_of[ch] for ch in s])
      except KeyError as e:
        raise KeyError("character %r of transcript %r has no class" % (e.args[0], s))
    W = max([len(r) for r in rows] + [1])
    tg = torch.zeros((len(rows), W), dtype=torch.int32)
    for b, r in enumerate(rows):
      tg[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return tg, torch.tensor([len(r) for r in rows], dtype=torch.int32)

  def records(self, out, targets, target_lens):
    """align_ids' dict -> one host record per sample (the ONE device->host read):
    dict(status, total, chars=[(label, start, end, logp)], words=[(word, start, end, logp)]) with frames as ints;
    a sample that was not aligned (status != 0) has empty lists."""
    B, W = out["tok_start"].shape
    if targets.shape[1] < W:   # (align_ids widens a (B, 0) target to one column)
      targets = torch.nn.functional.pad(targets, (0, W - targets.shape[1]))
    words = "n_words" in out
    ints = [out["tok_start"], out["tok_end"], targets.to(device=out["status"].device, dtype=torch.int32)[:, :W]]
    if words:
      ints += [out[k] for k in ("word_first", "word_count", "word_start", "word_end")]
    cols = [out["status"].reshape(B, 1), target_lens.to(device=out["status"].device, dtype=torch.int32).reshape(B, 1)]
    if words:
      cols.append(out["n_words"].reshape(B, 1))
    fl = [out["tok_logp"]] + ([out["word_logp"]] if words else []) + [out["total"].reshape(B, 1)]
    # (floats ride on the same copy as the integers, bit for bit)
    host = torch.cat([t.reshape(B, -1) for t in ints + cols] + [t.reshape(B, -1).view(torch.int32) for t in fl],
                     dim=1).cpu()
    ni = len(ints)
    iv = [host[:, k * W:(k + 1) * W].tolist() for k in range(ni)]
    at = ni * W
    cv = host[:, at:at + len(cols)].tolist()
    at += len(cols)
    fv = host[:, at:].contiguous().view(torch.float32)
    tok_lp = fv[:, :W].tolist()
    word_lp = fv[:, W:2 * W].tolist() if words else None
    tot = fv[:, -1].tolist()
    recs = []
    for b in range(B):
      status, L = cv[b][0], cv[b][1]
      rec = dict(status=status, total=tot[b], chars=[], words=[])
      if status == 0:
        ids = iv[2][b]
        rec["chars"] = [(self.labels[ids[i]], iv[0][b][i], iv[1][b][i], tok_lp[b][i]) for i in range(L)]
        if words:
          for w in range(cv[b][2]):
            f, c = iv[3][b][w], iv[4][b][w]
            rec["words"].append((''.join(self.labels[ids[i]] for i in range(f, f + c)), iv[5][b][w], iv[6][b][w],
                                 word_lp[b][w]))
      recs.append(rec)
    return recs

  def align(self, log_probs, sizes, transcripts):
    """log_probs (B, T, C) on the GPU, sizes (B,) or None, transcripts a list of B strings -> one record per sample
    (see records()).  One launch, one device->host read."""
    _C.require_cuda(log_probs, sizes)
    if len(transcripts) != log_probs.shape[0]:
      raise ValueError("%d transcripts for %d samples" % (len(transcripts), log_probs.shape[0]))
    tg, tl = self.encode(transcripts)
    dev = log_probs.device
    tg, tl = tg.to(dev), tl.to(dev)
    return self.records(self.align_ids(log_probs, sizes, tg, tl), tg, tl)
