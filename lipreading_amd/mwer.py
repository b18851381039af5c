"""N-best minimum error rate training of the CTC head on the MI355X (BUILD-DEFINED: the reference trains that head on
the frame-synchronous likelihood alone, lipreading_amd/ctc.py).

The driver reports, and picks checkpoints by, the edit-distance error of the decoded transcript.  This module trains on
that quantity: the expected risk over an N-best list,

  R_b = sum_n p_n r_n,   p_n = softmax_n(ll_n),   ll_n = the full-sum CTC log-likelihood of hypothesis n,

with the lattices, the softmax and the gradient in lr_nbest.hip (the specification: include/lipreading_hip.h, A6h).
`nbest_risk_loss` is the front door of those kernels; `MWERLoss` chains search -> score -> loss on the device:
BeamCTCDecoder.decode_ids for the N-best list, EditScorer.score for the risks.  Nothing here reads the device.
"""
import torch

from . import _C, _host

_REDUCTIONS = {"sum": 0, "mean": 1}
MAX_SLOTS = _C.LR_NBEST_MAX_SLOTS
MAX_CLASSES = _C.LR_NBEST_MAX_CLASSES
MAX_HYP_LEN = _C.LR_NBEST_MAX_HYP_LEN


def _hyp_args(hyp_ids, hyp_lens, risk):
  """(ids, address of slot (b, n)'s row as two strides, lens, risk) as lr_ctc_nbest_risk takes them."""
  return (hyp_ids.data_ptr(), hyp_ids.stride(0), hyp_ids.stride(1), hyp_lens.data_ptr(), hyp_lens.stride(0),
          risk.data_ptr())


class _NbestRiskFunction(torch.autograd.Function):
  """forward: the N lattices per utterance -> softmax -> expected risk.  backward: the risk-weighted occupancies."""

  @staticmethod
  def forward(ctx, log_probs, sizes, hyp_ids, hyp_lens, risk, blank, reduction):
    L = _C.lib()
    ctx.set_materialize_grads(False)   # only the loss gets a gradient: no zero tensors for the other outputs
    B, T, C = log_probs.shape
    N, max_len = hyp_ids.shape[1], hyp_ids.shape[2]
    dev = log_probs.device
    ws_bytes = L.lr_ctc_nbest_workspace_bytes(B, T, C, N, max_len)
    if ws_bytes == 0:
      raise _C.LipReadingHipError("lr_ctc_nbest_risk: unsupported shape B=%d T=%d C=%d N=%d max_hyp_len=%d"
                                  % (B, T, C, N, max_len))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    hyp_ll = torch.empty((B, N), dtype=torch.float32, device=dev)
    post = torch.empty((B, N), dtype=torch.float32, device=dev)
    hyp_status = torch.empty((B, N), dtype=torch.int32, device=dev)
    utt_risk = torch.empty(B, dtype=torch.float32, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    gw = torch.empty(B, dtype=torch.float32, device=dev)
    _host.launch(dev, "lr_ctc_nbest_risk", L.lr_ctc_nbest_risk, log_probs.data_ptr(), log_probs.stride(0),
                 log_probs.stride(1), _C.ptr(sizes), *_hyp_args(hyp_ids, hyp_lens, risk), blank, reduction,
                 hyp_ll.data_ptr(), post.data_ptr(), hyp_status.data_ptr(), utt_risk.data_ptr(), out.data_ptr(),
                 status.data_ptr(), gw.data_ptr(), ws.data_ptr(), ws_bytes, B, T, C, N, max_len)
    ctx.save_for_backward(log_probs, sizes, hyp_ids, hyp_lens, risk, hyp_ll, post, hyp_status, utt_risk, gw, ws)
    ctx.consts = (blank, reduction)
    ctx.mark_non_differentiable(status, hyp_ll, post, hyp_status, utt_risk)
    return out.reshape(()), status, hyp_ll, post, hyp_status, utt_risk

  @staticmethod
  def backward(ctx, grad_out, *_):
    if grad_out is None:
      return (None,) * 7
    log_probs, sizes, hyp_ids, hyp_lens, risk, hyp_ll, post, hyp_status, utt_risk, gw, ws = ctx.saved_tensors
    blank, reduction = ctx.consts
    L = _C.lib()
    B, T, C = log_probs.shape
    N, max_len = hyp_ids.shape[1], hyp_ids.shape[2]
    dev = log_probs.device
    # the incoming gradient multiplies every row INSIDE the kernel (a device scalar), as in _CTCLossFunction
    go = grad_out.reshape(1)
    if go.dtype != torch.float32:
      go = go.float()
    # grad is addressed like log_probs: a contiguous copy where the input was a transposed view (the tables in the
    # workspace do not depend on the layout)
    lp = log_probs if log_probs.is_contiguous() else log_probs.contiguous()
    grad = torch.empty((B, T, C), dtype=torch.float32, device=dev)   # every element is written
    _host.launch(dev, "lr_ctc_nbest_risk_grad", L.lr_ctc_nbest_risk_grad, lp.data_ptr(), lp.stride(0), lp.stride(1),
                 _C.ptr(sizes), *_hyp_args(hyp_ids, hyp_lens, risk), blank, reduction, hyp_ll.data_ptr(),
                 post.data_ptr(), hyp_status.data_ptr(), utt_risk.data_ptr(), gw.data_ptr(), go.data_ptr(),
                 grad.data_ptr(), ws.data_ptr(), ws.numel(), B, T, C, N, max_len)
    return grad, None, None, None, None, None, None


def nbest_risk_loss(log_probs, sizes, hyp_ids, hyp_lens, risk, blank_index=0, reduction='mean'):
  """The expected risk of N hypothesis slots per utterance under the CTC head, on the device.

  log_probs (B, T, C) fp32 log-probabilities (any batch / time strides: the transposed view of a (T, B, C) tensor goes
  in as it is); sizes (B,) frames per utterance or None (= T); hyp_ids (B, N, Lmax) class ids (any strides over B and
  N: `ids[:, :N]` of a beam search's (B, W, T) goes in as it is), hyp_lens (B, N) with -1 for an empty slot, risk
  (B, N), finite and >= 0.  N <= 16, C <= 256, Lmax <= 256.

  Returns (loss, status, info): `loss` a differentiable 0-dim tensor ('mean' over the utterances with a usable slot, or
  'sum'); `status` (1,) int32, 1 when no utterance has a usable slot (the loss is then 0 with a zero gradient: skip the
  batch, as ctc_loss_with_status); `info` a dict of device tensors: hyp_ll (B, N) (-inf for an unused slot), posterior
  (B, N), hyp_status (B, N) int32 (0 used, 1 empty, 2 rejected, 3 infeasible), utt_risk (B,).  No host synchronisation."""
  _C.require_cuda(log_probs, sizes, hyp_ids, hyp_lens, risk)
  if reduction not in _REDUCTIONS:
    raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
  if log_probs.dim() != 3:
    raise ValueError("log_probs must be (batch, frames, classes), got %s" % (tuple(log_probs.shape),))
  B, T, C = log_probs.shape
  if hyp_ids.dim() != 3 or hyp_ids.shape[0] != B:
    raise ValueError("hyp_ids must be (%d, N, max_hyp_len), got %s" % (B, tuple(hyp_ids.shape)))
  N = hyp_ids.shape[1]
  if not 1 <= N <= MAX_SLOTS:
    raise ValueError("%d hypothesis slots per utterance: at least 1, at most %d" % (N, MAX_SLOTS))
  if tuple(hyp_lens.shape) != (B, N) or tuple(risk.shape) != (B, N):
    raise ValueError("hyp_lens and risk must be (%d, %d), got %s and %s"
                     % (B, N, tuple(hyp_lens.shape), tuple(risk.shape)))
  if C > MAX_CLASSES or hyp_ids.shape[2] > MAX_HYP_LEN:
    raise ValueError("%d classes, hypotheses up to %d ids: at most %d and %d"
                     % (C, hyp_ids.shape[2], MAX_CLASSES, MAX_HYP_LEN))
  if not 0 <= blank_index < C:
    raise ValueError("blank_index %d outside the %d classes" % (blank_index, C))
  lp = _host.log_probs_3d(log_probs, C, "log_probs")
  sz = _host.int32_vector(sizes, B, "sizes", device=lp.device)
  ids = hyp_ids if hyp_ids.dtype == torch.int32 else hyp_ids.to(torch.int32)
  if ids.shape[2] == 0:
    ids = ids.new_zeros((B, N, 1))
  if ids.stride(2) != 1 or ids.stride(0) < 0 or ids.stride(1) < 0:
    ids = ids.contiguous()
  lens = hyp_lens if hyp_lens.dtype == torch.int32 else hyp_lens.to(torch.int32)
  if lens.stride(1) != 1 or lens.stride(0) < 0:
    lens = lens.contiguous()
  r = risk if risk.dtype == torch.float32 else risk.float()
  r = r.detach().contiguous()
  loss, status, hyp_ll, post, hyp_status, utt_risk = _NbestRiskFunction.apply(
      lp, sz, ids, lens, r, int(blank_index), _REDUCTIONS[reduction])
  return loss, status, dict(hyp_ll=hyp_ll, posterior=post, hyp_status=hyp_status, utt_risk=utt_risk)


class MWERLoss(object):
  """Minimum word / character error rate over the beam search's own N-best list.

  `decoder`: a BeamCTCDecoder with log_probs_input=True and beam_width >= nbest; its language model and hotwords shape
  the list as they do at evaluation.  `unit`: 'char' or 'word' edit distance as the risk.  with_reference=True adds the
  reference transcript as one more slot, with risk 0, for the utterances none of whose beams has distance 0 (decided on
  the device; elsewhere the extra slot is empty).

  __call__(log_probs, sizes, ref_ids, ref_lens) -> (loss, status, info) as nbest_risk_loss, `info` also holding the
  slots it built: hyp_ids, hyp_lens, risk.  ref_ids (B, Lr) are class ids in the decoder's layout.  The search and the
  scoring run under no_grad on the detached log-probabilities; only the loss is differentiated."""

  def __init__(self, decoder, nbest=4, unit='char', with_reference=False):
    if not hasattr(decoder, "decode_ids") or not hasattr(decoder, "beam_width"):
      raise TypeError("MWERLoss needs a BeamCTCDecoder")
    if not getattr(decoder, "log_probs_input", False):
      raise ValueError("MWERLoss needs a decoder with log_probs_input=True: it searches the head's log-probabilities")
    if unit not in ('char', 'word'):
      raise ValueError("unit must be 'char' or 'word', got %r" % (unit,))
    nbest, with_reference = int(nbest), bool(with_reference)
    if not 1 <= nbest or nbest + with_reference > MAX_SLOTS:
      raise ValueError("nbest=%d%s: at least 1, at most %d slots" % (nbest, " plus the reference" * with_reference,
                                                                    MAX_SLOTS))
    if decoder.beam_width < nbest:
      raise ValueError("nbest=%d of a search that keeps beam_width=%d hypotheses" % (nbest, decoder.beam_width))
    self.decoder, self.nbest, self.unit, self.with_reference = decoder, nbest, unit, with_reference
    self.scorer = decoder.scorer()   # its own: nobody's evaluation totals are touched

  def slots(self, log_probs, sizes, ref_ids, ref_lens):
    """(hyp_ids (B, N', L) int32, hyp_lens (B, N') int32, risk (B, N') fp32) on the device, N' = nbest (+ 1)."""
    N = self.nbest
    with torch.no_grad():
      ids, _, lens, scores = self.decoder.decode_ids(log_probs.detach(), sizes)
      B, _, T = ids.shape
      dev = ids.device
      ref = ref_ids if ref_ids.dtype == torch.int32 else ref_ids.to(torch.int32)
      rl = _host.int32_vector(ref_lens, B, "ref_lens", device=dev)
      if ref.dim() != 2 or ref.shape[0] != B:
        raise ValueError("ref_ids must be (%d, width), got %s" % (B, tuple(ref.shape)))
      Lr = ref.shape[1]
      hyp = ids[:, :N].contiguous()
      # an empty beam slot is lens == 0 with scores == +inf; a genuine empty transcript keeps len 0
      found = ~((lens[:, :N] == 0) & (scores[:, :N] == float("inf")))
      out = self.scorer.score(hyp.view(B * N, T), lens[:, :N].reshape(B * N),
                              ref.unsqueeze(1).expand(B, N, Lr).reshape(B * N, Lr),
                              rl.unsqueeze(1).expand(B, N).reshape(B * N), unit=self.unit)
      dist = out["distance"].view(B, N)
      hl = torch.where(found, lens[:, :N], torch.full_like(dist, -1))
      risk = dist.to(torch.float32)
      if self.with_reference:
        exact = ((dist == 0) & found).any(dim=1)
        W = max(T, Lr)
        slots = torch.zeros((B, N + 1, W), dtype=torch.int32, device=dev)
        slots[:, :N, :T] = hyp
        slots[:, N, :Lr] = ref
        hyp = slots
        hl = torch.cat((hl, torch.where(exact, torch.full_like(rl, -1), rl).unsqueeze(1)), dim=1)
        risk = torch.cat((risk, risk.new_zeros((B, 1))), dim=1)
    return hyp, hl, risk

  def __call__(self, log_probs, sizes, ref_ids, ref_lens):
    _C.require_cuda(log_probs, sizes, ref_ids, ref_lens)
    hyp, hl, risk = self.slots(log_probs, sizes, ref_ids, ref_lens)
    loss, status, info = nbest_risk_loss(log_probs, sizes, hyp, hl, risk, blank_index=self.decoder.blank_index,
                                         reduction='mean')
    info.update(hyp_ids=hyp, hyp_lens=hl, risk=risk)
    return loss, status, info
