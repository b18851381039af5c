"""A transducer head on the MI355X (BUILD-DEFINED: the reference has none).

Frame-synchronous like the CTC head and label-conditioned like the attention decoder (Graves 2012): per frame t and
label position u a joint network scores the next class given the encoder's `hidden` at t and the last `context` labels,

  e = enc_proj(hidden)                                                    (B, T, J)
  p_u = pred_proj.bias + sum_{k < context} pred_proj.weight[:, kE:(k+1)E] . embed[y_{u-k}]     (y_j = 0 for j <= 0)
  log p(. | t, u) = masked log_softmax(joint(tanh(e_t + p_u)))

over the CTC head's class layout (class 0 the blank, class c character c - 1, PAD + 1 and BOS + 1 masked).  The
prediction network is stateless, so each context slot is a (V1, J) table and p_u a sum of table rows; the loss with its
gradients and the greedy decoder are lr_transducer.hip (the specification: include/lipreading_hip.h, A6i).  Nothing here
reads the device but decode_strings.
"""
import torch
from torch import nn

from . import _C, _host
from .data import BOS, EOS, PAD

_REDUCTIONS = {"sum": 0, "mean": 1}
MAX_T = _C.LR_RNNT_MAX_T
MAX_U = _C.LR_RNNT_MAX_U
MAX_CLASSES = _C.LR_RNNT_MAX_CLASSES
MAX_JOINT = _C.LR_RNNT_MAX_JOINT
BEAM_MAX_WIDTH = _C.LR_RNNT_BEAM_MAX_WIDTH
BEAM_MAX_SYMBOLS = _C.LR_RNNT_BEAM_MAX_SYMBOLS
BEAM_BAD_STATE = _C.LR_RNNT_BEAM_BAD_STATE
BAD_ID = _C.LR_RNNT_BAD_ID
BAD_LENGTH = _C.LR_RNNT_BAD_LENGTH


def _direct(weights):
  from .encoder import _direct_grads
  return _direct_grads(weights)


class _RNNTLossFunction(torch.autograd.Function):
  """forward: joint stage + alpha + batch reduction.  backward: beta + the tiles' gradients + the combine."""

  @staticmethod
  def forward(ctx, e, p, weight, bias, mask, labels, frame_lens, label_lens, reduction):
    L = _C.lib()
    ctx.set_materialize_grads(False)
    B, T, J = e.shape
    U, V1 = p.shape[1] - 1, weight.shape[0]
    dev = e.device
    ws_bytes = L.lr_rnnt_workspace_bytes(B, T, U, V1, J)
    if ws_bytes == 0:
      raise ValueError("lr_rnnt_loss_forward: unsupported shape B=%d T=%d U=%d V1=%d J=%d (at most T %d, U %d, V1 %d, J %d)"
                       % (B, T, U, V1, J, MAX_T, MAX_U, MAX_CLASSES, MAX_JOINT))
    p, weight, bias, mask = p.contiguous(), weight.contiguous(), bias.contiguous(), mask.contiguous()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    sstat = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _host.launch(dev, "lr_rnnt_loss_forward", L.lr_rnnt_loss_forward, e.data_ptr(), e.stride(0), e.stride(1),
                 p.data_ptr(), weight.data_ptr(), bias.data_ptr(), mask.data_ptr(), labels.data_ptr(),
                 labels.stride(0), frame_lens.data_ptr(), label_lens.data_ptr(), reduction, nll.data_ptr(),
                 sstat.data_ptr(), out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, B, T, U, V1, J)
    ctx.save_for_backward(e, p, weight, bias, mask, labels, frame_lens, label_lens, nll, sstat, ws)
    ctx.weights = (weight, bias)   # (the leaves themselves when they were contiguous: their .grad may take the sums)
    ctx.mark_non_differentiable(status, nll, sstat)
    return out.reshape(()), status, nll, sstat

  @staticmethod
  def backward(ctx, grad_out, *_):
    if grad_out is None:
      return (None,) * 9
    e, p, weight, bias, mask, labels, frame_lens, label_lens, nll, sstat, ws = ctx.saved_tensors
    L = _C.lib()
    B, T, J = e.shape
    U, V1 = p.shape[1] - 1, weight.shape[0]
    dev = e.device
    go = grad_out.reshape(1)
    if go.dtype != torch.float32:
      go = go.float()
    d_e = torch.empty((B, T, J), dtype=torch.float32, device=dev)
    d_p = torch.empty((B, U + 1, J), dtype=torch.float32, device=dev)
    direct = _direct(ctx.weights)
    d_w = ctx.weights[0].grad if direct else torch.empty((V1, J), dtype=torch.float32, device=dev)
    d_b = ctx.weights[1].grad if direct else torch.empty((V1,), dtype=torch.float32, device=dev)
    _host.launch(dev, "lr_rnnt_loss_backward", L.lr_rnnt_loss_backward, e.data_ptr(), e.stride(0), e.stride(1),
                 p.data_ptr(), weight.data_ptr(), bias.data_ptr(), mask.data_ptr(), labels.data_ptr(),
                 labels.stride(0), frame_lens.data_ptr(), label_lens.data_ptr(), nll.data_ptr(), sstat.data_ptr(),
                 go.data_ptr(), d_e.data_ptr(), d_p.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), 1 if direct else 0,
                 ws.data_ptr(), ws.numel(), B, T, U, V1, J)
    if direct:
      return d_e, d_p, None, None, None, None, None, None, None
    return d_e, d_p, d_w, d_b, None, None, None, None, None


def rnnt_loss(e, p, joint_weight, joint_bias, class_mask, labels_p1, frame_lens, label_lens, reduction='mean'):
  """The transducer loss of the joint network over the lattice, on the device (lr_rnnt_loss_forward / _backward).

  e (B, T, J) fp32 with unit J stride (any batch / time strides: the transposed view of a (T, B, J) tensor goes in as it
  is), p (B, U + 1, J), joint_weight (V1, J), joint_bias (V1,), class_mask (V1,) with 0 for a masked class, labels_p1
  (B, U) class ids, frame_lens / label_lens (B,).  Returns (loss, status, info): `loss` a 0-dim tensor differentiable in
  e, p, joint_weight and joint_bias; `status` (1,) int32, 1 when no sample was usable (the loss is then 0 with zero
  gradients: skip the batch); `info` = dict(nll (B,), sample_status (B,) int32: 0, BAD_ID or BAD_LENGTH).  A shape the
  kernels reject raises ValueError.  No host synchronisation."""
  _C.require_cuda(e, p, joint_weight, joint_bias, class_mask, labels_p1, frame_lens, label_lens)
  if reduction not in _REDUCTIONS:
    raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
  if e.dim() != 3 or p.dim() != 3 or p.shape[0] != e.shape[0] or p.shape[2] != e.shape[2] or p.shape[1] < 1:
    raise ValueError("e must be (B, T, J) and p (B, U + 1, J), got %s and %s" % (tuple(e.shape), tuple(p.shape)))
  B, T, J = e.shape
  U = p.shape[1] - 1
  if joint_weight.dim() != 2 or joint_weight.shape[1] != J:
    raise ValueError("joint_weight must be (V1, %d), got %s" % (J, tuple(joint_weight.shape)))
  V1 = joint_weight.shape[0]
  if tuple(joint_bias.shape) != (V1,) or tuple(class_mask.shape) != (V1,):
    raise ValueError("joint_bias and class_mask must be (%d,)" % V1)
  if labels_p1.dim() != 2 or labels_p1.shape[0] != B or labels_p1.shape[1] != U:
    raise ValueError("labels_p1 must be (%d, %d), got %s" % (B, U, tuple(labels_p1.shape)))
  if e.dtype != torch.float32:
    e = e.float()
  if e.stride(2) != 1 or e.stride(0) < 0 or e.stride(1) < 0:
    e = e.contiguous()
  if p.dtype != torch.float32:
    p = p.float()
  lab = labels_p1 if labels_p1.dtype == torch.int32 else labels_p1.to(torch.int32)
  if U == 0:
    lab = lab.new_zeros((B, 1))
  elif lab.stride(1) != 1 or lab.stride(0) < 0:
    lab = lab.contiguous()
  fl = _host.int32_vector(frame_lens, B, "frame_lens", device=e.device)
  ll = _host.int32_vector(label_lens, B, "label_lens", device=e.device)
  mask = class_mask if class_mask.dtype == torch.float32 else class_mask.float()
  loss, status, nll, sstat = _RNNTLossFunction.apply(e, p, joint_weight, joint_bias, mask, lab, fl, ll,
                                                     _REDUCTIONS[reduction])
  return loss, status, dict(nll=nll, sample_status=sstat)


def rnnt_greedy(e, sizes, tables, joint_weight, joint_bias, class_mask, state=None, max_symbols=5, max_out=None):
  """Greedy transducer decoding in one launch (lr_rnnt_greedy_decode).  e (B, T, J) as rnnt_loss takes it, sizes (B,)
  or None (= T), tables (context, V1, J) with the prediction bias folded into table 0.  `state`: None for a one-shot
  decode, or the dict an earlier call returned (its tensors are continued IN PLACE: ids, frames, logp, lens, forced, the
  context and the frame base, which moves on by `sizes`), so that a clip fed in pieces gives the one-shot call's bits.
  max_out: the width of ids / frames / logp (default T * max_symbols; with a state, the state's).  Returns
  dict(ids, lens, frames, logp, forced, state) of device tensors; symbols past max_out are counted in lens, not written."""
  _C.require_cuda(e, sizes, tables, joint_weight, joint_bias, class_mask)
  if e.dim() != 3 or tables.dim() != 3 or tables.shape[0] not in (1, 2) or tables.shape[2] != e.shape[2]:
    raise ValueError("e must be (B, T, J) and tables (1 or 2, V1, J), got %s and %s"
                     % (tuple(e.shape), tuple(tables.shape)))
  B, T, J = e.shape
  context, V1 = tables.shape[0], tables.shape[1]
  if tuple(joint_weight.shape) != (V1, J) or tuple(joint_bias.shape) != (V1,) or tuple(class_mask.shape) != (V1,):
    raise ValueError("joint_weight must be (%d, %d), joint_bias and class_mask (%d,)" % (V1, J, V1))
  max_symbols = int(max_symbols)
  if max_symbols < 1:
    raise ValueError("max_symbols must be at least 1, got %d" % max_symbols)
  if not (1 <= T <= MAX_T and V1 <= MAX_CLASSES and J <= MAX_JOINT):
    raise ValueError("lr_rnnt_greedy_decode: unsupported shape T=%d V1=%d J=%d (at most %d, %d, %d)"
                     % (T, V1, J, MAX_T, MAX_CLASSES, MAX_JOINT))
  dev = e.device
  if e.dtype != torch.float32:
    e = e.float()
  if e.stride(2) != 1 or e.stride(0) < 0 or e.stride(1) < 0:
    e = e.contiguous()
  sz = _host.int32_vector(sizes, B, "sizes", device=dev)
  if state is None:
    width = int(max_out) if max_out is not None else T * max_symbols
    if width < 1:
      raise ValueError("max_out must be at least 1, got %d" % width)
    out = dict(ids=torch.zeros((B, width), dtype=torch.int32, device=dev),
               frames=torch.zeros((B, width), dtype=torch.int32, device=dev),
               logp=torch.zeros((B, width), dtype=torch.float32, device=dev),
               lens=torch.zeros(B, dtype=torch.int32, device=dev),
               forced=torch.zeros(B, dtype=torch.int32, device=dev),
               state=dict(context=torch.zeros((B, context), dtype=torch.int32, device=dev),
                          frame_base=torch.zeros(B, dtype=torch.int32, device=dev)))
    st = out["state"]
    st.update({k: out[k] for k in ("ids", "frames", "logp", "lens", "forced")})
  else:
    st = state
    out = dict(ids=st["ids"], frames=st["frames"], logp=st["logp"], lens=st["lens"], forced=st["forced"], state=st)
    if tuple(st["context"].shape) != (B, context):
      raise ValueError("the state is of %s streams and context, the call of %s"
                       % (tuple(st["context"].shape), (B, context)))
  _host.launch(dev, "lr_rnnt_greedy_decode", _C.lib().lr_rnnt_greedy_decode, e.data_ptr(), e.stride(0), e.stride(1),
               _C.ptr(sz), tables.contiguous().data_ptr(), joint_weight.contiguous().data_ptr(),
               joint_bias.contiguous().data_ptr(), class_mask.contiguous().data_ptr(), st["context"].data_ptr(),
               st["frame_base"].data_ptr(), out["ids"].data_ptr(), out["frames"].data_ptr(), out["logp"].data_ptr(),
               out["lens"].data_ptr(), out["forced"].data_ptr(), B, T, V1, J, context, max_symbols,
               out["ids"].shape[1])
  st["frame_base"] += (sz.clamp(0, T) if sz is not None else T)
  return out


def rnnt_beam(e, sizes, tables, joint_weight, joint_bias, class_mask, beam_width=8, max_symbols=3, nbest=None,
              state=None, max_out=None):
  """Time-synchronous transducer beam search in one search launch (lr_rnnt_beam_decode; the specification:
  include/lipreading_hip.h, A6j).  e, sizes, tables, joint_weight, joint_bias and class_mask as rnnt_greedy takes them.
  beam_width in [1, 32], max_symbols in [1, 8] label rounds per frame, nbest (default beam_width) hypotheses reported,
  max_out in [1, 256] the width of ids / frames (default min(T * max_symbols, 256); with a state, the state's).
  `state`: None for a one-shot search, or the dict an earlier call returned, continued IN PLACE (the beams, `truncated`
  and the frame base, which moves on by `sizes`): a clip fed in pieces at any frame boundaries gives the one-shot
  call's bits.  A state made for another batch, width, max_out or context raises ValueError.  Returns dict(ids, frames
  (B, nbest, max_out) int32, lens (B, nbest), scores (B, nbest) fp32 descending with -inf in empty slots, count (B,),
  truncated (B,), state) of device tensors; state["status"] is the device's word on the buffer (0, or BEAM_BAD_STATE).
  No host synchronisation."""
  _C.require_cuda(e, sizes, tables, joint_weight, joint_bias, class_mask)
  if e.dim() != 3 or tables.dim() != 3 or tables.shape[0] not in (1, 2) or tables.shape[2] != e.shape[2]:
    raise ValueError("e must be (B, T, J) and tables (1 or 2, V1, J), got %s and %s"
                     % (tuple(e.shape), tuple(tables.shape)))
  B, T, J = e.shape
  context, V1 = tables.shape[0], tables.shape[1]
  if tuple(joint_weight.shape) != (V1, J) or tuple(joint_bias.shape) != (V1,) or tuple(class_mask.shape) != (V1,):
    raise ValueError("joint_weight must be (%d, %d), joint_bias and class_mask (%d,)" % (V1, J, V1))
  beam_width, max_symbols = int(beam_width), int(max_symbols)
  if not 1 <= beam_width <= BEAM_MAX_WIDTH:
    raise ValueError("beam_width must be in [1, %d], got %d" % (BEAM_MAX_WIDTH, beam_width))
  if not 1 <= max_symbols <= BEAM_MAX_SYMBOLS:
    raise ValueError("max_symbols must be in [1, %d], got %d" % (BEAM_MAX_SYMBOLS, max_symbols))
  nbest = beam_width if nbest is None else int(nbest)
  if not 1 <= nbest <= beam_width:
    raise ValueError("nbest must be in [1, beam_width = %d], got %d" % (beam_width, nbest))
  if not (1 <= B <= 65535 and 1 <= T <= MAX_T and 2 <= V1 <= MAX_CLASSES and 1 <= J <= MAX_JOINT):
    raise ValueError("lr_rnnt_beam_decode: unsupported shape B=%d T=%d V1=%d J=%d (at most 65535, %d, %d, %d)"
                     % (B, T, V1, J, MAX_T, MAX_CLASSES, MAX_JOINT))
  if state is None:
    width = int(max_out) if max_out is not None else min(T * max_symbols, MAX_U)
  else:
    width = state["max_out"]
    if max_out is not None and int(max_out) != width:
      raise ValueError("the state holds hypotheses of at most %d labels, the call asks for %d" % (width, int(max_out)))
  if not 1 <= width <= MAX_U:
    raise ValueError("max_out must be in [1, %d], got %d" % (MAX_U, width))
  L = _C.lib()
  dev = e.device
  if state is None:
    nbytes = L.lr_rnnt_beam_state_bytes(B, beam_width, width)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = dict(buffer=buf, status=buf[:32].view(torch.int32)[5], B=B, beam_width=beam_width, max_out=width,
              context=context, truncated=torch.zeros(B, dtype=torch.int32, device=dev),
              frame_base=torch.zeros(B, dtype=torch.int32, device=dev))
    fresh = 1
  else:
    st = state
    if (st["B"], st["beam_width"], st["max_out"], st["context"]) != (B, beam_width, width, context):
      raise ValueError("the state is of (B, beam_width, max_out, context) = %s, the call of %s"
                       % ((st["B"], st["beam_width"], st["max_out"], st["context"]), (B, beam_width, width, context)))
    _C.require_cuda(st["buffer"])
    if st["buffer"].numel() != L.lr_rnnt_beam_state_bytes(B, beam_width, width):
      raise ValueError("the state's buffer holds %d bytes, a state of this geometry %d"
                       % (st["buffer"].numel(), L.lr_rnnt_beam_state_bytes(B, beam_width, width)))
    fresh = 0
  if e.dtype != torch.float32:
    e = e.float()
  if e.stride(2) != 1 or e.stride(0) < 0 or e.stride(1) < 0:
    e = e.contiguous()
  sz = _host.int32_vector(sizes, B, "sizes", device=dev)
  f32 = lambda t: (t if t.dtype == torch.float32 else t.float()).contiguous()
  ws_bytes = L.lr_rnnt_beam_workspace_bytes(B, V1, J, beam_width, max_symbols)
  ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
  out = dict(ids=torch.empty((B, nbest, width), dtype=torch.int32, device=dev),
             frames=torch.empty((B, nbest, width), dtype=torch.int32, device=dev),
             lens=torch.empty((B, nbest), dtype=torch.int32, device=dev),
             scores=torch.empty((B, nbest), dtype=torch.float32, device=dev),
             count=torch.empty(B, dtype=torch.int32, device=dev), truncated=st["truncated"], state=st)
  _host.launch(dev, "lr_rnnt_beam_decode", L.lr_rnnt_beam_decode, e.data_ptr(), e.stride(0), e.stride(1), _C.ptr(sz),
               f32(tables).data_ptr(), f32(joint_weight).data_ptr(), f32(joint_bias).data_ptr(),
               f32(class_mask).data_ptr(), st["buffer"].data_ptr(), st["buffer"].numel(), fresh,
               st["frame_base"].data_ptr(), out["ids"].data_ptr(), out["frames"].data_ptr(), out["lens"].data_ptr(),
               out["scores"].data_ptr(), out["count"].data_ptr(), st["truncated"].data_ptr(), ws.data_ptr(), ws_bytes,
               B, T, V1, J, context, beam_width, max_symbols, nbest, width)
  st["frame_base"] += (sz.clamp(0, T) if sz is not None else T)
  return out


class TransducerHead(nn.Module):
  """enc_proj, embed, pred_proj and joint of the transducer over `enc_dim`-wide encoder states (any encoder family:
  the head takes nothing but `hidden`).  vocab_size and char2idx as VideoEncoder takes them."""

  def __init__(self, enc_dim, vocab_size, char2idx, joint_dim=256, embed_dim=64, context=2):
    super().__init__()
    if context not in (1, 2):
      raise ValueError("context must be 1 or 2, got %r" % (context,))
    V1 = vocab_size + 1
    if V1 > MAX_CLASSES or joint_dim > MAX_JOINT:
      raise ValueError("TransducerHead: at most %d classes and a joint width of %d (got %d, %d)"
                       % (MAX_CLASSES, MAX_JOINT, V1, joint_dim))
    self.enc_dim, self.vocab_size, self.adj_vocab_size = enc_dim, vocab_size, V1
    self.joint_dim, self.embed_dim, self.context = joint_dim, embed_dim, context
    self.char2idx = char2idx
    self.best_error = 1
    self.enc_proj = nn.Linear(enc_dim, joint_dim)
    self.embed = nn.Embedding(V1, embed_dim)
    self.pred_proj = nn.Linear(context * embed_dim, joint_dim)
    self.joint = nn.Linear(joint_dim, V1)
    mask = torch.ones(V1)
    mask[char2idx[PAD] + 1] = 0
    mask[char2idx[BOS] + 1] = 0
    self.register_buffer("output_mask", mask, persistent=False)

  def tables(self):
    """(context, V1, J): table k row c = pred_proj.weight[:, kE:(k+1)E] . embed[c], the bias folded into table 0."""
    E = self.embed_dim
    tabs = [self.embed.weight @ self.pred_proj.weight[:, k * E:(k + 1) * E].t() for k in range(self.context)]
    tabs[0] = tabs[0] + self.pred_proj.bias
    return torch.stack(tabs, 0)

  def prediction(self, labels_p1):
    """p (B, U + 1, J) for labels (B, U): p_u from y_u, y_{u-1}, with y_j = 0 for j <= 0."""
    tabs = self.tables()
    B = labels_p1.shape[0]
    y = torch.cat((labels_p1.new_zeros((B, self.context)), labels_p1), dim=1).long().clamp(0, self.adj_vocab_size - 1)
    U1 = labels_p1.shape[1] + 1
    p = tabs[0][y[:, self.context - 1:self.context - 1 + U1]]
    if self.context == 2:
      p = p + tabs[1][y[:, 0:U1]]
    return p

  def loss(self, hidden, frame_lens, labels_p1, label_lens, reduction='mean'):
    """(loss, status, info) of rnnt_loss for the encoder's `hidden` (B, T, enc_dim) and the CTC labels
    (ctc.prepare_ctc_inputs: chars[:, 1:] + 1).  Differentiable in `hidden` and every parameter; no host read."""
    _C.require_cuda(hidden, frame_lens, labels_p1, label_lens)
    e = self.enc_proj(hidden)
    p = self.prediction(labels_p1)
    return rnnt_loss(e, p, self.joint.weight, self.joint.bias, self.output_mask, labels_p1, frame_lens, label_lens,
                     reduction)

  def greedy(self, hidden, sizes, state=None, max_symbols=5):
    """dict(ids, lens, frames, logp, forced, state), all device tensors, of rnnt_greedy: the greedy transcript of
    `hidden` (B, T, enc_dim), or of its next chunk when `state` is an earlier call's."""
    _C.require_cuda(hidden, sizes)
    with torch.no_grad():
      return rnnt_greedy(self.enc_proj(hidden), sizes, self.tables(), self.joint.weight, self.joint.bias,
                         self.output_mask, state=state, max_symbols=max_symbols)

  def beam(self, hidden, sizes, beam_width=8, max_symbols=3, nbest=None, state=None):
    """dict(ids, frames, lens, scores, count, truncated, state), all device tensors, of rnnt_beam: the N-best list of
    `hidden` (B, T, enc_dim), or of the clip so far when `state` is an earlier call's."""
    _C.require_cuda(hidden, sizes)
    with torch.no_grad():
      return rnnt_beam(self.enc_proj(hidden), sizes, self.tables(), self.joint.weight, self.joint.bias,
                       self.output_mask, beam_width=beam_width, max_symbols=max_symbols, nbest=nbest, state=state)

  def decode_strings(self, hidden, sizes, max_symbols=5, beam_width=0):
    """The transcripts as strings (EOS removed), after the one host read, as GreedyDecoder's: the greedy ones at
    beam_width 0, the beam search's top hypothesis at a positive beam_width."""
    from .decoder import ctc_labels
    labels = ctc_labels(self.char2idx)
    if beam_width > 0:
      out = self.beam(hidden, sizes, beam_width=beam_width, max_symbols=max_symbols, nbest=1)
      ids, lens = out["ids"][:, 0].cpu(), out["lens"][:, 0].cpu()
    else:
      out = self.greedy(hidden, sizes, max_symbols=max_symbols)
      ids, lens = out["ids"].cpu(), out["lens"].cpu()
    width = ids.shape[1]
    return [''.join(labels[int(c)] for c in ids[b, :min(int(lens[b]), width)]).replace(EOS, '')
            for b in range(ids.shape[0])]

  def save_best_model(self, error, file_path):
    import os
    if error < self.best_error:
      self.best_error = error
      folder = os.path.dirname(file_path)
      if folder and not os.path.exists(folder):
        os.makedirs(folder)
      torch.save(self.state_dict(), file_path)
