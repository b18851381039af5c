"""Resumable transformer encoder sessions (lr_tfm_stream_*): a chunk-limited TransformerVideoEncoder fed
chunk by chunk.

encoder_stream resumes a recurrent encoder, frontend_stream the conv frontend, BeamCTCDecoder.stream the search.  A
TransformerStream resumes the transformer: it holds, for `batch` independent slots, the input frames of the attention
chunk that is not whole yet and every layer's keys and values of the last attn_left_chunks * attn_chunk positions in
one device tensor.  feed() takes the next frames of every slot and returns the rows of the chunks they complete — what
TransformerVideoEncoder.forward computes on the whole clip under the same chunk mask, the same bits however the clip is
cut, in whichever slot it sits.  A row trails its frame by at most attn_chunk - 1 frames, whatever the depth.

Only a model trained under the mask can be cached: with attn_chunk = 0 every frame of every layer looks at the whole
clip, and no record of the past reproduces that.  ChunkedTransformerEncoder runs a whole padded batch through a session
(what the evaluation loops take in the encoder's place: the driver's --stream_tfm=True), TransformerLiveTranscriber is
frames — or, with a conv frontend, pixels — in, transcript out.

Arithmetic is exact fp32 (fp32 products, softmax and cache), whatever the encoder's one-shot modes are.  Offline work
on whole clips stays with TransformerVideoEncoder.forward.  Inference only — nothing is kept for a backward.
"""
import math

import torch

from . import _C, _host
from .encoder import _ptr_array


def count_rule(n, ended, chunk):
  """E(n, ended): rows a slot has emitted after n frames."""
  return n if ended else (n // chunk) * chunk


def _check_encoder(encoder):
  """What a session cannot run, by the encoder's own attributes: raises before any device work."""
  from .transformer import TransformerVideoEncoder
  if not isinstance(encoder, TransformerVideoEncoder):
    raise TypeError("encoder must be a TransformerVideoEncoder, got %s" % type(encoder).__name__)
  if encoder.attn_chunk < 1:
    raise ValueError("encoder.attn_chunk is 0: a full-attention model cannot be cached (every frame of every layer "
                     "attends to the whole clip, so no record of the past reproduces it); build and train it with "
                     "attn_chunk >= 1")


class TransformerStream(object):
  """`batch` slots of a chunk-limited TransformerVideoEncoder's pending frames and key / value rings.  feed() is
  5 + 7 x layers launches on the current stream; read() / frames() are one launch and change nothing.  The weights are
  read in place at every advance: refresh() only re-collects their pointers (after load_state_dict on new tensors).
  Use TransformerVideoEncoder.stream()."""

  def __init__(self, encoder, batch, device):
    _check_encoder(encoder)
    device = torch.device(device)
    if device.type != "cuda":
      raise _C.LipReadingHipError("lipreading_amd ops run on the MI355X only; got device %s (no CPU fallback)" % device)
    if int(batch) < 1:
      raise ValueError("batch must be >= 1, got %d" % batch)
    self.encoder, self.batch = encoder, int(batch)
    self.I, self.Dm, self.nhead = int(encoder.frame_dim), int(encoder.d_model), int(encoder.nhead)
    self.F, self.layers = int(encoder.layers[0].linear1.out_features), len(encoder.layers)
    self.chunk, self.left = int(encoder.attn_chunk), int(encoder.attn_left_chunks)
    self.eps = float(encoder.layers[0].norm1.eps)
    self.C = int(encoder.adj_vocab_size) if encoder.enable_ctc else 0
    self._collect()   # (a CPU encoder is refused before the library is touched)
    L = _C.lib()
    self.device = torch.device(device.type, _host.device_key(device)[1])
    self._cfg = (self.I, self.Dm, self.nhead, self.F, self.layers, self.chunk, self.left)
    nstate = L.lr_tfm_stream_state_bytes(self.batch, *self._cfg)
    if nstate == 0:
      raise _C.LipReadingHipError("lr_tfm_stream: unsupported shape B=%d I=%d d_model=%d heads=%d feed-forward=%d layers=%d "
                                  "chunk=%d left_chunks=%d (1 <= chunk <= 32, (left_chunks + 1) * chunk <= 128, head "
                                  "dimension a multiple of 4 and <= 64)" % ((self.batch,) + self._cfg))
    # zeroed, so that the bytes between the sections are equal from session to session
    self.state_buf = torch.zeros((nstate,), dtype=torch.uint8, device=self.device)
    self._ws = _host.GrowingWorkspace()
    self.refresh()
    self.reset()

  def _collect(self):
    enc = self.encoder
    ws = [enc.input_proj.weight, enc.input_proj.bias]
    for layer in enc.layers:
      at = layer.self_attn
      ws += [at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias, layer.linear1.weight,
             layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm1.weight, layer.norm1.bias,
             layer.norm2.weight, layer.norm2.bias]
    head = [enc.output_proj.weight, enc.output_proj.bias, enc.output_mask] if self.C else []
    ws, head, pe = [p.detach() for p in ws], [p.detach() for p in head], enc.pe.detach()
    for t in ws + head + [pe]:
      if not t.is_cuda:
        raise _C.LipReadingHipError("encoder's weights are on %s: a session runs on the MI355X only (no CPU fallback)"
                                    % t.device)
      if t.dtype != torch.float32:
        raise TypeError("encoder's weights must be float32, got %s" % t.dtype)
    return [p.contiguous() for p in ws], [p.contiguous() for p in head] or None, pe.contiguous()

  def refresh(self):
    """Takes the encoder's weight tensors as they are now."""
    self._weights, self._head, self._pe = self._collect()
    return self

  def reset(self, mask=None):
    """Slots with a non-zero `mask` entry ((batch,) on the device; None: all) go back to no pending frame, zero rings,
    0 frames, not ended; the others keep every bit."""
    _C.require_cuda(mask)
    m = _host.int32_vector(mask if mask is None or mask.dtype != torch.bool else mask.int(), self.batch, "mask",
                           device=self.device)
    _host.launch(self.device, "lr_tfm_stream_reset", _C.lib().lr_tfm_stream_reset, self.state_buf.data_ptr(),
                 self.state_buf.numel(), _C.ptr(m), self.batch, *self._cfg)
    return self

  def _frames_3d(self, frames):
    if not torch.is_tensor(frames):
      raise TypeError("frames must be a tensor, got %s" % type(frames).__name__)
    if frames.dtype != torch.float32:
      raise TypeError("frames must be float32, got %s" % frames.dtype)
    if frames.dim() > 3:
      frames = frames.reshape(frames.shape[0], frames.shape[1], math.prod(frames.shape[2:]))   # a view where it can be
    if frames.dim() != 3:
      raise ValueError("frames must be (batch, t, I) or (batch, t, ...), got %s" % (tuple(frames.shape),))
    if frames.shape[0] != self.batch:
      raise ValueError("frames holds %d utterances, the session (batch) %d" % (frames.shape[0], self.batch))
    if frames.shape[2] != self.I:
      raise ValueError("frames has %d features per frame, the encoder's frame_dim (I) is %d" % (frames.shape[2], self.I))
    _C.require_cuda(frames)
    if frames.shape[1] > 0 and (frames.stride(2) != 1 or frames.stride(0) < 0 or frames.stride(1) < 0):
      frames = frames.contiguous()
    return frames

  def feed(self, frames, sizes=None, end=None, need_hidden=False):
    """One advance: frames (batch, t, I) fp32 — a view such as frames[:, t0:t1] goes in without a copy —, slot b
    consuming its first sizes[b] frames (None: all; 0: the slot is idle and keeps every bit); end (batch,) or None:
    non-zero = the slot's stream ends with these frames (t = 0: a flush).  Returns (log_probs (batch, rows, C), counts
    (batch,) int32) with rows = t + attn_chunk - 1: slot b's newly completed rows packed from row 0, at and past
    counts[b] the head of the zero row; with need_hidden (log_probs, hidden (batch, rows, d_model), counts), zero rows
    past counts[b]; an encoder without a CTC head returns (hidden, counts)."""
    x = self._frames_3d(frames)
    _C.require_cuda(sizes, end)
    B, T = self.batch, x.shape[1]
    sz = _host.int32_vector(sizes, B, "sizes", device=self.device)
    en = _host.int32_vector(end if end is None or end.dtype != torch.bool else end.int(), B, "end", device=self.device)
    rows = T + self.chunk - 1
    want_h = need_hidden or not self.C
    h = torch.empty((B, rows, self.Dm), dtype=torch.float32, device=self.device) if want_h else None
    lp = torch.empty((B, rows, self.C), dtype=torch.float32, device=self.device) if self.C else None
    counts = torch.zeros((B,), dtype=torch.int32, device=self.device)
    L = _C.lib()
    nbytes = L.lr_tfm_stream_workspace_bytes(B, T, self.I, self.Dm, self.nhead, self.F, self.layers, self.C, self.chunk,
                                             self.left)
    if nbytes == 0:
      raise _C.LipReadingHipError("lr_tfm_stream_advance: unsupported shape B=%d chunk_T=%d C=%d" % (B, T, self.C))
    ws = self._ws.get(self.device, nbytes)
    hw, hb, hm = self._head if self.C else (None, None, None)
    _host.launch(self.device, "lr_tfm_stream_advance", L.lr_tfm_stream_advance, x.data_ptr() if T else None, x.stride(0),
                 x.stride(1), _C.ptr(sz), _C.ptr(en), _ptr_array(self._weights), self._pe.data_ptr(), self._pe.shape[0],
                 _C.ptr(hw), _C.ptr(hb), _C.ptr(hm), _C.ptr(h), _C.ptr(lp), counts.data_ptr(), self.state_buf.data_ptr(),
                 self.state_buf.numel(), ws.data_ptr(), ws.numel(), B, T, self.I, self.Dm, self.nhead, self.F, self.layers,
                 self.C, self.chunk, self.left, self.eps)
    if not self.C:
      return h, counts
    return (lp, h, counts) if need_hidden else (lp, counts)

  def read(self):
    """(frames consumed, rows emitted, ended, status), each (batch,) int32 on the device: one launch, and no byte of
    the state changes."""
    meta = torch.empty((4, self.batch), dtype=torch.int32, device=self.device)
    _host.launch(self.device, "lr_tfm_stream_read", _C.lib().lr_tfm_stream_read, self.state_buf.data_ptr(),
                 self.state_buf.numel(), meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(), meta[3].data_ptr(),
                 self.batch, *self._cfg)
    return meta[0], meta[1], meta[2], meta[3]

  def check(self):
    """One device->host copy (the status words): a status bit raises LipReadingHipError naming the slot."""
    for b, s in enumerate(self.read()[3].cpu().tolist()):
      names = [name for name, bit in (("mismatch: a call's configuration is not the slot's", _C.LR_TFM_STREAM_MISMATCH),
                                      ("frames were fed after the slot's stream had ended: reset the slot first",
                                       _C.LR_TFM_STREAM_AFTER_END),
                                      ("full: the slot's frames would pass the positional table's %d rows"
                                       % self._pe.shape[0], _C.LR_TFM_STREAM_FULL)) if s & bit]
      if names:
        raise _C.LipReadingHipError("lr_tfm_stream: slot %d has status %d (%s)" % (b, s, "; ".join(names)))
    return self

  def frames(self):
    """Frames consumed per slot, (batch,) int32 on the device."""
    return self.read()[0]


def _place(out, rows, counts, emitted):
  """out (B, Tmax + 1, W) <- the packed rows of one advance at rows emitted[b] .. emitted[b] + counts[b] - 1; rows past
  counts[b] go to the spare last row.  Torch ops only: nothing is copied to the host."""
  r = torch.arange(rows.shape[1], device=rows.device, dtype=torch.int64)[None, :]
  idx = torch.where(r < counts[:, None], emitted[:, None].to(torch.int64) + r, out.shape[1] - 1)
  idx = idx.clamp_(max=out.shape[1] - 1)
  out.scatter_(1, idx[:, :, None].expand(-1, -1, rows.shape[2]), rows)


class ChunkedTransformerEncoder(object):
  """A chunk-limited TransformerVideoEncoder's forward run through a session in pieces of `chunk` frames (any size: it
  need not be the attention chunk): the same arguments and returns, so train.ctc_cer and the other evaluation loops
  take it in the encoder's place.  Rows at t >= frame_lens[b] are the zero row (its head in log_probs).  Everything else
  (eval(), enable_ctc ...) is the encoder's."""

  def __init__(self, encoder, chunk):
    _check_encoder(encoder)
    if int(chunk) < 1:
      raise ValueError("chunk must be >= 1, got %d" % chunk)
    self.encoder, self.chunk = encoder, int(chunk)
    self._streams = {}

  def __getattr__(self, name):
    return getattr(self.encoder, name)

  def __call__(self, frames, frame_lens, max_len=None, need_final_state=True, head_stream=None):
    _C.require_cuda(frames)
    if max_len is None:
      max_len = int(frame_lens.max())
    B, dev = frames.shape[0], frames.device
    assert 1 <= max_len <= frames.shape[1]
    key = (B, _host.device_key(dev))
    st = self._streams.get(key)
    if st is None:
      st = self._streams[key] = TransformerStream(self.encoder, B, dev)
    else:
      st.refresh().reset()
    lens = _host.int32_vector(frame_lens, B, "frame_lens", device=st.device).clamp(max=max_len)
    x = frames.reshape(B, frames.shape[1], math.prod(frames.shape[2:]))
    x = x if x.dtype == torch.float32 else x.float()
    hidden = torch.zeros((B, max_len + 1, st.Dm), dtype=torch.float32, device=st.device)
    lps = torch.empty((B, max_len + 1, st.C), dtype=torch.float32, device=st.device) if st.C else None
    emitted = torch.zeros((B,), dtype=torch.int32, device=st.device)
    if st.C:
      # rows at t >= frame_lens[b]: the head of the zero row (no decoder given the lengths reads them)
      enc = self.encoder
      lps[:] = torch.log_softmax(enc.output_proj.bias.detach() + torch.log(enc.output_mask.detach() + 1e-45), dim=0)
    for t0 in range(0, max_len, self.chunk):
      t1 = min(max_len, t0 + self.chunk)
      out = st.feed(x[:, t0:t1], (lens - t0).clamp_(0, t1 - t0), ((lens > t0) & (lens <= t1)).int(), need_hidden=True)
      h, counts = out[-2], out[-1]
      _place(hidden, h, counts, emitted)
      if st.C:
        _place(lps, out[0], counts, emitted)
      emitted = emitted + counts
    hidden[:, max_len].zero_()
    if st.C:
      return lps[:, :max_len], hidden[:, :max_len], None
    return hidden[:, :max_len], None


class ChunkedTransformerPixelLipReader(object):
  """A PixelLipReader's forward (conv frontend + chunk-limited transformer encoder) run through sessions:
  frontend_stream.ChunkedFrontend, then ChunkedTransformerEncoder.  The same arguments and returns as
  PixelLipReader.forward, so the evaluation loops take it in the model's place.  The frontend's features are bf16
  values: the session's exact fp32 products of them are what the one-shot model's 'bf16x3' projection approximates."""

  def __init__(self, model, chunk):
    from .frontend_stream import ChunkedFrontend
    if getattr(model, "frontend", None) is None or getattr(model, "encoder", None) is None:
      raise TypeError("model must be a PixelLipReader, got %s" % type(model).__name__)
    self.model, self.chunk = model, int(chunk)
    self.chunked_frontend = ChunkedFrontend(model.frontend, chunk)
    self.chunked_encoder = ChunkedTransformerEncoder(model.encoder, chunk)

  def __getattr__(self, name):
    return getattr(self.model, name)

  def __call__(self, clips, frame_lens, max_len=None, need_final_state=True, head_stream=None):
    if max_len is None:
      max_len = int(frame_lens.max())
    feats = self.chunked_frontend(clips, frame_lens, max_len=max_len)
    return self.chunked_encoder(feats, frame_lens, max_len=max_len, need_final_state=False)


class TransformerLiveTranscriber(object):
  """Frames — or, with a conv frontend, pixels — in, transcript out: an optional FrontendStream feeds a
  TransformerStream — with its counts as the sizes and its `end` forwarded — which feeds a BeamStream.
  `model_or_encoder` is a chunk-limited TransformerVideoEncoder with a CTC head, or a PixelLipReader around one (then
  height and width are the clips'); `max_frames` bounds an utterance, as in BeamCTCDecoder.stream.  The transcript
  trails the input by at most attn_chunk - 1 frames (and the frontend's 3) until `end`."""

  def __init__(self, model_or_encoder, ctc_decoder, batch, max_frames, device, height=None, width=None):
    model = model_or_encoder
    pixels = getattr(model, "frontend", None) is not None and getattr(model, "encoder", None) is not None
    encoder = model.encoder if pixels else model
    _check_encoder(encoder)
    if not encoder.enable_ctc:
      raise ValueError("encoder has no CTC head (enable_ctc=False): there is nothing to search")
    if not getattr(ctc_decoder, "log_probs_input", False):
      raise ValueError("ctc_decoder must take log-probabilities (log_probs_input=True): the encoder's head emits them")
    self.frontend_stream = None
    if pixels:
      from .frontend_stream import FrontendStream
      if height is None or width is None:
        raise ValueError("a PixelLipReader needs the clips' height and width")
      self.frontend_stream = FrontendStream(model.frontend, batch, height, width, device)
    elif height is not None or width is not None:
      raise ValueError("height and width go with a PixelLipReader (a conv frontend in front of the encoder)")
    self.encoder_stream = TransformerStream(encoder, batch, device)
    self.search = ctc_decoder.stream(batch, max_frames, device)

  def feed(self, frames, sizes=None, end=None):
    if self.frontend_stream is not None:
      frames, sizes = self.frontend_stream.feed(frames, sizes, end)
    lp, counts = self.encoder_stream.feed(frames, sizes, end)
    if lp.shape[1]:
      self.search.feed(lp, counts)
    return self

  def partial(self):
    return self.search.partial()

  def result(self):
    return self.search.result()

  def check(self):
    if self.frontend_stream is not None:
      self.frontend_stream.check()
    self.encoder_stream.check()
    return self

  def reset(self, mask=None):
    if self.frontend_stream is not None:
      self.frontend_stream.reset(mask)
    self.encoder_stream.reset(mask)
    self.search.reset(mask)
    return self
