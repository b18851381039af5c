"""Resumable conv frontend sessions (lr_conv_stream_*): ConvFrontend3D fed chunk by chunk.

encoder_stream and encoder_lookahead resume the encoder, BeamCTCDecoder.stream the search; all three start from
features.  A FrontendStream starts from pixels: it holds, for `batch` independent slots, the last two input frames of
each of the three convolutions in one device tensor; feed() takes the next frames of every slot and returns the feature
frames they complete — the same bits however the clip is cut, in whichever slot it sits.  Every convolution looks one
frame ahead, so feature frame t needs clip frames up to t + 3: a running slot has emitted max(0, n - 3) features after n
frames, and `end` hands out the last three (the frames after the last one are the zero padding).

A slot's features are ConvFrontend3D's on that slot's clip ALONE.  ConvFrontend3D.forward on a PADDED batch lets the
padding frames reach the last two feature frames of a shorter clip; a session has no padding to see.  The two agree on
unpadded clips.

ChunkedFrontend runs a whole padded batch through a session, ChunkedPixelLipReader puts it in front of a chunked encoder
(what the evaluation loops take in a PixelLipReader's place: the driver's --stream_frontend=True), PixelLiveTranscriber
is pixels in, transcript out: FrontendStream -> EncoderStream -> BeamStream.

Offline work on whole clips stays with ConvFrontend3D.forward and its tuned kernels.  Inference only — nothing is kept
for a backward.
"""
import torch

from . import _C, _host
from .frontend import LAYERS, ConvFrontend3D, _pack_weights, _pad4, feature_dim

LOOKAHEAD = 3   # clip frames a feature frame waits for


def _check_frontend(frontend):
  if not isinstance(frontend, ConvFrontend3D):
    raise TypeError("frontend must be a ConvFrontend3D, got %s" % type(frontend).__name__)


class FrontendStream(object):
  """`batch` slots of a ConvFrontend3D's frame rings at (height, width).  feed() is one plan launch, one ingest launch,
  three conv launches and two commit launches on the current stream; read() / frames() are one launch and change
  nothing.  The weights are packed once, here: call refresh() after they change.  Use ConvFrontend3D.stream()."""

  def __init__(self, frontend, batch, height, width, device):
    _check_frontend(frontend)
    device = torch.device(device)
    if device.type != "cuda":
      raise _C.LipReadingHipError("lipreading_amd ops run on the MI355X only; got device %s (no CPU fallback)" % device)
    if int(batch) < 1:
      raise ValueError("batch must be >= 1, got %d" % batch)
    self.H, self.W = int(height), int(width)
    if self.H < 16 or self.W < 16 or self.H % 16 or self.W % 16:
      raise ValueError("height and width must be positive multiples of 16, got %d x %d" % (self.H, self.W))
    self.frontend, self.batch = frontend, int(batch)
    self.F = feature_dim(self.H, self.W)
    self._params()   # (a CPU frontend is refused before the library is touched)
    L = _C.lib()
    self.device = torch.device(device.type, _host.device_key(device)[1])
    nstate = L.lr_conv_stream_state_bytes(self.batch, self.H, self.W)
    if nstate == 0:
      raise _C.LipReadingHipError("lr_conv_stream: unsupported shape B=%d H=%d W=%d" % (self.batch, self.H, self.W))
    self.state_buf = torch.zeros((nstate,), dtype=torch.uint8, device=self.device)
    self._w = [torch.zeros((cout, kt * kh * kw, _pad4(cin)), dtype=torch.bfloat16, device=self.device)
               for cin, cout, (kt, kh, kw), _, _ in LAYERS]
    self._ws = _host.GrowingWorkspace()
    self.refresh()
    self.reset()

  def _params(self):
    ps = [p.detach() for p in self.frontend.parameters_in_order()]
    for t in ps:
      if not t.is_cuda:
        raise _C.LipReadingHipError("frontend's weights are on %s: a session runs on the MI355X only (no CPU fallback)"
                                    % t.device)
      if t.dtype != torch.float32:
        raise TypeError("frontend's weights must be float32, got %s" % t.dtype)
    return [p.contiguous() for p in ps]

  def refresh(self):
    """Packs the frontend's weights as they are now (after an optimiser step or load_state_dict): one launch."""
    ps = self._params()
    self._bias = [ps[1], ps[3], ps[5]]
    packs = [(ps[2 * li], self._w[li], cout, cin, _pad4(cin), kt, kh, kw, 0)
             for li, (cin, cout, (kt, kh, kw), _, _) in enumerate(LAYERS)]
    with torch.cuda.device(self.device):
      _pack_weights(_C.lib(), packs, _C.stream_handle())
    return self

  def reset(self, mask=None):
    """Slots with a non-zero `mask` entry ((batch,) on the device; None: all) go back to empty rings, 0 frames, not
    ended; the others keep every bit."""
    _C.require_cuda(mask)
    m = _host.int32_vector(mask if mask is None or mask.dtype != torch.bool else mask.int(), self.batch, "mask",
                           device=self.device)
    _host.launch(self.device, "lr_conv_stream_reset", _C.lib().lr_conv_stream_reset, self.state_buf.data_ptr(),
                 self.state_buf.numel(), _C.ptr(m), self.batch, self.H, self.W)
    return self

  def _clips_5d(self, clips):
    if not torch.is_tensor(clips):
      raise TypeError("clips must be a tensor, got %s" % type(clips).__name__)
    if clips.dtype not in (torch.uint8, torch.float32):
      raise TypeError("clips must be uint8 or float32, got %s" % clips.dtype)
    if clips.dim() != 5:
      raise ValueError("clips must be (batch, t, 3, H, W), got %s" % (tuple(clips.shape),))
    if clips.shape[0] != self.batch:
      raise ValueError("clips holds %d utterances, the session (batch) %d" % (clips.shape[0], self.batch))
    if clips.shape[2] != 3:
      raise ValueError("clips has %d channels, the frontend takes 3" % clips.shape[2])
    if tuple(clips.shape[3:]) != (self.H, self.W):
      raise ValueError("clips are %d x %d, the session %d x %d" % (clips.shape[3], clips.shape[4], self.H, self.W))
    _C.require_cuda(clips)
    if clips.shape[1] > 0 and (tuple(clips.stride()[2:]) != (self.H * self.W, self.W, 1) or clips.stride(0) < 0 or
                               clips.stride(1) < 0):
      clips = clips.contiguous()
    return clips

  def feed(self, clips, sizes=None, end=None):
    """One advance: clips (batch, t, 3, H, W) uint8 (scaled by 1/255 on the device) or fp32 — a view such as
    clips[:, t0:t1] goes in without a copy —, slot b consuming its first sizes[b] frames (None: all; 0: the slot is idle
    and keeps every bit); end (batch,) or None: non-zero = the slot's stream ends with these frames (t = 0: a flush).
    Returns (features (batch, t + 3 if end is given else t, F) fp32, counts (batch,) int32): slot b's newly completed
    feature frames packed from row 0, zero rows at and past counts[b]."""
    x = self._clips_5d(clips)
    _C.require_cuda(sizes, end)
    B, T = self.batch, x.shape[1]
    sz = _host.int32_vector(sizes, B, "sizes", device=self.device)
    en = _host.int32_vector(end if end is None or end.dtype != torch.bool else end.int(), B, "end", device=self.device)
    rows = T + (LOOKAHEAD if en is not None else 0)
    feat = torch.empty((B, rows, self.F), dtype=torch.float32, device=self.device)
    counts = torch.zeros((B,), dtype=torch.int32, device=self.device)
    if rows > 0:
      L = _C.lib()
      nbytes = L.lr_conv_stream_workspace_bytes(B, T, self.H, self.W)
      if nbytes == 0:
        raise _C.LipReadingHipError("lr_conv_stream_advance: unsupported shape B=%d chunk_T=%d" % (B, T))
      ws = self._ws.get(self.device, nbytes)
      _host.launch(self.device, "lr_conv_stream_advance", L.lr_conv_stream_advance, x.data_ptr() if T else None,
                   _C.LR_CONV_STREAM_F32 if x.dtype == torch.float32 else 0, x.stride(0), x.stride(1), _C.ptr(sz),
                   _C.ptr(en), self._w[0].data_ptr(), self._w[1].data_ptr(), self._w[2].data_ptr(),
                   self._bias[0].data_ptr(), self._bias[1].data_ptr(), self._bias[2].data_ptr(), feat.data_ptr(),
                   counts.data_ptr(), self.state_buf.data_ptr(), self.state_buf.numel(), ws.data_ptr(), ws.numel(), B, T,
                   self.H, self.W)
    return feat, counts

  def read(self):
    """(frames consumed, features emitted, ended, status), each (batch,) int32 on the device: one launch, and no byte
    of the state changes."""
    meta = torch.empty((4, self.batch), dtype=torch.int32, device=self.device)
    _host.launch(self.device, "lr_conv_stream_read", _C.lib().lr_conv_stream_read, self.state_buf.data_ptr(),
                 self.state_buf.numel(), meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(), meta[3].data_ptr(),
                 self.batch, self.H, self.W)
    return meta[0], meta[1], meta[2], meta[3]

  def check(self):
    """One device->host copy (the status words): a status bit raises LipReadingHipError naming the slot."""
    for b, s in enumerate(self.read()[3].cpu().tolist()):
      if s & _C.LR_CONV_STREAM_MISMATCH:
        raise _C.LipReadingHipError("lr_conv_stream: slot %d has status %d (mismatch: a call's height or width is not "
                                    "the session's)" % (b, s))
      if s & _C.LR_CONV_STREAM_AFTER_END:
        raise _C.LipReadingHipError("lr_conv_stream: slot %d has status %d (frames were fed after the slot's stream had "
                                    "ended: reset the slot first)" % (b, s))
    return self

  def frames(self):
    """Frames consumed per slot, (batch,) int32 on the device."""
    return self.read()[0]


def _place(out, feat, counts, emitted):
  """out (B, Tmax + 1, F) <- the packed rows of one advance at rows emitted[b] .. emitted[b] + counts[b] - 1; rows past
  counts[b] (zeros) go to the spare last row.  Torch ops only: nothing is copied to the host."""
  rows = feat.shape[1]
  r = torch.arange(rows, device=feat.device, dtype=torch.int64)[None, :]
  idx = torch.where(r < counts[:, None], emitted[:, None].to(torch.int64) + r, out.shape[1] - 1)
  idx = idx.clamp_(max=out.shape[1] - 1)
  out.scatter_(1, idx[:, :, None].expand(-1, -1, feat.shape[2]), feat)


class ChunkedFrontend(object):
  """A ConvFrontend3D's forward run through a session in chunks of `chunk` frames: (clips (B, T, 3, H, W), frame_lens)
  -> features (B, Tmax, F) fp32 with zero rows at t >= frame_lens[b] — each slot's features are those of its own clip
  alone (see the module's note on padded batches).  Every slot ends with its last frames."""

  def __init__(self, frontend, chunk):
    _check_frontend(frontend)
    if int(chunk) < 1:
      raise ValueError("chunk must be >= 1, got %d" % chunk)
    self.frontend, self.chunk = frontend, int(chunk)
    self._streams = {}

  def __call__(self, clips, frame_lens, max_len=None):
    _C.require_cuda(clips)
    if max_len is None:
      max_len = clips.shape[1]
    B, dev = clips.shape[0], clips.device
    assert clips.dim() == 5 and 1 <= max_len <= clips.shape[1]
    key = (B, int(clips.shape[3]), int(clips.shape[4]), _host.device_key(dev))
    st = self._streams.get(key)
    if st is None:
      st = self._streams[key] = FrontendStream(self.frontend, B, clips.shape[3], clips.shape[4], dev)
    else:
      st.refresh().reset()
    lens = _host.int32_vector(frame_lens, B, "frame_lens", device=st.device).clamp(max=max_len)
    out = torch.zeros((B, max_len + 1, st.F), dtype=torch.float32, device=st.device)
    emitted = torch.zeros((B,), dtype=torch.int32, device=st.device)
    for t0 in range(0, max_len, self.chunk):
      t1 = min(max_len, t0 + self.chunk)
      feat, counts = st.feed(clips[:, t0:t1], (lens - t0).clamp_(0, t1 - t0), ((lens > t0) & (lens <= t1)).int())
      _place(out, feat, counts, emitted)
      emitted = emitted + counts
    out[:, max_len].zero_()
    return out[:, :max_len]


class ChunkedPixelLipReader(object):
  """A PixelLipReader's forward run through sessions: ChunkedFrontend, then ChunkedEncoder (lookahead None: a
  uni-directional encoder) or ChunkedLookaheadEncoder (lookahead an int: a bidirectional one).  The same arguments and
  returns as PixelLipReader.forward, so the evaluation loops take it in the model's place.  Everything else (eval(),
  enable_ctc ...) is the model's."""

  def __init__(self, model, chunk, lookahead=None):
    from .encoder_lookahead import ChunkedLookaheadEncoder
    from .encoder_stream import ChunkedEncoder
    if getattr(model, "frontend", None) is None or getattr(model, "encoder", None) is None:
      raise TypeError("model must be a PixelLipReader, got %s" % type(model).__name__)
    self.model, self.chunk, self.lookahead = model, int(chunk), lookahead
    self.chunked_frontend = ChunkedFrontend(model.frontend, chunk)
    # the frontend's features are bf16 values: the session's exact fp32 products of them are what the one-shot
    # model's 'bf16x3' projection approximates
    if lookahead is None:
      self.chunked_encoder = ChunkedEncoder(model.encoder, chunk, any_projection=True)
    else:
      self.chunked_encoder = ChunkedLookaheadEncoder(model.encoder, chunk, int(lookahead), any_projection=True)

  def __getattr__(self, name):
    return getattr(self.model, name)

  def __call__(self, clips, frame_lens, max_len=None, need_final_state=True, head_stream=None):
    if max_len is None:
      max_len = int(frame_lens.max())
    feats = self.chunked_frontend(clips, frame_lens, max_len=max_len)
    if self.lookahead is not None:
      need_final_state = False
    return self.chunked_encoder(feats, frame_lens, max_len=max_len, need_final_state=need_final_state)


class PixelLiveTranscriber(object):
  """Pixels in, transcript out: a FrontendStream feeds an EncoderStream — with its counts as the sizes — which feeds a
  BeamStream.  `model` is a PixelLipReader with a uni-directional recurrent encoder and a CTC head; `max_frames` bounds
  an utterance, as in BeamCTCDecoder.stream.  The transcript trails the camera by the frontend's 3 frames until `end`."""

  def __init__(self, model, ctc_decoder, batch, max_frames, height, width, device):
    from .encoder_stream import EncoderStream, _check_encoder
    if getattr(model, "frontend", None) is None or getattr(model, "encoder", None) is None:
      raise TypeError("model must be a PixelLipReader, got %s" % type(model).__name__)
    _check_encoder(model.encoder, any_projection=True)   # (a transformer encoder is refused here)
    if not model.encoder.enable_ctc:
      raise ValueError("encoder has no CTC head (enable_ctc=False): there is nothing to search")
    if not getattr(ctc_decoder, "log_probs_input", False):
      raise ValueError("ctc_decoder must take log-probabilities (log_probs_input=True): the encoder's head emits them")
    self.frontend_stream = FrontendStream(model.frontend, batch, height, width, device)
    self.encoder_stream = EncoderStream(model.encoder, batch, device, any_projection=True)
    self.search = ctc_decoder.stream(batch, max_frames, device)

  def feed(self, clips, sizes=None, end=None):
    feat, counts = self.frontend_stream.feed(clips, sizes, end)
    if feat.shape[1]:
      lp = self.encoder_stream.feed(feat, counts)
      self.search.feed(lp, counts)
    return self

  def partial(self):
    return self.search.partial()

  def result(self):
    return self.search.result()

  def reset(self, mask=None):
    self.frontend_stream.reset(mask)
    self.encoder_stream.reset(mask)
    self.search.reset(mask)
    return self
