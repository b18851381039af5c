"""Look-ahead encoder sessions (lr_rnn_bistream_*): a BIDIRECTIONAL VideoEncoder fed chunk by chunk.

encoder_stream's sessions run causally and refuse a bidirectional encoder.  A LookaheadEncoderStream runs it as a
latency-controlled bidirectional RNN: one feed() hands every slot a window of frames, of which the slot consumes the
first sizes[b] and sees ahead[b] more.  The forward direction carries its state from advance to advance (the state
after the last CONSUMED frame); the backward direction restarts from zero at the end of the slot's window at every
advance and carries nothing.  The look-ahead frames are fed again, as consumed frames, later.  With R frames of
look-ahead the encoder adds R frames of latency; with all a slot has left as look-ahead at every advance the outputs
and the state are bit for bit the single advance over the whole utterance, which is the one-shot bidirectional model.

ChunkedLookaheadEncoder runs a whole padded batch through a session (what the evaluation loops take in a VideoEncoder's
place: the driver's --stream_lookahead=N), LookaheadTranscriber puts a session in front of a BeamStream.  Inference
only.
"""
import torch

from . import _C, _host
from .encoder import _MODES, _ptr_array


def _check_encoder(encoder, any_projection=False):
  """What a look-ahead session cannot run, by the encoder's own attributes: raises before any device work."""
  if getattr(encoder, "rnn", None) is None or getattr(encoder, "rnn_type", None) not in _MODES:
    raise TypeError("encoder must be a recurrent VideoEncoder (GRU / LSTM / RNN), got %s" % type(encoder).__name__)
  if not encoder.bidirectional:
    raise ValueError("encoder is uni-directional: there is nothing to look ahead for; use VideoEncoder.stream "
                     "(encoder_stream.EncoderStream)")
  if not any_projection and encoder.input_projection != 'f32':
    raise ValueError("encoder.input_projection is %r: a session runs the exact fp32 projection ('f32') only"
                     % (encoder.input_projection,))


class LookaheadEncoderStream(object):
  """`batch` slots of a bidirectional VideoEncoder's forward state.  feed() is layers x window step launches (both
  directions in each), one head launch and one commit launch on the current stream; read() / frames() are one launch
  and change nothing.  The weights are packed once, here: call refresh() after they change.  Use
  VideoEncoder.stream_lookahead()."""

  def __init__(self, encoder, batch, device, any_projection=False):
    _check_encoder(encoder, any_projection)
    self.any_projection = bool(any_projection)
    device = torch.device(device)
    if device.type != "cuda":
      raise _C.LipReadingHipError("lipreading_amd ops run on the MI355X only; got device %s (no CPU fallback)" % device)
    if int(batch) < 1:
      raise ValueError("batch must be >= 1, got %d" % batch)
    self.encoder, self.batch = encoder, int(batch)
    self.mode = _MODES[encoder.rnn_type]
    self.I, self.H, self.layers = int(encoder.frame_dim), int(encoder.hidden_size), int(encoder.num_layers)
    self.C = int(encoder.adj_vocab_size) if encoder.enable_ctc else 0
    self._weights()   # (a CPU encoder is refused before the library is touched)
    L = _C.lib()
    self.device = torch.device(device.type, _host.device_key(device)[1])
    nstate = L.lr_rnn_bistream_state_bytes(self.mode, self.batch, self.H, self.layers)
    npack = L.lr_rnn_bistream_pack_bytes(self.mode, self.I, self.H, self.layers)
    if nstate == 0 or npack == 0:
      raise _C.LipReadingHipError("lr_rnn_bistream: unsupported shape B=%d I=%d H=%d layers=%d"
                                  % (self.batch, self.I, self.H, self.layers))
    # zeroed, so that the bytes between the sections are equal from session to session
    self.state_buf = torch.zeros((nstate,), dtype=torch.uint8, device=self.device)
    self._pack = torch.zeros((npack,), dtype=torch.uint8, device=self.device)
    self._ws = _host.GrowingWorkspace()
    self.refresh()
    self.reset()

  def _weights(self):
    """[w_ih, w_hh, b_ih, b_hh] per (layer, direction), forward before backward, and the head."""
    ws = []
    for l in range(self.layers):
      lw = [p.detach() for p in self.encoder.rnn.layer_weights(l, 2)]
      ws += [lw[:4], lw[4:]]
    head = None
    if self.C:
      head = [self.encoder.output_proj.weight.detach(), self.encoder.output_proj.bias.detach(),
              self.encoder.output_mask.detach()]
    for t in [p for lw in ws for p in lw] + (head or []):
      if not t.is_cuda:
        raise _C.LipReadingHipError("encoder's weights are on %s: a session runs on the MI355X only (no CPU fallback)"
                                    % t.device)
      if t.dtype != torch.float32:
        raise TypeError("encoder's weights must be float32, got %s" % t.dtype)
    return [[p.contiguous() for p in lw] for lw in ws], (None if head is None else [p.contiguous() for p in head])

  def refresh(self):
    """Packs the encoder's weights as they are now (after an optimiser step or load_state_dict)."""
    ws, self._head = self._weights()
    cols = [[lw[i] for lw in ws] for i in range(4)]
    _host.launch(self.device, "lr_rnn_bistream_pack", _C.lib().lr_rnn_bistream_pack, self._pack.data_ptr(),
                 self._pack.numel(), self.mode, _ptr_array(cols[0]), _ptr_array(cols[1]), _ptr_array(cols[2]),
                 _ptr_array(cols[3]), self.I, self.H, self.layers)
    return self

  def reset(self, mask=None):
    """Slots with a non-zero `mask` entry ((batch,) on the device; None: all) go back to the zero state with 0 frames;
    the others keep every bit."""
    _C.require_cuda(mask)
    m = _host.int32_vector(mask if mask is None or mask.dtype != torch.bool else mask.int(), self.batch, "mask",
                           device=self.device)
    _host.launch(self.device, "lr_rnn_bistream_reset", _C.lib().lr_rnn_bistream_reset, self.state_buf.data_ptr(),
                 self.state_buf.numel(), _C.ptr(m), self.mode, self.batch, self.H, self.layers)
    return self

  def _frames_3d(self, frames):
    if not torch.is_tensor(frames):
      raise TypeError("frames must be a tensor, got %s" % type(frames).__name__)
    if frames.dtype != torch.float32:
      raise TypeError("frames must be float32, got %s" % frames.dtype)
    if frames.dim() == 4:
      frames = frames.reshape(frames.shape[0], frames.shape[1], -1)   # a view of a view such as frames[:, t0:t1]
    if frames.dim() != 3:
      raise ValueError("frames must be (batch, w, I) or (batch, w, landmarks, dims), got %s" % (tuple(frames.shape),))
    if frames.shape[0] != self.batch:
      raise ValueError("frames holds %d utterances, the session (batch) %d" % (frames.shape[0], self.batch))
    if frames.shape[2] != self.I:
      raise ValueError("frames has %d features per frame, the encoder's frame_dim (I) is %d" % (frames.shape[2], self.I))
    _C.require_cuda(frames)
    if frames.shape[1] > 0 and (frames.stride(2) != 1 or frames.stride(0) < 0 or frames.stride(1) < 0):
      frames = frames.contiguous()
    return frames

  def feed(self, frames, sizes=None, ahead=None, need_hidden=False, chunk=None):
    """One advance over a window: frames (batch, w, I) or (batch, w, landmarks, dims) fp32 (views go in without a copy),
    slot b consuming its first sizes[b] frames (None: min(chunk, w); 0: the slot keeps every bit) and seeing ahead[b]
    more behind them (None: 0; clamped to the window).  The rule for the rows returned: `chunk` of them (None: all w)
    — no slot consumes more than `chunk` frames, and nothing is copied to the host to find max(sizes).  Returns
    log_probs (batch, chunk, C) — at t >= sizes[b] the head of the zero row, as VideoEncoder.forward gives at padded
    positions — and with need_hidden (log_probs, hidden (batch, chunk, 2 H), zero at t >= sizes[b]); an encoder
    without a CTC head returns hidden alone."""
    x = self._frames_3d(frames)
    _C.require_cuda(sizes, ahead)
    B, W = self.batch, x.shape[1]
    T = W if chunk is None else int(chunk)
    if not 0 <= T <= W:
      raise ValueError("chunk must be in [0, %d] (the window), got %d" % (W, T))
    sz = _host.int32_vector(sizes, B, "sizes", device=self.device)
    ah = _host.int32_vector(ahead, B, "ahead", device=self.device)
    want_y = need_hidden or not self.C
    y = torch.empty((B, T, 2 * self.H), dtype=torch.float32, device=self.device) if want_y else None
    lp = torch.empty((B, T, self.C), dtype=torch.float32, device=self.device) if self.C else None
    if T > 0:
      L = _C.lib()
      nbytes = L.lr_rnn_bistream_workspace_bytes(self.mode, B, T, W, self.I, self.H, self.layers, self.C)
      if nbytes == 0:
        raise _C.LipReadingHipError("lr_rnn_bistream_advance: unsupported shape B=%d chunk_T=%d window_T=%d C=%d"
                                    % (B, T, W, self.C))
      ws = self._ws.get(self.device, nbytes)
      hw, hb, hm = self._head if self.C else (None, None, None)
      _host.launch(self.device, "lr_rnn_bistream_advance", L.lr_rnn_bistream_advance, self.mode, x.data_ptr(),
                   x.stride(0), x.stride(1), _C.ptr(sz), _C.ptr(ah), self._pack.data_ptr(), self._pack.numel(),
                   _C.ptr(hw), _C.ptr(hb), _C.ptr(hm), _C.ptr(y), _C.ptr(lp), self.state_buf.data_ptr(),
                   self.state_buf.numel(), ws.data_ptr(), ws.numel(), B, T, W, self.I, self.H, self.layers, self.C)
    if not self.C:
      return y
    return (lp, y) if need_hidden else lp

  def read(self):
    """(h (layers, batch, H), c or None, frames (batch,) int32, status (batch,) int32) on the device: one launch, and
    no byte of the state changes.  h and c are the FORWARD direction's halves after the last consumed frame: the
    backward direction's final state does not exist in a session (it would need the utterance's end), so there is no
    state() to hand a decoder as VideoEncoder.forward's final_state."""
    B, dev = self.batch, self.device
    h = torch.empty((self.layers, B, self.H), dtype=torch.float32, device=dev)
    c = torch.empty_like(h) if self.mode == _C.LR_RNN_LSTM else None
    meta = torch.empty((2, B), dtype=torch.int32, device=dev)
    _host.launch(dev, "lr_rnn_bistream_read", _C.lib().lr_rnn_bistream_read, self.state_buf.data_ptr(),
                 self.state_buf.numel(), h.data_ptr(), _C.ptr(c), meta[0].data_ptr(), meta[1].data_ptr(), B, self.H,
                 self.layers)
    return h, c, meta[0], meta[1]

  def frames(self):
    """Frames consumed per slot (look-ahead frames are not counted), (batch,) int32 on the device."""
    return self.read()[2]


class ChunkedLookaheadEncoder(object):
  """A bidirectional VideoEncoder's forward run through a look-ahead session: `chunk` frames consumed per advance,
  `lookahead` more seen.  The same arguments and returns as VideoEncoder.forward, except that there is no final state
  (None in its place; need_final_state=True raises), so train.ctc_cer and the other evaluation loops, which pass
  need_final_state=False, take it in the encoder's place.  lookahead >= the longest utterance is the one-shot model."""

  def __init__(self, encoder, chunk, lookahead, any_projection=False):
    _check_encoder(encoder, any_projection)
    self.any_projection = bool(any_projection)
    if int(chunk) < 1:
      raise ValueError("chunk must be >= 1, got %d" % chunk)
    if int(lookahead) < 0:
      raise ValueError("lookahead must be >= 0, got %d" % lookahead)
    self.encoder, self.chunk, self.lookahead = encoder, int(chunk), int(lookahead)
    self._streams = {}

  def __getattr__(self, name):
    return getattr(self.encoder, name)

  def __call__(self, frames, frame_lens, max_len=None, need_final_state=False, head_stream=None):
    if need_final_state:
      raise ValueError("a look-ahead session has no final_state: the backward direction restarts at every advance and "
                       "carries nothing (pass need_final_state=False)")
    _C.require_cuda(frames)
    if max_len is None:
      max_len = int(frame_lens.max())
    B, dev = frames.shape[0], frames.device
    assert 1 <= max_len <= frames.shape[1]
    key = (B, _host.device_key(dev))
    st = self._streams.get(key)
    if st is None:
      st = self._streams[key] = LookaheadEncoderStream(self.encoder, B, dev, self.any_projection)
    else:
      st.refresh().reset()
    lens = _host.int32_vector(frame_lens, B, "frame_lens", device=st.device)
    x = frames if frames.dtype == torch.float32 else frames.float()
    lps, hs = [], []
    for t0 in range(0, max_len, self.chunk):
      t1 = min(max_len, t0 + self.chunk + self.lookahead)
      n = min(self.chunk, max_len - t0)
      out = st.feed(x[:, t0:t1], (lens - t0).clamp_(0, n), (lens - t0 - n).clamp_(0, self.lookahead), need_hidden=True,
                    chunk=n)
      if st.C:
        lps.append(out[0])
        hs.append(out[1])
      else:
        hs.append(out)
    hidden = hs[0] if len(hs) == 1 else torch.cat(hs, dim=1)
    if st.C:
      return (lps[0] if len(lps) == 1 else torch.cat(lps, dim=1)), hidden, None
    return hidden, None


class LookaheadTranscriber(object):
  """A LookaheadEncoderStream in front of a BeamStream: feed() advances the encoder over a window and then the search
  on the consumed frames' log-probs; partial() / result() are the search's.  `max_frames` bounds an utterance, as in
  BeamCTCDecoder.stream."""

  def __init__(self, encoder, ctc_decoder, batch, max_frames, device):
    _check_encoder(encoder)
    if not encoder.enable_ctc:
      raise ValueError("encoder has no CTC head (enable_ctc=False): there is nothing to search")
    if not getattr(ctc_decoder, "log_probs_input", False):
      raise ValueError("ctc_decoder must take log-probabilities (log_probs_input=True): the encoder's head emits them")
    self.encoder_stream = LookaheadEncoderStream(encoder, batch, device)
    self.search = ctc_decoder.stream(batch, max_frames, device)

  def feed(self, frames, sizes=None, ahead=None, chunk=None):
    """As LookaheadEncoderStream.feed; the search is fed the `chunk` rows it returns with the same sizes."""
    lp = self.encoder_stream.feed(frames, sizes, ahead, chunk=chunk)
    if lp.shape[1]:
      self.search.feed(lp, sizes)
    return self

  def partial(self):
    return self.search.partial()

  def result(self):
    return self.search.result()

  def reset(self, mask=None):
    self.encoder_stream.reset(mask)
    self.search.reset(mask)
    return self
