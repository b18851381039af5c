"""Resumable encoder sessions (lr_rnn_stream_*): a uni-directional VideoEncoder fed chunk by chunk.

BeamCTCDecoder.stream resumes the search; these resume the model in front of it.  An EncoderStream holds, for `batch`
independent slots, the recurrent state of every layer in one device tensor; feed() takes the next frames of every slot
and returns their log-probabilities — the same bits however the utterance is cut, in whichever slot it sits.
ChunkedEncoder runs a whole padded batch through a session (what the evaluation loops take in a VideoEncoder's place),
LiveTranscriber puts a session in front of a BeamStream, and TwoPassTranscriber adds the attention decoder's second pass
over the search's N-best when the utterance ends.

Offline decoding of whole clips stays with VideoEncoder.forward and its one-launch recurrences: a session re-reads the
weights at every frame.  Inference only — nothing is kept for a backward.
"""
import torch

from . import _C, _host
from .encoder import _MODES, _ptr_array


def _check_encoder(encoder, any_projection=False):
  """What a session cannot run, by the encoder's own attributes: raises before any device work."""
  if getattr(encoder, "rnn", None) is None or getattr(encoder, "rnn_type", None) not in _MODES:
    raise TypeError("encoder must be a recurrent VideoEncoder (GRU / LSTM / RNN), got %s" % type(encoder).__name__)
  if encoder.bidirectional:
    raise ValueError("encoder is bidirectional: a session runs causally, which needs bidirectional=False")
  if not any_projection and encoder.input_projection != 'f32':
    raise ValueError("encoder.input_projection is %r: a session runs the exact fp32 projection ('f32') only"
                     % (encoder.input_projection,))


class EncoderStream(object):
  """`batch` slots of a uni-directional VideoEncoder's state.  feed() is layers x frames step launches, one head
  launch and one commit launch on the current stream; state() / frames() are one launch and change nothing.  The
  weights are packed once, here: call refresh() after they change.  Use VideoEncoder.stream()."""

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
    nstate = L.lr_rnn_stream_state_bytes(self.mode, self.batch, self.H, self.layers)
    npack = L.lr_rnn_stream_pack_bytes(self.mode, self.I, self.H, self.layers)
    if nstate == 0 or npack == 0:
      raise _C.LipReadingHipError("lr_rnn_stream: unsupported shape B=%d I=%d H=%d layers=%d"
                                  % (self.batch, self.I, self.H, self.layers))
    # zeroed, so that the bytes between the sections are equal from session to session
    self.state_buf = torch.zeros((nstate,), dtype=torch.uint8, device=self.device)
    self._pack = torch.zeros((npack,), dtype=torch.uint8, device=self.device)
    self._ws = _host.GrowingWorkspace()
    self.refresh()
    self.reset()

  def _weights(self):
    ws = [[p.detach() for p in self.encoder.rnn.layer_weights(l, 1)] for l in range(self.layers)]
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
    _host.launch(self.device, "lr_rnn_stream_pack", _C.lib().lr_rnn_stream_pack, self._pack.data_ptr(),
                 self._pack.numel(), self.mode, _ptr_array(cols[0]), _ptr_array(cols[1]), _ptr_array(cols[2]),
                 _ptr_array(cols[3]), self.I, self.H, self.layers)
    return self

  def reset(self, mask=None):
    """Slots with a non-zero `mask` entry ((batch,) on the device; None: all) go back to the zero state with 0 frames;
    the others keep every bit."""
    _C.require_cuda(mask)
    m = _host.int32_vector(mask if mask is None or mask.dtype != torch.bool else mask.int(), self.batch, "mask",
                           device=self.device)
    _host.launch(self.device, "lr_rnn_stream_reset", _C.lib().lr_rnn_stream_reset, self.state_buf.data_ptr(),
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
      raise ValueError("frames must be (batch, t, I) or (batch, t, landmarks, dims), got %s" % (tuple(frames.shape),))
    if frames.shape[0] != self.batch:
      raise ValueError("frames holds %d utterances, the session (batch) %d" % (frames.shape[0], self.batch))
    if frames.shape[2] != self.I:
      raise ValueError("frames has %d features per frame, the encoder's frame_dim (I) is %d" % (frames.shape[2], self.I))
    _C.require_cuda(frames)
    if frames.shape[1] > 0 and (frames.stride(2) != 1 or frames.stride(0) < 0 or frames.stride(1) < 0):
      frames = frames.contiguous()
    return frames

  def feed(self, frames, sizes=None, need_hidden=False):
    """One advance: frames (batch, t, I) or (batch, t, landmarks, dims) fp32, slot b consuming its first sizes[b]
    frames (None: all; 0: the slot is idle).  Returns log_probs (batch, t, C) — at t >= sizes[b] the head of the zero
    row, as VideoEncoder.forward gives at padded positions — and with need_hidden (log_probs, hidden (batch, t, H));
    an encoder without a CTC head returns hidden alone."""
    x = self._frames_3d(frames)
    _C.require_cuda(sizes)
    B, T = self.batch, x.shape[1]
    sz = _host.int32_vector(sizes, B, "sizes", device=self.device)
    want_y = need_hidden or not self.C
    y = torch.empty((B, T, self.H), dtype=torch.float32, device=self.device) if want_y else None
    lp = torch.empty((B, T, self.C), dtype=torch.float32, device=self.device) if self.C else None
    if T > 0:
      L = _C.lib()
      nbytes = L.lr_rnn_stream_workspace_bytes(self.mode, B, T, self.I, self.H, self.layers, self.C)
      if nbytes == 0:
        raise _C.LipReadingHipError("lr_rnn_stream_advance: unsupported shape B=%d chunk_T=%d C=%d" % (B, T, self.C))
      ws = self._ws.get(self.device, nbytes)
      hw, hb, hm = self._head if self.C else (None, None, None)
      _host.launch(self.device, "lr_rnn_stream_advance", L.lr_rnn_stream_advance, self.mode, x.data_ptr(), x.stride(0),
                   x.stride(1), _C.ptr(sz), self._pack.data_ptr(), self._pack.numel(), _C.ptr(hw), _C.ptr(hb),
                   _C.ptr(hm), _C.ptr(y), _C.ptr(lp), self.state_buf.data_ptr(), self.state_buf.numel(), ws.data_ptr(),
                   ws.numel(), B, T, self.I, self.H, self.layers, self.C)
    if not self.C:
      return y
    return (lp, y) if need_hidden else lp

  def read(self):
    """(h (layers, batch, H), c or None, frames (batch,) int32, status (batch,) int32) on the device: one launch, and
    no byte of the state changes."""
    B, dev = self.batch, self.device
    h = torch.empty((self.layers, B, self.H), dtype=torch.float32, device=dev)
    c = torch.empty_like(h) if self.mode == _C.LR_RNN_LSTM else None
    meta = torch.empty((2, B), dtype=torch.int32, device=dev)
    _host.launch(dev, "lr_rnn_stream_read", _C.lib().lr_rnn_stream_read, self.state_buf.data_ptr(),
                 self.state_buf.numel(), h.data_ptr(), _C.ptr(c), meta[0].data_ptr(), meta[1].data_ptr(), B, self.H,
                 self.layers)
    return h, c, meta[0], meta[1]

  def _raise_for(self, status):
    for b, s in enumerate(status):
      if s & _C.LR_RNN_STREAM_MISMATCH:
        raise _C.LipReadingHipError("lr_rnn_stream: slot %d has status %d (mismatch: a call's configuration is not the "
                                    "session's)" % (b, s))

  def state(self):
    """final_state as VideoEncoder.forward returns it for the frames fed so far: h (layers, batch, H), for the LSTM
    (h, c) — usable as CharDecodingStep's previous_state.  One device->host copy (the status words); a status bit raises
    LipReadingHipError naming the slot."""
    h, c, _, status = self.read()
    self._raise_for(status.cpu().tolist())
    return h if c is None else (h, c)

  def frames(self):
    """Frames consumed per slot, (batch,) int32 on the device."""
    return self.read()[2]


class ChunkedEncoder(object):
  """A uni-directional VideoEncoder's forward run through a session in chunks of `chunk` frames: the same arguments
  and returns, so train.ctc_cer and the other evaluation loops take it in the encoder's place.  Everything else
  (eval(), recurrence, enable_ctc ...) is the encoder's."""

  def __init__(self, encoder, chunk, any_projection=False):
    _check_encoder(encoder, any_projection)
    self.any_projection = bool(any_projection)
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
      st = self._streams[key] = EncoderStream(self.encoder, B, dev, self.any_projection)
    else:
      st.refresh().reset()
    lens = _host.int32_vector(frame_lens, B, "frame_lens", device=st.device)
    x = frames if frames.dtype == torch.float32 else frames.float()
    lps, hs = [], []
    for t0 in range(0, max_len, self.chunk):
      t1 = min(max_len, t0 + self.chunk)
      out = st.feed(x[:, t0:t1], (lens - t0).clamp_(0, t1 - t0), need_hidden=True)
      if st.C:
        lps.append(out[0])
        hs.append(out[1])
      else:
        hs.append(out)
    hidden = hs[0] if len(hs) == 1 else torch.cat(hs, dim=1)
    final_state = None
    if need_final_state:   # (read(), not state(): the session is this call's own, and nothing is copied to the host)
      h, c = st.read()[:2]
      final_state = h if c is None else (h, c)
    if st.C:
      return (lps[0] if len(lps) == 1 else torch.cat(lps, dim=1)), hidden, final_state
    return hidden, final_state


class LiveTranscriber(object):
  """An EncoderStream in front of a BeamStream: feed() advances the encoder and then the search on its log-probs;
  partial() / result() are the search's.  `max_frames` bounds an utterance, as in BeamCTCDecoder.stream."""

  def __init__(self, encoder, ctc_decoder, batch, max_frames, device):
    _check_encoder(encoder)
    if not encoder.enable_ctc:
      raise ValueError("encoder has no CTC head (enable_ctc=False): there is nothing to search")
    if not getattr(ctc_decoder, "log_probs_input", False):
      raise ValueError("ctc_decoder must take log-probabilities (log_probs_input=True): the encoder's head emits them")
    self.encoder_stream = EncoderStream(encoder, batch, device)
    self.search = ctc_decoder.stream(batch, max_frames, device)

  def feed(self, frames, sizes=None):
    lp = self.encoder_stream.feed(frames, sizes)
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


class TwoPassTranscriber(LiveTranscriber):
  """A LiveTranscriber that also keeps every slot's encoder states, (batch, max_frames, H) on the device, for the
  second pass of two-pass decoding: partial() / result() stay the CTC search's, live; when the
  utterances end, rescored() has the attention decoder rescore the search's N best hypotheses
  (CharDecodingStep.rescore) from the session's final state.  feed() writes each chunk at the slot's own frame offset
  without a host synchronisation.  `max_frames` is at most 1024, the longest hypothesis rescore takes.  An utterance
  longer than max_frames is an error, not a truncation: its later frames are not kept here, the search marks the slot
  (LR_BEAM_STREAM_OVERFLOW) while the encoder session's state goes on past them, and rescored() raises for that slot
  as result() does, until it is reset."""

  def __init__(self, encoder, decoding_step, ctc_decoder, batch, max_frames, device):
    if not 1 <= int(max_frames) <= 1024:
      raise ValueError("max_frames must be in [1, 1024] (the longest hypothesis rescore takes), got %d" % max_frames)
    super(TwoPassTranscriber, self).__init__(encoder, ctc_decoder, batch, max_frames, device)
    from .decoder import ctc_labels
    if list(ctc_decoder.labels) != ctc_labels(decoding_step.char2idx) or ctc_decoder.blank_index != 0:
      raise ValueError("ctc_decoder's labels must be decoder.ctc_labels(decoding_step.char2idx) with blank_index 0")
    if decoding_step.hidden_size != encoder.hidden_size or decoding_step.num_layers != encoder.num_layers:
      raise ValueError("decoding_step was not built for this encoder (hidden size or layers differ)")
    self.decoding_step = decoding_step
    st = self.encoder_stream
    self.max_frames = int(max_frames)
    # rows (slot, frame), plus one spare row at the end that takes the writes of idle positions (never read)
    self._rows = torch.zeros((st.batch * self.max_frames + 1, st.H), dtype=torch.float32, device=st.device)
    self._row0 = torch.arange(st.batch, device=st.device)[:, None] * self.max_frames
    self._at = torch.zeros((st.batch,), dtype=torch.int64, device=st.device)

  @property
  def hidden(self):
    """(batch, max_frames, H): each slot's encoder states so far, zero past its frames."""
    return self._rows[:-1].view(self.encoder_stream.batch, self.max_frames, self.encoder_stream.H)

  def feed(self, frames, sizes=None):
    st = self.encoder_stream
    lp, y = st.feed(frames, sizes, need_hidden=True)
    t = lp.shape[1]
    if t:
      self.search.feed(lp, sizes)
      step = torch.arange(t, device=st.device)[None, :]
      took = (torch.full((st.batch,), t, device=st.device) if sizes is None
              else sizes.to(device=st.device, dtype=torch.int64).clamp(0, t))
      pos = self._at[:, None] + step
      row = torch.where((step < took[:, None]) & (pos < self.max_frames), self._row0 + pos,
                        pos.new_tensor(st.batch * self.max_frames))
      self._rows.index_copy_(0, row.reshape(-1), y.reshape(-1, st.H))
      self._at = (self._at + took).clamp_(max=self.max_frames)
    return self

  def reset(self, mask=None):
    super(TwoPassTranscriber, self).reset(mask)
    if mask is None:
      self._rows.zero_()
      self._at.zero_()
    else:
      keep = (mask.to(self._at.device) == 0)
      self.hidden.mul_(keep[:, None, None].to(self._rows.dtype))
      self._at.mul_(keep.to(self._at.dtype))
    return self

  def rescored_ids(self, nbest=10, ctc_weight=0.5, length_bonus=0.0):
    """The second pass on the device: (ids, offsets, lens, scores, attn_scores, status) with the search's `nbest`
    best hypotheses reordered by CharDecodingStep.rescore — ids / offsets (batch, nbest, max_frames), the rest
    (batch, nbest) and status (2, batch), the search's and the encoder session's: read_ids(nbest),
    encoder_stream.read() and one rescore call."""
    ids, off, lens, first, _, _, status = self.search.read_ids(nbest, self.max_frames)
    h, c, frames, estatus = self.encoder_stream.read()
    order, scores, attn = self.decoding_step.rescore(self.hidden, frames, h if c is None else (h, c), ids, lens, first,
                                                     ctc_weight=ctc_weight, length_bonus=length_bonus)
    o = order.long()
    wide = o[:, :, None].expand(-1, -1, ids.shape[2])
    return (torch.gather(ids, 1, wide), torch.gather(off, 1, wide), torch.gather(lens, 1, o), scores, attn,
            torch.stack((status, estatus)))

  def rescored(self, nbest=10, ctc_weight=0.5, length_bonus=0.0):
    """(strings, offsets) in BeamCTCDecoder.decode's contract, the `nbest` best hypotheses of the first pass in the
    second pass's order (best first).  A status bit of either session raises LipReadingHipError."""
    ids, off, lens, _, _, status = self.rescored_ids(nbest, ctc_weight, length_bonus)
    status = status.cpu().tolist()
    self.search._raise_for(status[0])
    self.encoder_stream._raise_for(status[1])
    return self.search.decoder._strings(ids, off, lens)
