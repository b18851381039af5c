"""Cases, the reference and the ABI helper of the encoder-session tests (tests/test_encoder_stream_cpu.py,
tests/test_gpu_encoder_stream.py).

The reference for every number is torch.nn.GRU / LSTM / RNN on the CPU, fed chunk by chunk with h0 / c0 carried
(stream_ref): one single-layer module per layer and slot, so that what a session must do at a chunk border — carry
every layer's state, hand layer 1 the SAME frame's output of layer 0, leave an idle slot alone, keep b_hn inside
r * (...) — is written out and can be got wrong on purpose (`variant`).

A plan is a list of operations: ("feed", chunk_T, sizes) — slot b consumes its next sizes[b] frames, chunk_T >= every
size — and ("reset", mask).
"""
import collections
import ctypes
import math

import torch

Case = collections.namedtuple("Case", "name cell I H layers B T C sat")
CASES = collections.OrderedDict((c.name, c) for c in [
    Case("gru20_i7", "GRU", 7, 20, 1, 1, 9, 5, False),       # I % 4 != 0, unaligned W_ih rows, partial unit tile, 3 K chunks
    Case("lstm36_b17", "LSTM", 12, 36, 2, 17, 40, 7, False),  # a second slot tile of one row, two layers, c carried
    Case("rnn16", "RNN", 4, 16, 1, 3, 5, 4, False),           # the one-gate cell
    Case("gru256", "GRU", 204, 256, 2, 4, 12, 65, False),     # the landmark regime: 29 K chunks
    Case("lstm700", "LSTM", 204, 700, 1, 2, 6, 29, False),    # defaults.txt: H % 16 != 0, 57 K chunks (second trip)
    Case("sat_gru", "GRU", 12, 20, 1, 5, 6, 5, True),         # pre-activations near +-30
    Case("sat_lstm", "LSTM", 12, 20, 1, 5, 6, 5, True),
])
GATES = {"GRU": 3, "LSTM": 4, "RNN": 1}
MODE = {"GRU": 0, "LSTM": 1, "RNN": 2}
BIT_CASES = ("lstm36_b17", "gru256")


def weights(case):
  """float32 weights of the stack and the head, torch.nn's layouts and initial range; the head mask has two zeros."""
  g = torch.Generator().manual_seed(1000 + sum(map(ord, case.name)))
  k = 1.0 / math.sqrt(case.H)
  GH = GATES[case.cell] * case.H

  def uni(*shape):
    return (torch.rand(*shape, generator=g) * 2 - 1) * k
  w = dict(w_ih=[], w_hh=[], b_ih=[], b_hh=[])
  for l in range(case.layers):
    w["w_ih"].append(uni(GH, case.I if l == 0 else case.H))
    w["w_hh"].append(uni(GH, case.H))
    w["b_ih"].append(uni(GH))
    w["b_hh"].append(uni(GH))
    if case.sat:
      w["b_ih"][l][0::4] += 30.0
      w["b_ih"][l][1::4] -= 30.0
  w["head_w"], w["head_b"] = uni(case.C, case.H), uni(case.C)
  mask = torch.ones(case.C)
  mask[1] = mask[case.C - 1] = 0
  w["head_mask"] = mask
  return w


def inputs(case):
  """x (B, T, I) float32 and ragged lens (B,): slot 0 has all T frames, the others fewer (never 0)."""
  g = torch.Generator().manual_seed(77 + sum(map(ord, case.name)))
  x = torch.randn(case.B, case.T, case.I, generator=g)
  lens = [case.T] + [1 + int(torch.randint(0, case.T, (1,), generator=g)) for _ in range(case.B - 1)]
  return x, lens


def one_chunk(case, lens):
  return [("feed", case.T, list(lens))]


def frame_by_frame(case, lens):
  return [("feed", 1, [1 if n > t else 0 for n in lens]) for t in range(case.T)]


def in_chunks(case, lens, chunks=(7, 1, 0, 13, 19)):
  plan, pos = [], 0
  for c in chunks:
    plan.append(("feed", c, [min(max(n - pos, 0), c) for n in lens]))
    pos += c
  assert pos >= case.T
  return plan


def ragged(case, lens, seed=5):
  """A different split per slot, slots idle for whole chunks included."""
  g = torch.Generator().manual_seed(seed)
  left, plan = list(lens), []
  while any(left):
    c = 1 + int(torch.randint(0, 6, (1,), generator=g))
    sizes = []
    for b in range(case.B):
      idle = int(torch.randint(0, 3, (1,), generator=g)) == 0
      n = 0 if idle else min(left[b], int(torch.randint(0, c + 1, (1,), generator=g)))
      sizes.append(n)
      left[b] -= n
    plan.append(("feed", c, sizes))
  assert case.B < 2 or any(0 in op[2] and any(op[2]) for op in plan)
  return plan


def _layer(case, w, l, dtype):
  cls = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM, "RNN": torch.nn.RNN}[case.cell]
  m = cls(case.I if l == 0 else case.H, case.H, 1, batch_first=True).to(dtype)
  with torch.no_grad():
    for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
      getattr(m, name.replace("w_", "weight_").replace("b_", "bias_") + "_l0").copy_(w[name][l].to(dtype))
  return m


def head(case, w, y, dtype):
  """masked log-softmax head; log(mask + 1e-45) is a float32 evaluation in both dtypes (-103.2789), as in the kernel"""
  lm = torch.log(w["head_mask"] + 1e-45).to(dtype)
  return torch.log_softmax(y.to(dtype) @ w["head_w"].to(dtype).t() + w["head_b"].to(dtype) + lm, dim=-1)


def fold_bhn(case, w):
  """the wrong variant `b_hn folded`: the GRU's b_hn moved out of r * (...) into b_in"""
  H = case.H
  w = dict(w, b_ih=[b.clone() for b in w["b_ih"]], b_hh=[b.clone() for b in w["b_hh"]])
  for l in range(case.layers):
    w["b_ih"][l][2 * H:] += w["b_hh"][l][2 * H:]
    w["b_hh"][l][2 * H:] = 0
  return w


def stream_ref(case, w, x, plan, dtype, variant=None):
  """dict(y (B, T, H) by each slot's own frame index, zero where nothing was fed; lp (B, T, C); h, c (layers, B, H)).
  variant: None, or one of the deliberately wrong 'idle_zeroed', 'c_not_reset', 'bhn_folded', 'layer1_prev_frame'."""
  if variant == "bhn_folded":
    w = fold_bhn(case, w)
  mods = [_layer(case, w, l, dtype) for l in range(case.layers)]
  B, T, H, Ls = case.B, case.T, case.H, case.layers
  x = x.to(dtype)
  h = torch.zeros(Ls, B, H, dtype=dtype)
  c = torch.zeros(Ls, B, H, dtype=dtype)
  last0 = torch.zeros(B, H, dtype=dtype)   # layer 0's output of the frame before (the wrong variant's input)
  y = torch.zeros(B, T, H, dtype=dtype)
  pos = [0] * B
  with torch.no_grad():
    for op in plan:
      if op[0] == "reset":
        for b in range(B):
          if op[1] is None or op[1][b]:
            h[:, b] = 0
            if variant != "c_not_reset":
              c[:, b] = 0
            last0[b] = 0
            y[b] = 0
            pos[b] = 0
        continue
      for b, n in enumerate(op[2]):
        assert 0 <= n <= op[1]
        if n == 0:
          if variant == "idle_zeroed":
            h[:, b] = 0
            c[:, b] = 0
          continue
        seq = x[b:b + 1, pos[b]:pos[b] + n]
        for l, m in enumerate(mods):
          if l == 1 and variant == "layer1_prev_frame":
            shifted = torch.cat((last0[b].view(1, 1, H), seq[:, :-1]), dim=1)
            last0[b] = seq[0, -1]
            seq = shifted
          h0 = h[l:l + 1, b:b + 1].contiguous()
          if case.cell == "LSTM":
            seq, (hn, cn) = m(seq, (h0, c[l:l + 1, b:b + 1].contiguous()))
            c[l, b] = cn[0, 0]
          else:
            seq, hn = m(seq, h0)
          h[l, b] = hn[0, 0]
        y[b, pos[b]:pos[b] + n] = seq[0]
        pos[b] += n
  return dict(y=y, lp=head(case, w, y, dtype), h=h, c=c if case.cell == "LSTM" else None)


def one_shot_ref(case, w, x, lens, dtype):
  """ONE packed-sequence torch.nn call of the whole stack over the whole utterances."""
  cls = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM, "RNN": torch.nn.RNN}[case.cell]
  m = cls(case.I, case.H, case.layers, batch_first=True).to(dtype)
  with torch.no_grad():
    for l in range(case.layers):
      for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
        getattr(m, name.replace("w_", "weight_").replace("b_", "bias_") + "_l%d" % l).copy_(w[name][l].to(dtype))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x.to(dtype), torch.tensor(lens), batch_first=True,
                                                     enforce_sorted=False)
    out, state = m(packed)
    y = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=case.T)[0]
  hn, cn = state if case.cell == "LSTM" else (state, None)
  return dict(y=y, lp=head(case, w, y, dtype), h=hn, c=cn)


def fed_rows(t, fed):
  """the rows (b, :fed[b]) of a (B, T, ...) tensor, stacked"""
  return torch.cat([t[b, :n] for b, n in enumerate(fed)], dim=0)


# ---- the ABI helper (GPU tests) -------------------------------------------------------------------------------------

GUARD = 64   # floats either side of y and log_probs


def ptr_array(tensors):
  return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class Session(object):
  """lr_rnn_stream_* called as the C ABI stands, on `dev`: pack, state, reset, advance with NaN-filled guarded
  outputs and a 0xFF-filled workspace, read."""

  def __init__(self, case, w, dev, B=None, with_head=True):
    from lipreading_amd import _C
    self.C_, self.L = _C, _C.lib()
    self.case, self.dev, self.B = case, dev, case.B if B is None else B
    self.mode = MODE[case.cell]
    self.wd = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in w.items()}
    self.with_head = with_head
    c = case
    self.pack = torch.zeros(self.L.lr_rnn_stream_pack_bytes(self.mode, c.I, c.H, c.layers), dtype=torch.uint8, device=dev)
    self.state = torch.zeros(self.L.lr_rnn_stream_state_bytes(self.mode, self.B, c.H, c.layers), dtype=torch.uint8,
                             device=dev)
    assert self.pack.numel() and self.state.numel()
    _C.check(self.L.lr_rnn_stream_pack(self.pack.data_ptr(), self.pack.numel(), self.mode, ptr_array(self.wd["w_ih"]),
                                       ptr_array(self.wd["w_hh"]), ptr_array(self.wd["b_ih"]),
                                       ptr_array(self.wd["b_hh"]), c.I, c.H, c.layers, _C.stream_handle()), "pack")
    self.reset()

  def reset(self, mask=None):
    m = None if mask is None else torch.tensor([int(v) for v in mask], dtype=torch.int32, device=self.dev)
    c = self.case
    self.C_.check(self.L.lr_rnn_stream_reset(self.state.data_ptr(), self.state.numel(), self.C_.ptr(m), self.mode,
                                             self.B, c.H, c.layers, self.C_.stream_handle()), "reset")

  def advance_raw(self, x, sizes, y, lp, ws, mode=None, H=None, layers=None, state_bytes=None, pack_bytes=None,
                  ws_bytes=None, T=None):
    """One lr_rnn_stream_advance; returns the status code."""
    c = self.case
    head = (self.wd["head_w"], self.wd["head_b"], self.wd["head_mask"]) if lp is not None else (None, None, None)
    P = self.C_.ptr
    return self.L.lr_rnn_stream_advance(
        self.mode if mode is None else mode, x.data_ptr(), x.stride(0), x.stride(1), P(sizes), self.pack.data_ptr(),
        self.pack.numel() if pack_bytes is None else pack_bytes, P(head[0]), P(head[1]), P(head[2]), P(y), P(lp),
        self.state.data_ptr(), self.state.numel() if state_bytes is None else state_bytes, ws.data_ptr(),
        ws.numel() if ws_bytes is None else ws_bytes, self.B, x.shape[1] if T is None else T, c.I, c.H if H is None else H,
        c.layers if layers is None else layers, c.C if lp is not None else 0, self.C_.stream_handle())

  def feed(self, xc, sizes):
    """xc (B, chunk_T, I) on the device (any strides with a unit feature stride), sizes a list or None -> (y, lp) with the
    guards checked."""
    c, B, T = self.case, self.B, xc.shape[1]
    sz = None if sizes is None else torch.tensor(sizes, dtype=torch.int32, device=self.dev)
    nws = self.L.lr_rnn_stream_workspace_bytes(self.mode, B, T, c.I, c.H, c.layers, c.C if self.with_head else 0)
    assert nws > 0
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=self.dev)
    ybuf = torch.full((2 * GUARD + B * T * c.H,), float("nan"), device=self.dev)
    lbuf = torch.full((2 * GUARD + B * T * c.C,), float("nan"), device=self.dev)
    y = ybuf[GUARD:GUARD + B * T * c.H].view(B, T, c.H)
    lp = lbuf[GUARD:GUARD + B * T * c.C].view(B, T, c.C) if self.with_head else None
    self.C_.check(self.advance_raw(xc, sz, y, lp, ws), "lr_rnn_stream_advance")
    for buf, n in ((ybuf, B * T * c.H), (lbuf, B * T * c.C)):
      assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), "a guard word was written"
    return y, lp

  def read(self):
    c, B = self.case, self.B
    h = torch.full((c.layers, B, c.H), float("nan"), device=self.dev)
    cc = torch.full((c.layers, B, c.H), float("nan"), device=self.dev) if c.cell == "LSTM" else None
    meta = torch.full((2, B), -7, dtype=torch.int32, device=self.dev)
    self.C_.check(self.L.lr_rnn_stream_read(self.state.data_ptr(), self.state.numel(), h.data_ptr(), self.C_.ptr(cc),
                                            meta[0].data_ptr(), meta[1].data_ptr(), B, c.H, c.layers,
                                            self.C_.stream_handle()), "lr_rnn_stream_read")
    return h, cc, meta[0], meta[1]

  def run(self, x, plan, read_between=False):
    """The plan on this session: x (B, T, I) on the host.  Unfed rows of a chunk are NaN.  Returns dict(y, lp by each
    slot's own frame index as stream_ref (lp rows no frame was fed for stay 0: compare fed_rows), h, c, frames,
    state = a copy of the state's bytes, fed = frames fed per slot, zero_row)."""
    c, B = self.case, self.B
    y = torch.zeros(B, c.T, c.H, device=self.dev)
    lp = torch.zeros(B, c.T, c.C, device=self.dev) if self.with_head else None
    pos = [0] * B
    zero_row = None   # log_probs of a row past a slot's frames (the head of the zero row), the first one met
    for op in plan:
      if op[0] == "reset":
        self.reset(op[1])
        for b in range(B):
          if op[1] is None or op[1][b]:
            pos[b] = 0
            y[b] = 0
        continue
      T = op[1]
      xc = torch.full((B, T, c.I), float("nan"))
      for b, n in enumerate(op[2]):
        xc[b, :n] = x[b, pos[b]:pos[b] + n]
      if T == 0:
        sz = torch.tensor(op[2], dtype=torch.int32, device=self.dev)
        ws = torch.full((max(1, self.L.lr_rnn_stream_workspace_bytes(self.mode, B, 0, c.I, c.H, c.layers, 0)),), 0xFF,
                        dtype=torch.uint8, device=self.dev)
        self.C_.check(self.advance_raw(torch.zeros(B, 1, c.I, device=self.dev), sz, None, None, ws, T=0),
                      "advance of no frame")
      else:
        yc, lc = self.feed(xc.to(self.dev), op[2])
        for b, n in enumerate(op[2]):
          y[b, pos[b]:pos[b] + n] = yc[b, :n]
          assert not yc[b, n:].any(), "y past a slot's frames is not zero"
          if lp is not None:
            lp[b, pos[b]:pos[b] + n] = lc[b, :n]
            if n < T:
              assert torch.equal(lc[b, n:], lc[b, n:n + 1].expand(T - n, -1)), "log_probs past a slot's frames"
              zero_row = lc[b, n].clone() if zero_row is None else zero_row
              assert torch.equal(zero_row, lc[b, n]), "log_probs past a slot's frames differ between slots"
          pos[b] += n
      if read_between:
        before = self.state.clone()
        self.read()
        assert torch.equal(before, self.state), "a read changed the state"
    h, cc, frames, status = self.read()
    assert not status.any(), status
    return dict(y=y, lp=lp, h=h, c=cc, frames=frames, state=self.state.clone(), fed=pos, zero_row=zero_row)
