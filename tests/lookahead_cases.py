"""Cases, the reference and the ABI helper of the look-ahead session tests (tests/test_lookahead_cpu.py,
tests/test_gpu_lookahead.py).

The reference for every number is torch.nn.GRU / LSTM / RNN on the CPU (lc_ref): one single-layer, single-direction
module per (layer, direction), run slot by slot, so that every rule of a look-ahead advance is written out and can be
got wrong on purpose (`variant`):
  * the forward direction starts from the slot's carried state, runs over the consumed AND the look-ahead frames, and
    commits the state after the last consumed frame;
  * the backward direction starts from zero at the end of the slot's own window and carries nothing;
  * an upper layer's input is [fwd | bwd] of the same frame, look-ahead frames included.

A plan is a list of operations: ("feed", chunk_T, window_T, sizes, ahead) — slot b consumes its next sizes[b] frames
and sees ahead[b] more; sizes[b] <= chunk_T and sizes[b] + ahead[b] <= window_T — and ("reset", mask).
"""
import collections
import ctypes
import math

import torch

Case = collections.namedtuple("Case", "name cell I H layers B T C sat")
CASES = collections.OrderedDict((c.name, c) for c in [
    Case("bigru20_i7", "GRU", 7, 20, 1, 1, 9, 5, False),        # unaligned rows, partial unit tile
    Case("bilstm36_b17", "LSTM", 12, 36, 2, 17, 40, 7, False),  # a second slot tile of one row; the padded seam between
                                                                # the directions in layer 1's K; c across the look-ahead
    Case("birnn16", "RNN", 4, 16, 2, 3, 5, 4, False),           # the one-gate cell
    Case("bigru256", "GRU", 204, 256, 2, 4, 12, 65, False),     # regime R; upper layer K = 512 + 256
    Case("bilstm700", "LSTM", 204, 700, 1, 2, 6, 29, False),    # H % 16 != 0, head over K = 1400
    Case("sat_bilstm", "LSTM", 12, 20, 1, 5, 6, 5, True),       # pre-activations near +-30
])
GATES = {"GRU": 3, "LSTM": 4, "RNN": 1}
MODE = {"GRU": 0, "LSTM": 1, "RNN": 2}
BIT_CASES = ("bilstm36_b17", "bigru256")
VARIANTS = ("carry_bwd", "commit_late", "window_end", "blind_upper", "swapped")
FULL = "full"


def weights(case):
  """float32 weights of the stack (w_ih ... [2 l + d], d = 0 forward, 1 backward) and the head over 2 H, torch.nn's
  layouts and initial range; the head mask has two zeros."""
  g = torch.Generator().manual_seed(2000 + sum(map(ord, case.name)))
  k = 1.0 / math.sqrt(case.H)
  GH = GATES[case.cell] * case.H

  def uni(*shape):
    return (torch.rand(*shape, generator=g) * 2 - 1) * k
  w = dict(w_ih=[], w_hh=[], b_ih=[], b_hh=[])
  for l in range(case.layers):
    for d in range(2):
      w["w_ih"].append(uni(GH, case.I if l == 0 else 2 * case.H))
      w["w_hh"].append(uni(GH, case.H))
      w["b_ih"].append(uni(GH))
      w["b_hh"].append(uni(GH))
      if case.sat:
        w["b_ih"][-1][0::4] += 30.0
        w["b_ih"][-1][1::4] -= 30.0
  w["head_w"], w["head_b"] = uni(case.C, 2 * case.H), uni(case.C)
  mask = torch.ones(case.C)
  mask[1] = mask[case.C - 1] = 0
  w["head_mask"] = mask
  return w


def inputs(case):
  """x (B, T, I) float32 and ragged lens (B,): slot 0 has all T frames, the others fewer (never 0)."""
  g = torch.Generator().manual_seed(177 + sum(map(ord, case.name)))
  x = torch.randn(case.B, case.T, case.I, generator=g)
  lens = [case.T] + [1 + int(torch.randint(0, case.T - 1, (1,), generator=g)) for _ in range(case.B - 1)]
  return x, lens


# ---- plans -----------------------------------------------------------------------------------------------------------

def one_chunk(case, lens):
  return [("feed", case.T, case.T, list(lens), [0] * len(lens))]


def blocks(chunk, lookahead):
  """`chunk` frames consumed per advance, `lookahead` more seen (FULL: all a slot has left)."""
  def plan(case, lens):
    ops = []
    for t0 in range(0, case.T, chunk):
      c = min(chunk, case.T - t0)
      w = case.T - t0 if lookahead == FULL else min(chunk + lookahead, case.T - t0)
      sizes = [min(max(n - t0, 0), c) for n in lens]
      ahead = [min(max(n - t0 - c, 0), w - c if lookahead == FULL else lookahead) for n in lens]
      ops.append(("feed", c, w, sizes, ahead))
    return ops
  plan.__name__ = "blocks_%d_%s" % (chunk, lookahead)
  return plan


blocks_5_3 = blocks(5, 3)
blocks_1_0 = blocks(1, 0)
blocks_4_full = blocks(4, FULL)
frame_by_frame_full = blocks(1, FULL)
frame_by_frame_full.__name__ = "frame_by_frame_full"


def ragged(case, lens, seed=5):
  """A different split and look-ahead per slot; idle slots (0, 0) and look-only slots (0 consumed, some seen)."""
  g = torch.Generator().manual_seed(seed)

  def rnd(n):
    return int(torch.randint(0, n, (1,), generator=g))
  left, plan = list(lens), []
  while any(left):
    c = 1 + rnd(6)
    w = c + rnd(5)
    sizes, ahead = [], []
    for b in range(len(lens)):
      kind = rnd(4)   # 0: idle, 1: look-only, else: consume
      n = 0 if kind < 2 else min(left[b], rnd(c + 1))
      a = 0 if kind == 0 else min(left[b] - n, rnd(w - n + 1))
      sizes.append(n)
      ahead.append(a)
      left[b] -= n
    plan.append(("feed", c, w, sizes, ahead))
  if len(lens) >= 3:
    feeds = [(n, a) for op in plan for n, a in zip(op[3], op[4])]
    assert any(n == 0 and a > 0 for n, a in feeds) and any(n > 0 and a > 0 for n, a in feeds)
    assert any((0, 0) in zip(op[3], op[4]) and any(op[3]) for op in plan)
  return plan


PLANS = dict(one_chunk=one_chunk, blocks_5_3=blocks_5_3, blocks_1_0=blocks_1_0, blocks_4_full=blocks_4_full,
             frame_by_frame_full=frame_by_frame_full, ragged=ragged)


# ---- the reference ---------------------------------------------------------------------------------------------------

def _module(case, w, l, d, dtype):
  cls = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM, "RNN": torch.nn.RNN}[case.cell]
  m = cls(case.I if l == 0 else 2 * case.H, case.H, 1, batch_first=True).to(dtype)
  with torch.no_grad():
    for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
      getattr(m, name.replace("w_", "weight_").replace("b_", "bias_") + "_l0").copy_(w[name][2 * l + d].to(dtype))
  return m


def head(case, w, y, dtype):
  """masked log-softmax head over 2 H; log(mask + 1e-45) is a float32 evaluation in both dtypes, as in the kernel"""
  lm = torch.log(w["head_mask"] + 1e-45).to(dtype)
  return torch.log_softmax(y.to(dtype) @ w["head_w"].to(dtype).t() + w["head_b"].to(dtype) + lm, dim=-1)


def _run(case, m, seq, state):
  """one module over seq (1, n, K) from state (h (1, 1, H), c or None) -> (out (1, n, H), state after the last frame)"""
  if seq.shape[1] == 0:
    return seq.new_zeros(1, 0, case.H), state
  if case.cell == "LSTM":
    out, (h, c) = m(seq, (state[0].contiguous(), state[1].contiguous()))
    return out, (h, c)
  out, h = m(seq, state[0].contiguous())
  return out, (h, None)


def lc_ref(case, w, x, plan, dtype, variant=None):
  """dict(y (B, T, 2 H) by each slot's own frame index, zero where nothing was consumed; lp (B, T, C); h, c
  (layers, B, H): the forward direction's committed state; frames: consumed per slot).
  variant: None, or one of the deliberately wrong VARIANTS:
    carry_bwd    the backward state is kept across advances
    commit_late  the forward state is committed after the look-ahead
    window_end   the backward direction starts at window_T - 1, not at e_b - 1 (over the frames that lie there)
    blind_upper  the upper layers' look-ahead frames see zeros from the layer below
    swapped      the upper layers' input is [bwd | fwd]"""
  assert variant is None or variant in VARIANTS
  mods = [[_module(case, w, l, d, dtype) for d in range(2)] for l in range(case.layers)]
  B, T, H, Ls = len(x), case.T, case.H, case.layers
  lstm = case.cell == "LSTM"
  x = x.to(dtype)
  h = torch.zeros(Ls, B, H, dtype=dtype)
  c = torch.zeros(Ls, B, H, dtype=dtype)
  bh = torch.zeros(Ls, B, H, dtype=dtype)   # carry_bwd only: what the backward direction ended the last advance with
  bc = torch.zeros(Ls, B, H, dtype=dtype)
  y = torch.zeros(B, T, 2 * H, dtype=dtype)
  pos = [0] * B
  with torch.no_grad():
    for op in plan:
      if op[0] == "reset":
        for b in range(B):
          if op[1] is None or op[1][b]:
            h[:, b] = 0
            c[:, b] = 0
            bh[:, b] = 0
            bc[:, b] = 0
            y[b] = 0
            pos[b] = 0
        continue
      _, chunk_T, window_T, sizes, ahead = op
      assert chunk_T <= window_T
      for b in range(B):
        n, a = sizes[b], ahead[b]
        assert 0 <= n <= chunk_T and 0 <= a <= window_T - n
        if n == 0:
          continue                       # idle or look-only: nothing is returned and nothing committed
        e = n + a
        inp = x[b:b + 1, pos[b]:pos[b] + e]
        assert inp.shape[1] == e, "the plan looks past the frames there are"
        if variant == "window_end":      # the frames that lie between e and the window's end (zeros past x)
          e = window_T
          more = x[b:b + 1, pos[b] + n + a:pos[b] + window_T]
          inp = torch.cat((inp, more, x.new_zeros(1, window_T - n - a - more.shape[1], case.I)), dim=1)
        for l in range(Ls):
          if l > 0 and variant == "blind_upper":
            inp = torch.cat((inp[:, :n], torch.zeros_like(inp[:, n:])), dim=1)
          st0 = (h[l:l + 1, b:b + 1], c[l:l + 1, b:b + 1] if lstm else None)
          out1, st1 = _run(case, mods[l][0], inp[:, :n], st0)
          out2, st2 = _run(case, mods[l][0], inp[:, n:], st1)          # the look-ahead frames, from the same state
          keep = st2 if variant == "commit_late" else st1
          h[l, b] = keep[0][0, 0]
          if lstm:
            c[l, b] = keep[1][0, 0]
          zero = torch.zeros(1, 1, H, dtype=dtype)
          bst0 = (bh[l:l + 1, b:b + 1], bc[l:l + 1, b:b + 1] if lstm else None) if variant == "carry_bwd" else \
                 (zero, zero if lstm else None)
          outb, bst = _run(case, mods[l][1], inp.flip(1), bst0)
          bh[l, b] = bst[0][0, 0]
          if lstm:
            bc[l, b] = bst[1][0, 0]
          parts = (torch.cat((out1, out2), dim=1), outb.flip(1))
          inp = torch.cat(parts[::-1] if variant == "swapped" else parts, dim=2)
        if variant == "swapped":         # (the rule is about what an upper layer is fed: y keeps torch's order)
          inp = torch.cat((inp[..., H:], inp[..., :H]), dim=2)
        y[b, pos[b]:pos[b] + n] = inp[0, :n]
        pos[b] += n
  return dict(y=y, lp=head(case, w, y, dtype), h=h, c=c if lstm else None, frames=list(pos))


def one_shot_ref(case, w, x, lens, dtype):
  """ONE packed-sequence call of torch.nn's bidirectional stack over the whole utterances; h / c are the forward
  direction's final states."""
  cls = {"GRU": torch.nn.GRU, "LSTM": torch.nn.LSTM, "RNN": torch.nn.RNN}[case.cell]
  m = cls(case.I, case.H, case.layers, batch_first=True, bidirectional=True).to(dtype)
  with torch.no_grad():
    for l in range(case.layers):
      for d, suffix in enumerate(("", "_reverse")):
        for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
          attr = name.replace("w_", "weight_").replace("b_", "bias_") + "_l%d%s" % (l, suffix)
          getattr(m, attr).copy_(w[name][2 * l + d].to(dtype))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x.to(dtype), torch.tensor(lens), batch_first=True,
                                                     enforce_sorted=False)
    out, state = m(packed)
    y = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=case.T)[0]
  hn, cn = state if case.cell == "LSTM" else (state, None)
  fwd = lambda s: s.view(case.layers, 2, len(lens), case.H)[:, 0].contiguous()   # noqa: E731
  return dict(y=y, lp=head(case, w, y, dtype), h=fwd(hn), c=None if cn is None else fwd(cn), frames=list(lens))


def fed_rows(t, fed):
  """the rows (b, :fed[b]) of a (B, T, ...) tensor, stacked"""
  return torch.cat([t[b, :n] for b, n in enumerate(fed)], dim=0)


# ---- the ABI helper (GPU tests) -------------------------------------------------------------------------------------

GUARD = 64   # floats either side of y and log_probs


def ptr_array(tensors):
  return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class Session(object):
  """lr_rnn_bistream_* called as the C ABI stands, on `dev`: pack, state, reset, advance with NaN-filled guarded
  outputs and a 0xFF-filled workspace, read."""

  def __init__(self, case, w, dev, B=None, with_head=True):
    from lipreading_amd import _C
    self.C_, self.L = _C, _C.lib()
    self.case, self.dev, self.B = case, dev, case.B if B is None else B
    self.mode = MODE[case.cell]
    self.wd = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in w.items()}
    self.with_head = with_head
    c = case
    self.pack = torch.zeros(self.L.lr_rnn_bistream_pack_bytes(self.mode, c.I, c.H, c.layers), dtype=torch.uint8,
                            device=dev)
    self.state = torch.zeros(self.L.lr_rnn_bistream_state_bytes(self.mode, self.B, c.H, c.layers), dtype=torch.uint8,
                             device=dev)
    assert self.pack.numel() and self.state.numel()
    _C.check(self.L.lr_rnn_bistream_pack(self.pack.data_ptr(), self.pack.numel(), self.mode,
                                         ptr_array(self.wd["w_ih"]), ptr_array(self.wd["w_hh"]),
                                         ptr_array(self.wd["b_ih"]), ptr_array(self.wd["b_hh"]), c.I, c.H, c.layers,
                                         _C.stream_handle()), "pack")
    self.reset()

  def reset(self, mask=None):
    m = None if mask is None else torch.tensor([int(v) for v in mask], dtype=torch.int32, device=self.dev)
    c = self.case
    self.C_.check(self.L.lr_rnn_bistream_reset(self.state.data_ptr(), self.state.numel(), self.C_.ptr(m), self.mode,
                                               self.B, c.H, c.layers, self.C_.stream_handle()), "reset")

  def advance_raw(self, x, sizes, ahead, y, lp, ws, chunk_T, mode=None, H=None, layers=None, state=None,
                  state_bytes=None, pack_bytes=None, ws_bytes=None, window_T=None):
    """One lr_rnn_bistream_advance over the window x (B, window_T, I); returns the status code."""
    c = self.case
    head_ = (self.wd["head_w"], self.wd["head_b"], self.wd["head_mask"]) if lp is not None else (None, None, None)
    P = self.C_.ptr
    state = self.state if state is None else state
    return self.L.lr_rnn_bistream_advance(
        self.mode if mode is None else mode, x.data_ptr(), x.stride(0), x.stride(1), P(sizes), P(ahead),
        self.pack.data_ptr(), self.pack.numel() if pack_bytes is None else pack_bytes, P(head_[0]), P(head_[1]),
        P(head_[2]), P(y), P(lp), state.data_ptr(), state.numel() if state_bytes is None else state_bytes,
        ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, self.B, chunk_T,
        x.shape[1] if window_T is None else window_T, c.I, c.H if H is None else H,
        c.layers if layers is None else layers, c.C if lp is not None else 0, self.C_.stream_handle())

  def feed(self, xw, chunk_T, sizes, ahead):
    """xw (B, window_T, I) on the device (any strides with a unit feature stride), sizes / ahead lists or None ->
    (y (B, chunk_T, 2 H), lp (B, chunk_T, C)) with the guards checked."""
    c, B, W, T = self.case, self.B, xw.shape[1], chunk_T
    sz = None if sizes is None else torch.tensor(sizes, dtype=torch.int32, device=self.dev)
    ah = None if ahead is None else torch.tensor(ahead, dtype=torch.int32, device=self.dev)
    nws = self.L.lr_rnn_bistream_workspace_bytes(self.mode, B, T, W, c.I, c.H, c.layers, c.C if self.with_head else 0)
    assert nws > 0
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=self.dev)
    ny, nl = B * T * 2 * c.H, B * T * c.C
    ybuf = torch.full((2 * GUARD + ny,), float("nan"), device=self.dev)
    lbuf = torch.full((2 * GUARD + nl,), float("nan"), device=self.dev)
    y = ybuf[GUARD:GUARD + ny].view(B, T, 2 * c.H)
    lp = lbuf[GUARD:GUARD + nl].view(B, T, c.C) if self.with_head else None
    self.C_.check(self.advance_raw(xw, sz, ah, y, lp, ws, T), "lr_rnn_bistream_advance")
    for buf, n in ((ybuf, ny), (lbuf, nl)):
      assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), "a guard word was written"
    return y, lp

  def read(self):
    c, B = self.case, self.B
    h = torch.full((c.layers, B, c.H), float("nan"), device=self.dev)
    cc = torch.full((c.layers, B, c.H), float("nan"), device=self.dev) if c.cell == "LSTM" else None
    meta = torch.full((2, B), -7, dtype=torch.int32, device=self.dev)
    self.C_.check(self.L.lr_rnn_bistream_read(self.state.data_ptr(), self.state.numel(), h.data_ptr(),
                                              self.C_.ptr(cc), meta[0].data_ptr(), meta[1].data_ptr(), B, c.H, c.layers,
                                              self.C_.stream_handle()), "lr_rnn_bistream_read")
    return h, cc, meta[0], meta[1]

  def slot_bytes(self, state, b):
    """every byte of `state` (a uint8 copy) that belongs to slot b: its header and its rows of h (and c), by the
    header's layout formulas"""
    c, B = self.case, self.B
    Hp = (c.H + 15) // 16 * 16
    a256 = lambda n: (n + 255) // 256 * 256   # noqa: E731
    parts = [state[32 * b:32 * b + 32]]
    for sec in range(2 if c.cell == "LSTM" else 1):
      base = a256(32 * B) + sec * a256(4 * c.layers * B * Hp)
      for l in range(c.layers):
        o = base + 4 * (l * B + b) * Hp
        parts.append(state[o:o + 4 * Hp])
    return torch.cat(parts)

  def run(self, x, plan, read_between=False):
    """The plan on this session: x (B, T, I) on the host.  Window rows past a slot's e_b are NaN.  Returns dict(y, lp by
    each slot's own frame index as lc_ref (lp rows nothing was consumed for stay 0: compare fed_rows), h, c, frames,
    state = a copy of the state's bytes, fed = frames consumed per slot, zero_row)."""
    c, B = self.case, self.B
    y = torch.zeros(B, c.T, 2 * c.H, device=self.dev)
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
      _, T, W, sizes, ahead = op
      xw = torch.full((B, W, c.I), float("nan"))
      for b in range(B):
        e = sizes[b] + ahead[b]
        xw[b, :e] = x[b, pos[b]:pos[b] + e]
      before = self.state.clone()
      yc, lc = self.feed(xw.to(self.dev), T, sizes, ahead)
      after = self.state.clone()
      for b, n in enumerate(sizes):
        y[b, pos[b]:pos[b] + n] = yc[b, :n]
        assert not yc[b, n:].any(), "y past a slot's frames is not zero"
        if lp is not None:
          lp[b, pos[b]:pos[b] + n] = lc[b, :n]
          if n < T:
            assert torch.equal(lc[b, n:], lc[b, n:n + 1].expand(T - n, -1)), "log_probs past a slot's frames"
            zero_row = lc[b, n].clone() if zero_row is None else zero_row
            assert torch.equal(zero_row, lc[b, n]), "log_probs past a slot's frames differ between slots"
        pos[b] += n
      for b, n in enumerate(sizes):   # idle and look-only slots keep every byte
        if n == 0:
          assert torch.equal(self.slot_bytes(before, b), self.slot_bytes(after, b)), "slot %d consumed nothing" % b
      if read_between:
        before = self.state.clone()
        self.read()
        assert torch.equal(before, self.state), "a read changed the state"
    h, cc, frames, status = self.read()
    assert not status.any(), status
    return dict(y=y, lp=lp, h=h, c=cc, frames=frames, state=self.state.clone(), fed=pos, zero_row=zero_row)
