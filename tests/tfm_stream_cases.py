"""Cases and CPU references of chunk-limited attention and the transformer sessions.

The rule: with chunk = C >= 1 and left_chunks = Lc >= 0, query q of a sample of len frames sits in chunk c = q // C and
attends to key k iff  max(0, c - Lc) * C <= k < min(len, (c + 1) * C).  C = 0: every key < len.

masked_ref   torch's own nn.TransformerEncoder under that rule.  The rule and the key padding are handed over as ONE
             additive mask per sample (B * heads, T, T): given separately, torch's src_key_padding_mask leaves a padded
             query whose chunk window holds no valid key with a row of -inf, i.e. NaN, and 0 x NaN then reaches the valid
             rows of the next layer.  Such a query (never one below len) attends to key 0 here; its row is not compared.
stream_ref   the same layers' weights applied chunk by chunk with an explicit key / value cache of the last Lc * C
             positions and a buffer of pending frames: what a session computes, in plain torch.
Both run in whatever dtype the reference module has (float64: the truth; float32: the CPU's own error).
"""
import torch
import torch.nn.functional as Fn

from oracle import torch_oracle as O

VOCAB = 64


def window(q, length, C, Lc):
  if C <= 0:
    return 0, length
  c = q // C
  return max(0, c - Lc) * C, min(length, (c + 1) * C)


def count_rule(n, ended, C):
  return n if ended else (n // C) * C


def make_ref(frame_dim, d_model, nhead, layers, ff, seed=0):
  torch.manual_seed(seed)
  ref = O.OracleTransformerEncoder(frame_dim, d_model, nhead, layers, ff, VOCAB, O.default_char2idx())
  with torch.no_grad():   # (LayerNorm parameters and biases off their initial 1 / 0, so that a slip there shows)
    for name, p in ref.named_parameters():
      if "norm" in name or name.endswith("bias"):
        p.add_(0.1 * torch.randn_like(p))
  return ref


def state_for_encoder(ref):
  return {k: v for k, v in ref.state_dict().items() if not k.startswith("encoder.")}


def additive_mask(T, lens, C, Lc, nhead, dtype):
  B = len(lens)
  m = torch.full((B, T, T), float("-inf"), dtype=dtype)
  for b in range(B):
    length = min(max(int(lens[b]), 1), T)
    for q in range(T):
      lo, hi = window(q, length, C, Lc)
      if hi > lo:
        m[b, q, lo:hi] = 0
      else:
        m[b, q, 0] = 0
  return m.repeat_interleave(nhead, dim=0)


def masked_ref(ref, x, lens, C, Lc):
  """x (B, T, I) in ref's dtype -> (log_probs (B, T, V + 1), hidden (B, T, Dm)), autograd intact."""
  B, T = x.shape[0], x.shape[1]
  nhead = ref.layers[0].self_attn.num_heads
  h = ref.input_proj(x) + ref.pe[:T]
  h = ref.encoder(h, mask=additive_mask(T, lens, C, Lc, nhead, x.dtype))
  logits = ref.output_proj(h)
  return O.masked_log_softmax(logits, ref.output_mask.expand_as(logits)), h


def _layer_rows(layer, h, kcache, vcache, nhead, scale_dh):
  """One encoder layer on the rows h (n, Dm) of ONE chunk, keys / values = cache + the chunk's own -> (h2, k, v)."""
  at = layer.self_attn
  Dm = h.shape[1]
  q, k, v = Fn.linear(h, at.in_proj_weight, at.in_proj_bias).split(Dm, dim=1)
  keys, vals = torch.cat((kcache, k)), torch.cat((vcache, v))
  dh = Dm // nhead
  ctx = []
  for hd in range(nhead):
    s = q[:, hd * dh:(hd + 1) * dh] @ keys[:, hd * dh:(hd + 1) * dh].T / scale_dh
    ctx.append(torch.softmax(s, dim=1) @ vals[:, hd * dh:(hd + 1) * dh])
  a = at.out_proj(torch.cat(ctx, dim=1))
  h1 = layer.norm1(h + a)
  h2 = layer.norm2(h1 + layer.linear2(torch.relu(layer.linear1(h1))))
  return h2, k, v


class StreamRef(object):
  """One slot of a session in plain torch: feed(frames (t, I), end) -> (log_probs rows, hidden rows) of the chunks the
  frames complete."""

  def __init__(self, ref, C, Lc):
    self.ref, self.C, self.Lc = ref, C, Lc
    p = ref.input_proj.weight
    self.Dm, self.nhead = p.shape[0], ref.layers[0].self_attn.num_heads
    self.pending = torch.zeros((0, p.shape[1]), dtype=p.dtype)
    self.k = [torch.zeros((0, self.Dm), dtype=p.dtype) for _ in ref.layers]
    self.v = [torch.zeros((0, self.Dm), dtype=p.dtype) for _ in ref.layers]
    self.n = self.emitted = 0
    self.ended = False

  def feed(self, frames, end=False):
    assert not self.ended or frames.shape[0] == 0
    ref, C = self.ref, self.C
    buf = torch.cat((self.pending, frames))
    self.n += frames.shape[0]
    self.ended = self.ended or bool(end)
    target = count_rule(self.n, self.ended, C)
    hs = []
    with torch.no_grad():
      while self.emitted < target:
        n = min(C, target - self.emitted)
        rows, buf = buf[:n], buf[n:]
        h = ref.input_proj(rows) + ref.pe[self.emitted:self.emitted + n]
        for l, layer in enumerate(ref.layers):
          h, k, v = _layer_rows(layer, h, self.k[l], self.v[l], self.nhead, (self.Dm // self.nhead) ** 0.5)
          keep = self.Lc * C
          self.k[l] = torch.cat((self.k[l], k))[-keep:] if keep else self.k[l]
          self.v[l] = torch.cat((self.v[l], v))[-keep:] if keep else self.v[l]
        hs.append(h)
        self.emitted += n
      self.pending = buf
      h = torch.cat(hs) if hs else torch.zeros((0, self.Dm), dtype=buf.dtype)
      logits = ref.output_proj(h)
      return O.masked_log_softmax(logits, ref.output_mask.expand_as(logits)), h


def stream_ref(ref, x, pieces, C, Lc):
  """x (n, I) fed in `pieces` (sizes summing to n; the last one ends the stream; [] with n = 0 is an empty flush) ->
  (log_probs (n, V + 1), hidden (n, Dm), counts per piece)."""
  st = StreamRef(ref, C, Lc)
  lps, hs, counts, t = [], [], [], 0
  pieces = list(pieces) or [0]
  for i, n in enumerate(pieces):
    lp, h = st.feed(x[t:t + n], end=i == len(pieces) - 1)
    t += n
    lps.append(lp)
    hs.append(h)
    counts.append(lp.shape[0])
  assert t == x.shape[0]
  return torch.cat(lps).detach(), torch.cat(hs).detach(), counts


def plans(n, C, seed=0):
  """Feeding plans of n frames: name -> piece sizes (each >= 0, summing to n)."""
  g = torch.Generator().manual_seed(1000 * n + 10 * C + seed)
  out = {"one": [n], "frames": [1] * n}
  ragged, left = [], n
  while left > 0:
    k = min(left, int(torch.randint(1, 2 * C + 3, (1,), generator=g)))
    ragged.append(k)
    left -= k
  out["ragged"] = ragged
  out["boundaries"] = [C] * (n // C) + ([n % C] if n % C else [])
  inside, left = [], n                      # every cut inside a chunk: C // 2 + 1, then whole-chunk strides from there
  first = min(n, C // 2 + 1)
  inside.append(first)
  left -= first
  while left > 0:
    k = min(left, C)
    inside.append(k)
    left -= k
  out["inside"] = inside
  several, left = [], n                     # several chunks per advance, and a tail
  while left > 0:
    k = min(left, 3 * C + 1)
    several.append(k)
    left -= k
  out["several"] = several
  for k, v in out.items():
    assert sum(v) == n and all(p >= 0 for p in v), (k, v)
  return out


def batch_plan(pieces_per_slot):
  """Per-slot piece lists -> advances [(sizes (B,), end (B,))]: advance i hands slot b its i-th piece, `end` with its
  last one; a slot that has run out is idle (size 0, no end)."""
  steps = max(len(p) for p in pieces_per_slot)
  out = []
  for i in range(steps):
    sizes = [p[i] if i < len(p) else 0 for p in pieces_per_slot]
    end = [1 if i == len(p) - 1 else 0 for p in pieces_per_slot]
    out.append((sizes, end))
  return out


# (d_model, heads): head dimension 16 (fp32 attention only) and 32 (the fused bf16 attention's)
MODELS = {"d64": (64, 4), "d128": (128, 4)}
FRAME_DIM, FF, LAYERS = 36, 96, 2
LENGTHS = (21, 96, 97)
CHUNKS = (1, 5, 8, 32)
LEFTS = (0, 1, 3)


def ragged_lens(T, C):
  """full, 1, 0, and a length that is not a multiple of C (nor 1 short of T when that is one)"""
  odd = T - 2 if (T - 2) % max(C, 2) else T - 3
  if C > 1 and odd % C == 0:
    odd -= 1
  return [T, 1, 0, max(odd, 2)]


# ---- the GPU harness: raw calls into lr_tfm_stream_* with traps around every buffer -------------------------------------

GUARD = 64   # floats either side of h_out / log_probs; 256 bytes either side of the state and the workspace


class Session(object):
  """B slots of `enc` (a TransformerVideoEncoder on the device) driven through the C ABI: every advance runs with
  NaN-filled outputs, a 0xFF-filled workspace, guard words either side of h_out, log_probs, the state and the workspace,
  and NaN in the rows of x no frame is fed for; rows at and past counts[b] are checked to be zeros / the head of the
  zero row."""

  def __init__(self, enc, B, dev):
    from lipreading_amd import _C
    self._C, self.L, self.enc, self.B, self.dev = _C, _C.lib(), enc, B, dev
    st = enc.stream(1, dev)   # (for its collected weights and configuration; its own state is not used)
    self.weights, self.head, self.pe, self.cfg = st._weights, st._head, st._pe, st._cfg
    self.I, self.Dm, self.nhead, self.F, self.layers, self.C, self.Lc = self.cfg
    self.Cv, self.eps = st.C, st.eps
    self.nstate = self.L.lr_tfm_stream_state_bytes(B, *self.cfg)
    assert self.nstate > 0 and self.nstate % B == 0
    self.raw = torch.full((self.nstate + 512,), 0xA5, dtype=torch.uint8, device=dev)
    self.state = self.raw[256:256 + self.nstate]
    self.fed = [0] * B
    self.reset()

  def _i32(self, v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=self.dev)

  def reset(self, mask=None):
    m = self._i32(mask)
    self._C.check(self.L.lr_tfm_stream_reset(self.state.data_ptr(), self.nstate, self._C.ptr(m), self.B, *self.cfg,
                                             self._C.stream_handle()), "reset")
    for b in range(self.B):
      if mask is None or mask[b]:
        self.fed[b] = 0
    self.check_guards()

  def check_guards(self):
    assert bool((self.raw[:256] == 0xA5).all()) and bool((self.raw[256 + self.nstate:] == 0xA5).all()), "state guards"

  def slot_bytes(self, b):
    n = self.nstate // self.B
    return self.state[b * n:(b + 1) * n].clone()

  def advance_raw(self, x_t, sizes_t, end_t, h_t, lp_t, counts_t, ws_t, **kw):
    """the call itself on tensors, any argument of the C call replaceable by name (pointers as integers): -> status"""
    from lipreading_amd.encoder import _ptr_array
    C_ = self._C
    T = x_t.shape[1] if x_t is not None else 0
    a = dict(x=C_.ptr(x_t) if T else None, sb=x_t.stride(0) if x_t is not None else 0,
             st=x_t.stride(1) if x_t is not None else 0, sizes=C_.ptr(sizes_t), end=C_.ptr(end_t),
             weights=_ptr_array(self.weights), pe=self.pe.data_ptr(), pe_rows=self.pe.shape[0], hw=C_.ptr(self.head[0]),
             hb=C_.ptr(self.head[1]), hm=C_.ptr(self.head[2]), h=C_.ptr(h_t), lp=C_.ptr(lp_t), counts=C_.ptr(counts_t),
             state=self.state.data_ptr(), state_bytes=self.nstate, ws=C_.ptr(ws_t),
             ws_bytes=ws_t.numel() if ws_t is not None else 0, B=self.B, T=T, I=self.I, Dm=self.Dm, nhead=self.nhead,
             F=self.F, layers=self.layers, Cv=self.Cv, C=self.C, Lc=self.Lc, eps=self.eps)
    a.update(kw)
    return self.L.lr_tfm_stream_advance(a["x"], a["sb"], a["st"], a["sizes"], a["end"], a["weights"], a["pe"], a["pe_rows"],
                                        a["hw"], a["hb"], a["hm"], a["h"], a["lp"], a["counts"], a["state"],
                                        a["state_bytes"], a["ws"], a["ws_bytes"], a["B"], a["T"], a["I"], a["Dm"],
                                        a["nhead"], a["F"], a["layers"], a["Cv"], a["C"], a["Lc"], a["eps"],
                                        C_.stream_handle())

  def workspace(self, T, B=None):
    n = self.L.lr_tfm_stream_workspace_bytes(B or self.B, T, self.I, self.Dm, self.nhead, self.F, self.layers, self.Cv,
                                             self.C, self.Lc)
    assert n > 0
    raw = torch.full((n + 512,), 0xFF, dtype=torch.uint8, device=self.dev)
    return raw, raw[256:256 + n]

  def feed(self, x, sizes, end=None, T=None):
    """x (B, Tall, I) on the CPU: slot b is fed its NEXT sizes[b] frames.  -> (h rows, lp rows, counts) per slot, the
    rows below counts[b] only, on the CPU."""
    B = self.B
    T = max(sizes) if T is None else T
    xc = torch.full((B, T, self.I), float("nan"))
    for b, n in enumerate(sizes):
      xc[b, :n] = x[b, self.fed[b]:self.fed[b] + n]
    rows = T + self.C - 1
    hraw = torch.full((B * rows * self.Dm + 2 * GUARD,), float("nan"), device=self.dev)
    lraw = torch.full((B * rows * self.Cv + 2 * GUARD,), float("nan"), device=self.dev)
    hraw[:GUARD] = hraw[-GUARD:] = lraw[:GUARD] = lraw[-GUARD:] = 12345.0
    h = hraw[GUARD:GUARD + B * rows * self.Dm].view(B, rows, self.Dm)
    lp = lraw[GUARD:GUARD + B * rows * self.Cv].view(B, rows, self.Cv)
    counts = torch.full((B,), -7, dtype=torch.int32, device=self.dev)
    wraw, ws = self.workspace(T)
    self._C.check(self.advance_raw(xc.to(self.dev) if T else None, self._i32(sizes), self._i32(end), h, lp, counts, ws),
                  "advance")
    torch.cuda.synchronize()
    self.check_guards()
    assert bool((wraw[:256] == 0xFF).all()) and bool((wraw[-256:] == 0xFF).all()), "workspace guards"
    for raw in (hraw, lraw):
      assert bool((raw[:GUARD] == 12345.0).all()) and bool((raw[-GUARD:] == 12345.0).all()), "output guards"
    cn = counts.cpu().tolist()
    h, lp = h.cpu(), lp.cpu()
    zero_row = None
    for b in range(B):
      assert 0 <= cn[b] <= rows
      assert not h[b, cn[b]:].any(), "rows past counts[b] are zeros"
      if cn[b] < rows:
        zero_row = lp[b, cn[b]] if zero_row is None else zero_row
        assert bool((lp[b, cn[b]:] == zero_row).all()) and torch.isfinite(zero_row).all(), "the head of the zero row"
      assert torch.isfinite(h[b, :cn[b]]).all() and torch.isfinite(lp[b, :cn[b]]).all()
      self.fed[b] += sizes[b]
    self.zero_row = zero_row
    return [h[b, :cn[b]] for b in range(B)], [lp[b, :cn[b]] for b in range(B)], cn

  def read(self):
    meta = torch.full((4, self.B), -9, dtype=torch.int32, device=self.dev)
    self._C.check(self.L.lr_tfm_stream_read(self.state.data_ptr(), self.nstate, meta[0].data_ptr(), meta[1].data_ptr(),
                                            meta[2].data_ptr(), meta[3].data_ptr(), self.B, *self.cfg,
                                            self._C.stream_handle()), "read")
    return [m.tolist() for m in meta.cpu()]

  def run(self, x, advances):
    """every advance of a batch plan -> dict(h, lp: per slot all emitted rows; counts: per advance; state: per slot
    bytes; frames / emitted / ended / status)"""
    B = self.B
    hs, lps, counts = [[] for _ in range(B)], [[] for _ in range(B)], []
    seen, ended = [0] * B, [False] * B
    for sizes, end in advances:
      h, lp, cn = self.feed(x, sizes, end)
      for b in range(B):
        before = count_rule(seen[b], ended[b], self.C)
        seen[b] += sizes[b]
        ended[b] = ended[b] or bool(end[b])
        assert cn[b] == count_rule(seen[b], ended[b], self.C) - before, "counts follow E"
        hs[b].append(h[b])
        lps[b].append(lp[b])
      counts.append(cn)
    frames, emitted, end_words, status = self.read()
    assert frames == seen and emitted == [count_rule(n, e, self.C) for n, e in zip(seen, ended)]
    assert end_words == [int(e) for e in ended]
    return dict(h=[torch.cat(v) for v in hs], lp=[torch.cat(v) for v in lps], counts=counts,
                state=[self.slot_bytes(b) for b in range(B)], frames=frames, status=status, zero_row=self.zero_row)
