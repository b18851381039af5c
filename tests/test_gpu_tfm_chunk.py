"""Chunk-limited self-attention on the GPU (lr_attn_*_chunked, lr_tfm_*_chunked) against torch's own
nn.TransformerEncoder under the same mask on the CPU (tests/tfm_stream_cases.masked_ref) and against the rule itself.

Bounds: the fp32 attention path at the figures tests/test_gpu_transformer.py holds it to without the mask (rtol 2e-4 /
atol 2e-5 forward, 3e-3 norm-wise on gradients), the fused bf16 path at 3e-2 norm-wise, the raw fused entry points at
test_fused_bf16_attention_matches_the_formula's 2e-2 of the largest entry / 1e-2 norm-wise.  None was tuned to a device
result."""
import numpy as np
import pytest
import torch

from tests import tfm_stream_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def make_pair(dev, model, C, Lc, attention, layers=S.LAYERS, seed=3):
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.transformer import TransformerVideoEncoder
  dm, nh = S.MODELS[model]
  ref = S.make_ref(S.FRAME_DIM, dm, nh, layers, S.FF, seed=seed)
  enc = TransformerVideoEncoder(S.FRAME_DIM, dm, nh, layers, S.FF, enable_ctc=True, vocab_size=S.VOCAB,
                                char2idx=default_char2idx(), attn_chunk=C, attn_left_chunks=Lc)
  res = enc.load_state_dict(S.state_for_encoder(ref))
  assert not res.missing_keys and not res.unexpected_keys
  enc.attention = attention
  return ref.train(), enc.to(dev).train()


def run_encoder(enc, dev, x, lens, wgt, valid):
  enc.zero_grad(set_to_none=True)
  xd = x.to(dev).requires_grad_(True)
  lp, h, _ = enc(xd, lens, max_len=x.shape[1])
  vd = valid.to(dev)
  ((lp * wgt.to(dev) * vd).sum() + (h * vd).pow(2).sum()).backward()
  return [lp.detach().cpu(), h.detach().cpu(), xd.grad.cpu()] + [p.grad.cpu().clone() for p in enc.parameters()]


def inputs(T, lens, seed):
  g = torch.Generator().manual_seed(seed)
  B = len(lens)
  x = torch.randn(B, T, S.FRAME_DIM, generator=g)
  wgt = torch.randn(B, T, S.VOCAB + 1, generator=g)
  lens_t = torch.tensor(lens)
  valid = (torch.arange(T).unsqueeze(0) < lens_t.unsqueeze(1)).float().unsqueeze(-1)   # (dh_out is zero on padded rows)
  return x, wgt, lens_t, valid


# every chunk and every left context once per attention path, the three lengths on the fp32 path (97 is past the fused
# kernel's 96 frames)
F32_CASES = [(21, 1, 0), (21, 5, 1), (21, 8, 3), (21, 32, 0), (96, 1, 3), (96, 5, 0), (96, 8, 1), (96, 32, 1),
             (97, 5, 3), (97, 8, 0), (97, 32, 3)]
BF16_CASES = [(21, 1, 0), (21, 5, 1), (21, 8, 3), (21, 32, 0), (96, 1, 3), (96, 5, 0), (96, 8, 1), (96, 32, 3)]


@pytest.mark.parametrize("attention,model,T,C,Lc", [("f32", "d64", *c) for c in F32_CASES] +
                         [("bf16", "d128", *c) for c in BF16_CASES])
def test_masked_stack_matches_torch(dev, attention, model, T, C, Lc):
  """Forward h / log_probs and every parameter gradient of a 2-layer stack under the chunk mask."""
  from lipreading_amd import _C
  ref, enc = make_pair(dev, model, C, Lc, attention)
  if attention == "bf16":   # (else the stack would quietly take the fp32 attention)
    assert _C.lib().lr_attn_fused_supported(T, enc.d_model // enc.nhead)
  lens = [n for n in S.ragged_lens(T, C) if n > 0] + [7]
  x, wgt, lens_t, valid = inputs(T, lens, seed=T + C + Lc)
  xr = x.clone().requires_grad_(True)
  lp_r, h_r = S.masked_ref(ref, xr, lens, C, Lc)
  ((lp_r * wgt * valid).sum() + (h_r * valid).pow(2).sum()).backward()
  got = run_encoder(enc, dev, x, lens_t, wgt, valid)
  m = valid.bool().squeeze(-1)
  want = dict(ref.named_parameters())
  grads = [("dx", got[2], xr.grad)] + [(k, g, (want[k] if k in want else want["encoder." + k]).grad)
                                       for (k, _), g in zip(enc.named_parameters(), got[3:])]
  for g in got:
    assert torch.isfinite(g).all()
  if attention == "f32":
    np.testing.assert_allclose(got[0][m].numpy(), lp_r.detach()[m].numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(got[1][m].numpy(), h_r.detach()[m].numpy(), rtol=2e-4, atol=2e-5)
    tol = 3e-3
  else:
    tol = 3e-2
    for a, b in ((got[0][m], lp_r.detach()[m]), (got[1][m], h_r.detach()[m])):
      assert float((a - b).norm()) <= tol * float(b.norm())
  for k, a, b in grads:
    err = float((a - b).norm()) / max(1e-6, float(b.norm()))
    assert err <= tol, (k, err)


def formula(qkv, dout, lens, nhead, C, Lc):
  """fp64 evaluation of the rule on the same fp32 inputs: (out, dqkv); a query without a key gives a zero row"""
  B, T, D3 = qkv.shape
  D, dh = D3 // 3, D3 // 3 // nhead
  r = qkv.double().requires_grad_(True)
  q, k, v = [t.reshape(B, T, nhead, dh).transpose(1, 2) for t in r.split(D, dim=-1)]
  s = q @ k.transpose(-1, -2) / dh ** 0.5
  allowed = torch.zeros(B, 1, T, T, dtype=torch.bool)
  for b in range(B):
    length = min(max(int(lens[b]), 1), T)
    for qi in range(T):
      lo, hi = S.window(qi, length, C, Lc)
      allowed[b, 0, qi, lo:hi] = True
  some = allowed.any(dim=-1, keepdim=True)
  p = torch.softmax(s.masked_fill(~(allowed | ~some), float("-inf")), dim=-1) * some
  want = (p @ v).transpose(1, 2).reshape(B, T, D)
  want.backward(dout.double())
  return want.detach(), r.grad, bool((~some).any())


def run_attention(dev, qkv, dout, lens, nhead, fused, C, Lc):
  from lipreading_amd.transformer import _AttentionFunction
  x = qkv.to(dev).requires_grad_(True)
  out = _AttentionFunction.apply(x, torch.tensor(lens, dtype=torch.int32, device=dev), nhead, fused, C, Lc)
  out.backward(dout.to(dev))
  return out.detach().cpu(), x.grad.cpu()


@pytest.mark.parametrize("fused,B,T,nhead,dh,lens,C,Lc", [
    # (all but the (32, 3) cases leave padded queries without any key: (5, 1) at len 50 of 96, (8, 0) at len 7 of 33 ...)
    (True, 3, 96, 2, 64, [96, 50, 1], 5, 1), (True, 5, 33, 4, 32, [33, 20, 7, 33, 2], 8, 0),
    (True, 4, 75, 4, 64, [75, 0, 40, 13], 32, 3), (True, 2, 21, 4, 32, [21, 9], 1, 3),
    (False, 3, 97, 2, 16, [97, 50, 1], 5, 1), (False, 4, 33, 4, 32, [33, 0, 7, 20], 8, 0),
    (False, 2, 130, 2, 16, [130, 71], 32, 3), (False, 2, 21, 4, 16, [21, 9], 1, 3)])
def test_chunked_attention_entry_points_match_the_formula(dev, fused, B, T, nhead, dh, lens, C, Lc):
  """lr_attn_fused_{forward,backward}_chunked, and lr_attn_softmax_forward_chunked between the batched products, against
  the rule in fp64.  Padded queries whose window is empty give a zero context row and take no part in any gradient."""
  g = torch.Generator().manual_seed(T + dh + C)
  qkv = torch.randn(B, T, 3 * nhead * dh, generator=g)
  dout = torch.randn(B, T, nhead * dh, generator=g)
  want, dwant, has_empty = formula(qkv, dout, lens, nhead, C, Lc)
  out, dx = run_attention(dev, qkv, dout, lens, nhead, fused, C, Lc)
  assert torch.isfinite(out).all() and torch.isfinite(dx).all()
  assert has_empty == ((C, Lc) != (32, 3))
  if has_empty:
    empty = want.abs().sum(dim=-1) == 0
    assert bool((out[empty] == 0).all())
  for a, b in ((out.double(), want), (dx.double(), dwant)):
    if fused:
      assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max())
      assert float((a - b).norm()) <= 1e-2 * float(b.norm())
    else:
      np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=2e-4, atol=2e-5)


def test_negative_chunks_are_refused_before_any_launch(dev):
  from lipreading_amd import _C
  L, st = _C.lib(), _C.stream_handle()
  B, T, nh, dh = 2, 8, 2, 32
  qkv = torch.randn(B, T, 3 * nh * dh, device=dev)
  probs = torch.full((B, nh, T, T), 7.0, device=dev)
  out = torch.full((B, T, nh * dh), 7.0, device=dev)
  lens = torch.full((B,), T, dtype=torch.int32, device=dev)
  for C, Lc in ((-1, 0), (4, -1)):
    assert L.lr_attn_softmax_forward_chunked(probs.data_ptr(), lens.data_ptr(), 1.0, B, nh, T, C, Lc, st) == _C.LR_ERR_INVALID_ARG
    assert L.lr_attn_fused_forward_chunked(qkv.data_ptr(), lens.data_ptr(), out.data_ptr(), 1.0, B, T, nh, dh, C, Lc,
                                           st) == _C.LR_ERR_INVALID_ARG
    assert L.lr_attn_fused_backward_chunked(qkv.data_ptr(), lens.data_ptr(), out.data_ptr(), out.data_ptr(), 1.0, B, T, nh,
                                            dh, C, Lc, st) == _C.LR_ERR_INVALID_ARG
  torch.cuda.synchronize()
  assert bool((probs == 7.0).all()) and bool((out == 7.0).all())


@pytest.mark.parametrize("attention,model,T", [("f32", "d64", 21), ("f32", "d64", 97), ("bf16", "d128", 21),
                                               ("bf16", "d128", 96)])
def test_a_chunk_that_covers_the_clip_is_full_attention_bit_for_bit(dev, attention, model, T):
  """chunk >= T gives the bits of chunk = 0, forward and backward; so does a left context that reaches frame 0:
  Lc >= T / C equals Lc = ceil(T / C)."""
  _, enc = make_pair(dev, model, 0, 0, attention)
  lens = [T, 1, T - 2, 7]
  x, wgt, lens_t, valid = inputs(T, lens, seed=T)
  base = run_encoder(enc, dev, x, lens_t, wgt, valid)
  for C, Lc in ((T, 0), (T + 5, 2), (1 << 30, 1 << 30)):
    enc.attn_chunk, enc.attn_left_chunks = C, Lc
    for a, b in zip(base, run_encoder(enc, dev, x, lens_t, wgt, valid)):
      assert torch.equal(a, b), (C, Lc)
  C = 5
  enc.attn_chunk, enc.attn_left_chunks = C, -(-T // C)
  reach = run_encoder(enc, dev, x, lens_t, wgt, valid)
  for Lc in (T // C, T // C + 1, 10 * T, 1 << 30):
    enc.attn_left_chunks = Lc
    for a, b in zip(reach, run_encoder(enc, dev, x, lens_t, wgt, valid)):
      assert torch.equal(a, b), Lc
  assert not torch.equal(reach[1], base[1])   # (chunks of 5 with every earlier chunk visible is still not full attention)


@pytest.mark.parametrize("attention,model,T,C,Lc", [("f32", "d64", 21, 5, 1), ("f32", "d64", 97, 8, 3),
                                                    ("f32", "d64", 97, 32, 0), ("bf16", "d128", 96, 8, 1),
                                                    ("bf16", "d128", 21, 1, 3), ("bf16", "d128", 96, 32, 1)])
def test_a_chunk_cannot_see_outside_its_window(dev, attention, model, T, C, Lc):
  """One layer: changing the frames at t >= (c + 1) C, or at t < (c - Lc) C, leaves chunk c's output bits unchanged —
  masked keys have probability exactly 0, so the change meets the chunk as 0 x finite.  (With two layers the left reach
  is 2 Lc chunks; the right reach stays the chunk's own end at any depth, which the second half checks on a 2-layer
  stack.)  On full attention every row moves."""
  _, enc = make_pair(dev, model, C, Lc, attention, layers=1)
  g = torch.Generator().manual_seed(T + C)
  x = torch.randn(1, T, S.FRAME_DIM, generator=g)
  lens = torch.tensor([T])
  c = (T // C) // 2
  lo, hi = max(0, c - Lc) * C, min(T, (c + 1) * C)
  x2 = x.clone()
  x2[:, hi:] = 3 * torch.randn(1, T - hi, S.FRAME_DIM, generator=g)
  x2[:, :lo] = 3 * torch.randn(1, lo, S.FRAME_DIM, generator=g)
  assert lo > 0 or hi < T
  with torch.no_grad():
    a = enc(x.to(dev), lens, max_len=T)
    b = enc(x2.to(dev), lens, max_len=T)
    for u, v in zip(a[:2], b[:2]):
      assert torch.equal(u[:, c * C:hi], v[:, c * C:hi])
      assert not torch.equal(u, v)
    enc.attn_chunk = 0
    a, b = enc(x.to(dev), lens, max_len=T), enc(x2.to(dev), lens, max_len=T)
    assert not torch.equal(a[1][:, c * C:hi], b[1][:, c * C:hi])
  _, deep = make_pair(dev, model, C, Lc, attention, layers=2)
  x3 = x.clone()
  x3[:, hi:] = 3 * torch.randn(1, T - hi, S.FRAME_DIM, generator=g)
  if hi < T:
    with torch.no_grad():
      a, b = deep(x.to(dev), lens, max_len=T), deep(x3.to(dev), lens, max_len=T)
    assert torch.equal(a[1][:, :hi], b[1][:, :hi]) and not torch.equal(a[1], b[1])


@pytest.mark.parametrize("attention,model,T,C,Lc", [("f32", "d64", 21, 5, 1), ("f32", "d64", 97, 32, 1),
                                                    ("bf16", "d128", 96, 8, 3)])
def test_a_padded_batch_equals_each_sample_alone(dev, attention, model, T, C, Lc):
  """Rows < len of a sample depend on that sample's frames < len only: (a) what the padding holds changes no bit of
  them nor of any gradient; (b) the sample run alone, unpadded, agrees at the path's forward bound (another row count:
  other split-K and tile edges, so not the bits)."""
  ref, enc = make_pair(dev, model, C, Lc, attention)
  lens = [n for n in S.ragged_lens(T, C) if n > 0] + [7]
  x, wgt, lens_t, valid = inputs(T, lens, seed=3 * T)
  m = valid.bool().squeeze(-1)
  x2 = x.clone()
  x2[~m] = 1e4 * torch.sign(torch.randn(int((~m).sum()), S.FRAME_DIM, generator=torch.Generator().manual_seed(1)))
  a, b = run_encoder(enc, dev, x, lens_t, wgt, valid), run_encoder(enc, dev, x2, lens_t, wgt, valid)
  for i, (u, v) in enumerate(zip(a, b)):
    if i < 3:
      u, v = u[m], v[m]
    assert torch.isfinite(v).all() and torch.equal(u, v), i
  with torch.no_grad():
    for bi, n in enumerate(lens):
      lp1, h1, _ = enc(x[bi:bi + 1, :n].to(dev), torch.tensor([n]), max_len=n)
      for u, v in ((lp1[0].cpu(), a[0][bi, :n]), (h1[0].cpu(), a[1][bi, :n])):
        if attention == "f32":
          np.testing.assert_allclose(u.numpy(), v.numpy(), rtol=2e-4, atol=2e-5)
        else:
          assert float((u - v).norm()) <= 3e-2 * float(v.norm())


@pytest.mark.parametrize("attention,model,T,C,Lc", [("f32", "d64", 21, 5, 0), ("f32", "d64", 97, 8, 1),
                                                    ("bf16", "d128", 96, 5, 0), ("bf16", "d128", 21, 32, 3)])
def test_a_length_zero_sample_and_padded_queries_stay_finite(dev, attention, model, T, C, Lc):
  """A sample of length 0 (clamped to 1, as without the mask) and the padded queries whose window holds no key at all:
  every output and every gradient is finite, and the other samples' rows are what they are without that sample."""
  _, enc = make_pair(dev, model, C, Lc, attention)
  lens = [T, 0, 3, 1]
  x, wgt, lens_t, valid = inputs(T, lens, seed=T)
  got = run_encoder(enc, dev, x, lens_t, wgt, torch.ones_like(valid))   # (gradient through the padded rows as well)
  for g in got:
    assert torch.isfinite(g).all()
  keep = [0, 2, 3]
  alone = run_encoder(enc, dev, x[keep], lens_t[keep], wgt[keep], torch.ones_like(valid[keep]))
  m = valid[keep].bool().squeeze(-1)
  u, v = got[1][keep][m], alone[1][m]   # (another row count: not the bits)
  if attention == "f32":
    np.testing.assert_allclose(u.numpy(), v.numpy(), rtol=2e-4, atol=2e-5)
  else:
    assert float((u - v).norm()) <= 3e-2 * float(v.norm())
