"""CPU: a float64 restatement of the joint CTC/attention beam search (lr_decoder_joint_beam_search,
lipreading_amd/csrc/lr_attn_beam.hip), checked against brute-force CTC sums, the attention-only
restatement of tests/test_attn_beam_cpu.py at weight 0, exhaustive enumeration and a hand-built case where the CTC
frames correct the attention decoder; the ABI's and beam_search's rejections; the driver's new flags.
The GPU is checked against this restatement in tests/test_gpu_joint_beam.py."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import (BOS, EOS, PAD, UNK, _cat, _pick, _states, beam_ref, complete_hypotheses,
                                      greedy_trap, rescore, small_case)

NEG = -math.inf


def lae(x, y):
  """log(e^x + e^y); -inf only when both are."""
  m, d = max(x, y), min(x, y)
  return m if m == NEG else m + math.log1p(math.exp(d - m))


def empty_prefix(yb, Tb):
  """(gamma^n, gamma^b) of the empty prefix over t < Tb."""
  return np.full(Tb, NEG), np.cumsum(yb[:Tb, 0])


def extend(gn_g, gb_g, last, k, yb, Tb):
  """The rule's extension h = g + (class k): returns (gamma^n(h), gamma^b(h), log psi(h), log P(labelling = h)).
  `last` is last(g)'s class, None for the empty prefix."""
  gn = gb = psi = NEG
  phi = 0.0 if last is None else NEG
  out_n, out_b = np.empty(Tb), np.empty(Tb)
  for t in range(Tb):
    yk, y0 = float(yb[t, k]), float(yb[t, 0])
    psi = lae(psi, phi + yk)
    gn, gb = lae(gn, phi) + yk, lae(gb, gn) + y0
    out_n[t], out_b[t] = gn, gb
    phi = gb_g[t] if k == last else lae(gb_g[t], gn_g[t])
  return out_n, out_b, psi, lae(gn, gb)


def ctc_score(tokens, yb, Tb, eos=EOS):
  """The rule's CTC score of a complete or capped hypothesis (decoder token ids): the full-sequence log-probability
  when it ends with EOS, the prefix log-probability otherwise."""
  gn, gb = empty_prefix(yb, Tb)
  last, c = None, 0.0
  for v in tokens:
    gn, gb, psi, full = extend(gn, gb, last, v + 1, yb, Tb)
    last = v + 1
    c = full if v == eos else psi
  return c


def joint_score(a, c, lam):
  return c if lam == 1.0 else (1.0 - lam) * a + lam * c


def joint_ref(dec, enc, enc_lens, prev, y, K, Lmax, lam, P=None, bos=BOS, eos=EOS, pad=PAD):
  """The joint rule in float64.  y (B, T, V+1) CTC log-probs.  Returns, per utterance, (beam, margin):
  beam = [(tokens, s, a, c)] best first; margin as in beam_ref, on the joint score s."""
  dec = dec.double().eval()
  enc = enc.double()
  rnn_type = dec.rnn_type
  prev = tuple(p.double() for p in prev) if isinstance(prev, tuple) else prev.double()
  y = np.asarray(y, dtype=np.float64)
  V = dec.vocab_size
  if P is None:
    P = min(V - 2, -(-3 * K // 2))
  ctc = lam > 0
  out = []
  with torch.no_grad():
    for b, st0 in enumerate(_states(prev, rnn_type)):
      Tb = int(enc_lens[b])
      yb = y[b]
      gn0, gb0 = empty_prefix(yb, Tb)
      beam = [dict(h=[], st=st0, a=0.0, c=0.0, s=0.0, gn=gn0, gb=gb0)]
      margin = math.inf
      for _ in range(Lmax + 1):
        fin = [len(e["h"]) == Lmax + 1 or (e["h"] and e["h"][-1] == eos) for e in beam]
        if all(fin):
          break
        live = [i for i, f in enumerate(fin) if not f]
        inp = torch.tensor([beam[i]["h"][-1] if beam[i]["h"] else bos for i in live])
        n = len(live)
        lp, new_state = dec(inp, _cat([beam[i]["st"] for i in live], rnn_type), enc_lens[b:b + 1].expand(n),
                            enc[b:b + 1].expand(n, -1, -1))
        lp = lp.numpy()
        lst = []
        for i, e in enumerate(beam):
          if fin[i]:
            lst.append(e)
            continue
          j = live.index(i)
          order = sorted((v for v in range(V) if v not in (pad, bos)), key=lambda v: (-lp[j, v], v))
          last = e["h"][-1] + 1 if e["h"] else None
          for v in order[:P]:
            a = e["a"] + float(lp[j, v])
            c, gn, gb = 0.0, None, None
            if ctc:
              gn, gb, psi, full = extend(e["gn"], e["gb"], last, v + 1, yb, Tb)
              c = full if v == eos else psi
              if c == NEG:
                continue   # a structural zero
            s = joint_score(a, c, lam) if ctc else a
            lst.append(dict(h=e["h"] + [v], st=_pick(new_state, j, rnn_type), a=a, c=c, s=s, gn=gn, gb=gb))
        lst = sorted(lst, key=lambda x: -x["s"])   # stable
        if len(lst) > K:
          margin = min(margin, lst[K - 1]["s"] - lst[K]["s"])
        beam = lst[:K]
        if not beam:
          break
      for x, z in zip(beam, beam[1:]):
        margin = min(margin, x["s"] - z["s"])
      out.append(([(e["h"], e["s"], e["a"], e["c"]) for e in beam], margin))
  return out


def random_frames(B, T, C, seed, peak=3.0, f32=True):
  """Model-like CTC log-probs (B, T, C), float32 values held in float64 (f32=False: exactly normalised float64,
  as the brute-force sums need: they multiply out the frames past the prefix, which the rule takes to sum to 1)."""
  rng = np.random.default_rng(seed)
  x = rng.standard_normal((B, T, C))
  x[np.arange(B)[:, None], np.arange(T)[None, :], rng.integers(0, C, (B, T))] += peak
  x = x - np.log(np.exp(x).sum(2, keepdims=True))
  return x.astype(np.float32).astype(np.float64) if f32 else x


# ---- the CTC terms against brute force ------------------------------------------------------------------------------
def collapse(path):
  out, prev = [], None
  for c in path:
    if c != 0 and c != prev:
      out.append(c)
    prev = c
  return out


def brute(yb, Tb, h):
  """(log sum over alignments whose labelling starts with h, log sum over those whose labelling is h)."""
  C = yb.shape[1]
  pre = full = 0.0
  for path in itertools.product(range(C), repeat=Tb):
    lab = collapse(path)
    if lab[:len(h)] == h:
      p = math.exp(sum(float(yb[t, c]) for t, c in enumerate(path)))
      pre += p
      if lab == h:
        full += p
  return (math.log(pre) if pre > 0 else NEG), (math.log(full) if full > 0 else NEG)


@pytest.mark.parametrize("C,T,Tb,seed", [(3, 5, 5, 0), (4, 6, 4, 1), (5, 6, 6, 2), (5, 5, 3, 3), (4, 6, 6, 4)])
def test_prefix_and_full_scores_equal_brute_force(C, T, Tb, seed):
  """T_b < T, repeated labels and structural zeros included (labels up to 4 long over T_b <= 6 frames)."""
  yb = random_frames(1, T, C, seed, peak=1.0, f32=False)[0]
  zeros = 0
  for n in range(1, 5):
    for h in itertools.product(range(1, C), repeat=n):
      h = list(h)
      gn, gb = empty_prefix(yb, Tb)
      last, psi, full = None, 0.0, 0.0
      for k in h:
        gn, gb, psi, full = extend(gn, gb, last, k, yb, Tb)
        last = k
      want_pre, want_full = brute(yb, Tb, h)
      need = len(h) + sum(1 for x, z in zip(h, h[1:]) if x == z)   # frames a labelling needs
      if need > Tb:
        zeros += 1
        assert psi == NEG and full == NEG and want_pre == NEG, h
        continue
      assert abs(psi - want_pre) < 1e-9, (h, psi, want_pre)
      assert abs(full - want_full) < 1e-9, (h, full, want_full)
  assert zeros > 0 or Tb >= 6


def test_repeated_label_needs_a_blank():
  """With last(g) = k the path must pass a blank: two frames cannot spell 'k k', three spell it one way."""
  yb = random_frames(1, 4, 3, 9, f32=False)[0]
  gn, gb = empty_prefix(yb, 2)
  gn, gb, _, _ = extend(gn, gb, None, 1, yb, 2)
  _, _, psi, full = extend(gn, gb, 1, 1, yb, 2)
  assert psi == NEG and full == NEG
  gn, gb = empty_prefix(yb, 3)
  gn, gb, _, _ = extend(gn, gb, None, 1, yb, 3)
  _, _, psi, full = extend(gn, gb, 1, 1, yb, 3)
  assert math.isclose(psi, float(yb[0, 1] + yb[1, 0] + yb[2, 1]), abs_tol=1e-12) and psi == full


# ---- the restatement -------------------------------------------------------------------------------------------------
CASES = [(rt, at) for rt in ("GRU", "LSTM", "RNN") for at in ("none", "dot", "general", "1_layer_nn", "concat")]


@pytest.mark.parametrize("rnn_type,attn", CASES)
def test_weight_zero_is_the_attention_search(rnn_type, attn):
  dec, enc, lens, prev = small_case(rnn_type, attn, V=8, T=6, B=3, seed=21, scale=2.0, eos_bias=0.5)
  y = random_frames(3, 6, 9, 5)
  for K, P in ((1, 1), (1, 6), (3, 5)):
    want = beam_ref(dec, enc, lens, prev, K, 4)
    got = joint_ref(dec, enc, lens, prev, y, K, 4, 0.0, P=P)
    for (wb, _), (gb, _) in zip(want, got):
      assert [h for h, _ in wb] == [h for h, *_ in gb]
      assert [s for _, s in wb] == [s for _, s, _, _ in gb]


@pytest.mark.parametrize("rnn_type,attn,Lmax,lam", [
    ("GRU", "dot", 2, 0.3), ("LSTM", "concat", 3, 0.5), ("RNN", "none", 2, 1.0), ("GRU", "general", 3, 0.7),
    ("LSTM", "1_layer_nn", 2, 0.3), ("RNN", "dot", 3, 0.5)])
def test_exhaustive_search(rnn_type, attn, Lmax, lam):
  """K at least the number of complete hypotheses and P = V - 2: the beam is every complete hypothesis the frames
  allow (the others are structural zeros), scored by the rule and sorted."""
  dec, enc, lens, prev = small_case(rnn_type, attn, V=5, T=6, B=3, seed=3, scale=3.0)
  lens = torch.tensor([6, 4, 3])
  y = random_frames(3, 6, 6, 11, peak=1.0)
  hyps = complete_hypotheses(5, Lmax)
  K = len(hyps)
  got = joint_ref(dec, enc, lens, prev, y, K, Lmax, lam, P=3)
  dropped = 0
  for b in range(3):
    Tb = int(lens[b])
    want = []
    for h in hyps:
      c = ctc_score(h, y[b], Tb)
      if c == NEG:
        dropped += 1
        continue
      want.append((h, joint_score(rescore(dec, enc, lens, prev, b, h), c, lam)))
    want.sort(key=lambda e: -e[1])
    beam, _ = got[b]
    assert [h for h, *_ in beam] == [h for h, _ in want], b
    np.testing.assert_allclose([s for _, s, _, _ in beam], [s for _, s in want], rtol=0, atol=1e-9)
  assert dropped > 0


def ctc_trap():
  """greedy_trap's decoder (at K = 2 attention alone picks UNK EOS) with CTC frames that spell 'a' EOS:
  utterance 0 (T_b = 3) as a, blank, EOS; utterance 1 (T_b = 2) as a, EOS.  Each frame puts 0.9 on its class."""
  dec, enc, lens, prev = greedy_trap()
  C = 6
  spell = [[4 + 1, 0, EOS + 1], [4 + 1, EOS + 1, 0]]
  y = np.full((2, 3, C), math.log(0.1 / (C - 1)))
  for b, row in enumerate(spell):
    for t, k in enumerate(row):
      y[b, t, k] = math.log(0.9)
  return dec, enc, lens, prev, y.astype(np.float32)


def test_ctc_corrects_the_attention_decoder():
  dec, enc, lens, prev, y = ctc_trap()
  att = joint_ref(dec, enc, lens, prev, y, 2, 3, 0.0)
  for b in range(2):
    assert att[b][0][0][0] == [UNK, EOS]
  for lam in (0.5, 0.9):
    got = joint_ref(dec, enc, lens, prev, y, 2, 3, lam)
    for b in range(2):
      assert got[b][0][0][0] == [4, EOS], (lam, got[b])


def test_short_utterance_drops_structural_zeros():
  """T_b = 1: only one label fits, so every surviving hypothesis is a single token (EOS) or capped at one label."""
  dec, enc, lens, prev = small_case("GRU", "dot", V=6, T=5, B=2, seed=8, scale=2.0)
  lens = torch.tensor([1, 5])
  y = random_frames(2, 5, 7, 4)
  got = joint_ref(dec, enc, lens, prev, y, 4, 3, 0.5)
  beam, _ = got[0]
  assert beam and all(len(h) == 1 and h == [EOS] for h, *_ in beam)   # 'x EOS' needs two frames
  assert all(np.isfinite(s) for _, s, _, _ in beam)


# ---- rejections, without a device ----------------------------------------------------------------------------------
OK = (1, 3, 1, 4, 10, 100, 75, 64, 32, 64, 0, 65, 15)   # the beam query's arguments, then C = V + 1, P = 15


def test_joint_workspace_query_rejects_bad_sizes():
  from lipreading_amd import _C
  q = _C.lib().lr_decoder_joint_beam_workspace_bytes
  assert q(*OK) > _C.lib().lr_decoder_beam_workspace_bytes(*OK[:11])
  for i, bad in [(4, 0), (4, 33), (9, 1025), (11, 64), (11, 66), (12, 9), (12, 63), (6, 65536), (5, 0), (3, 0)]:
    args = list(OK)
    args[i] = bad
    assert q(*args) == 0, (i, bad)
  assert q(*OK[:12], 10) > 0 and q(*OK[:12], 62) > 0               # P = K and P = V - 2
  assert q(1, 3, 1, 4, 10, 100, 75, 64, 32, 8, 0, 9, 6) > 0        # V = 8: P in [6, 6]
  assert q(1, 3, 1, 4, 10, 100, 75, 64, 32, 8, 0, 9, 7) == 0
  assert q(1, 3, 1, 4, 32, 100, 75, 64, 32, 128, 0, 129, 64) > 0   # the limits
  assert q(1, 3, 1, 4, 32, 100, 75, 64, 32, 128, 0, 129, 65) == 0


def test_joint_entry_rejects_without_a_device():
  from lipreading_amd import _C
  L_ = _C.lib()

  def call(K=10, V=64, C=65, blank=0, lam=0.3, P=15, T=75):
    return L_.lr_decoder_joint_beam_search(1, 3, None, None, None, None, None, None, None, 75 * C, C, C, blank, lam,
                                           P, 1, 2, 0, K, 100, 1, None, None, None, None, None, 0, 4, T, 64, 32, V,
                                           0, None)
  assert call(C=64) == -1 and call(C=66) == -1
  assert call(blank=1) == -1
  assert call(lam=-0.1) == -1 and call(lam=1.5) == -1 and call(lam=float("nan")) == -1
  assert call(P=9) == -4 and call(P=63) == -4
  assert call(T=70000) == -4
  assert call(K=33) == -4 and call(K=0) == -1
  assert call() == -1   # NULL pointers


def test_beam_search_joint_raises_for_bad_inputs():
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  enc = VideoEncoder(204, 16, rnn_type="GRU", bidirectional=False)
  dec = CharDecodingStep(enc, char_dim=8, vocab_size=64, char2idx=default_char2idx(), attention_type="dot")
  h = torch.zeros(2, 5, 16)
  lens = torch.tensor([5, 4])
  prev = torch.zeros(1, 2, 16)
  for kw in (dict(ctc_log_probs=torch.zeros(2, 5, 65), ctc_weight=0.3), dict(ctc_log_probs=torch.zeros(2, 5, 64)),
             dict(ctc_log_probs=torch.zeros(2, 5, 65), ctc_weight=2.0)):
    with pytest.raises(ValueError, match="GPU"):
      dec.beam_search(h, lens, prev, **kw)


def test_joint_argument_checks():
  """beam_search's checks of the joint arguments, driven with a stand-in for device tensors."""
  from lipreading_amd.attention_decoder import _joint_args

  class Dev:
    """A tensor-like that claims to live on the device (the checks read shape, dtype, strides, device)."""
    def __init__(self, t, dev="cuda:0", strides=None):
      self.t, self.device, self._s = t, dev, strides
      self.is_cuda, self.dtype, self.shape = True, t.dtype, t.shape

    def dim(self):
      return self.t.dim()

    def stride(self, i=None):
      s = self._s or self.t.stride()
      return s if i is None else s[i]

  import lipreading_amd.attention_decoder as AD
  real = AD.torch.is_tensor
  AD.torch.is_tensor = lambda x: isinstance(x, Dev) or real(x)
  try:
    h = Dev(torch.zeros(2, 5, 16))
    lens = torch.tensor([5, 4])
    y = Dev(torch.zeros(2, 5, 65))
    assert _joint_args(y, 0.3, None, 10, 64, h, lens) == (0.3, 15)
    assert _joint_args(y, 0, 10, 10, 64, h, lens) == (0.0, 10)
    assert _joint_args(y, 1.0, 62, 10, 64, h, lens) == (1.0, 62)
    bad = [(Dev(torch.zeros(2, 5, 64)), 0.3, None, lens), (Dev(torch.zeros(2, 4, 65)), 0.3, None, lens),
           (Dev(torch.zeros(3, 5, 65)), 0.3, None, lens), (Dev(torch.zeros(2, 5, 65, dtype=torch.float64)), 0.3,
                                                           None, lens),
           (Dev(torch.zeros(2, 5, 65), strides=(325, 65, 2)), 0.3, None, lens),
           (Dev(torch.zeros(2, 5, 65), dev="cuda:1"), 0.3, None, lens),
           (y, -0.1, None, lens), (y, 1.5, None, lens), (y, float("nan"), None, lens), (y, True, None, lens),
           (y, 0.3, 9, lens), (y, 0.3, 63, lens), (y, 0.3, 15.0, lens),
           (y, 0.3, None, torch.tensor([5, 0])), (y, 0.3, None, torch.tensor([6, 4]))]
    for yy, lam, P, ll in bad:
      with pytest.raises(ValueError):
        _joint_args(yy, lam, P, 10, 64, h, ll)
  finally:
    AD.torch.is_tensor = real


# ---- driver ---------------------------------------------------------------------------------------------------------
def test_driver_joint_flags_parse():
  from lipreading_amd import driver
  f = driver.parse_flags([])
  assert f["attn_ctc_weight"] == pytest.approx(0.3) and f["attn_decode"] == "teacher"
  f = driver.parse_flags(["--attn_decode=joint", "--enable_ctc=True", "--attn_ctc_weight=0.5"])
  assert (f["attn_decode"], f["attn_ctc_weight"]) == ("joint", 0.5)
  for bad in (["--attn_decode=joint"], ["--attn_decode=joint", "--enable_ctc=False"],
              ["--attn_decode=joint", "--enable_ctc=True", "--attn_ctc_weight=1.5"],
              ["--attn_decode=joint", "--enable_ctc=True", "--attn_ctc_weight=-0.1"]):
    with pytest.raises(SystemExit):
      driver.parse_flags(bad)


def test_driver_error_of_routes_joint(monkeypatch):
  from lipreading_amd import driver, train
  calls = []
  monkeypatch.setattr(train, "attention_cer", lambda *a, **k: (calls.append(k), 0.25)[1])
  f = driver.parse_flags(["--attn_decode=joint", "--enable_ctc=True", "--attn_ctc_weight=0.4",
                          "--attn_beam_width=3"])
  err = driver.make_error_of(f, None, object(), None, "cpu", {})
  assert err([]) == 0.25 and calls == [dict(beam_width=3, max_label_len=100, ctc_weight=0.4)]


def test_joint_needs_the_ctc_head():
  from lipreading_amd import analysis, train
  from lipreading_amd.encoder import VideoEncoder
  enc = VideoEncoder(204, 16, rnn_type="GRU", bidirectional=False)
  with pytest.raises(ValueError, match="enable_ctc"):
    train.attention_cer(enc, None, [], "cpu", {"<EOS>": 2}, ctc_weight=0.3)
  with pytest.raises(ValueError, match="enable_ctc"):
    analysis.inference(enc, None, None, None, None, None, "cpu", {}, ctc_weight=0.3)
