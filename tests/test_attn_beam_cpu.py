"""CPU: a float64 restatement of the attention-decoder beam search (lipreading_amd/csrc/lr_attn_beam.hip, DESIGN.md
§14) on oracle.torch_oracle.OracleCharDecodingStep, checked against exhaustive enumeration, the greedy loop and a
hand-built case where the beam beats greedy; the ABI's and beam_search's rejections; the driver's new flags.
The GPU is checked against this restatement in tests/test_gpu_attn_beam.py."""
import itertools

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O

PAD, BOS, EOS, UNK = 0, 1, 2, 3


def _states(prev, rnn_type):
  """(h, c) or h, each (NL, B, Hd) -> per-utterance list of the same structure with B = 1."""
  if rnn_type == "LSTM":
    h, c = prev
    return [(h[:, b:b + 1], c[:, b:b + 1]) for b in range(h.shape[1])]
  return [prev[:, b:b + 1] for b in range(prev.shape[1])]


def _cat(states, rnn_type):
  if rnn_type == "LSTM":
    return (torch.cat([s[0] for s in states], 1), torch.cat([s[1] for s in states], 1))
  return torch.cat(states, 1)


def _pick(state, i, rnn_type):
  if rnn_type == "LSTM":
    return (state[0][:, i:i + 1], state[1][:, i:i + 1])
  return state[:, i:i + 1]


def beam_ref(dec, enc, enc_lens, prev, K, Lmax, bos=BOS, eos=EOS, pad=PAD, dtype=torch.float64):
  """The rule of lr_attn_beam.hip in float64: `dec` an OracleCharDecodingStep (converted to float64 here), enc
  (B, T, Hd), enc_lens (B,), prev the encoder's final state.  One oracle call per round over the live unfinished
  hypotheses of an utterance (`dtype` float32 only for timing).  Returns, per utterance, (beam, margin): beam = [(tokens, score)] best first; margin =
  the smallest of the gaps between the K-th and (K+1)-th entries of every round's sorted list (what decides the
  beam's membership) and between adjacent entries of the final beam (its order)."""
  dec = dec.to(dtype).eval()
  enc = enc.to(dtype)
  rnn_type = dec.rnn_type
  if isinstance(prev, tuple):
    prev = tuple(p.to(dtype) for p in prev)
  else:
    prev = prev.to(dtype)
  V = dec.vocab_size
  Kc = min(K, V - 2)
  out = []
  with torch.no_grad():
    for b, st0 in enumerate(_states(prev, rnn_type)):
      beam = [([], st0, 0.0)]
      margin = float("inf")
      for _ in range(Lmax + 1):
        fin = [len(h) == Lmax + 1 or (h and h[-1] == eos) for h, _, _ in beam]
        if all(fin):
          break
        live = [i for i, f in enumerate(fin) if not f]
        inp = torch.tensor([beam[i][0][-1] if beam[i][0] else bos for i in live])
        n = len(live)
        lp, new_state = dec(inp, _cat([beam[i][1] for i in live], rnn_type),
                            enc_lens[b:b + 1].expand(n), enc[b:b + 1].expand(n, -1, -1))
        lp = lp.numpy()
        lst = []
        for i, (h, s, sc) in enumerate(beam):
          if fin[i]:
            lst.append((h, s, sc))
            continue
          j = live.index(i)
          order = sorted((v for v in range(V) if v not in (pad, bos)), key=lambda v: (-lp[j, v], v))
          for v in order[:Kc]:
            lst.append((h + [v], _pick(new_state, j, rnn_type), sc + float(lp[j, v])))
        lst = sorted(lst, key=lambda e: -e[2])   # stable
        if len(lst) > K:
          margin = min(margin, lst[K - 1][2] - lst[K][2])
        beam = lst[:K]
      for x, y in zip(beam, beam[1:]):
        margin = min(margin, x[2] - y[2])
      out.append(([(h, sc) for h, _, sc in beam], margin))
  return out


def rescore(dec, enc, enc_lens, prev, b, tokens, bos=BOS):
  """float64 score of one token sequence of utterance b: the sum of its log-probabilities, fed BOS then itself."""
  dec = dec.double().eval()
  st = _states(tuple(p.double() for p in prev) if isinstance(prev, tuple) else prev.double(), dec.rnn_type)[b]
  s = 0.0
  x = bos
  with torch.no_grad():
    for v in tokens:
      lp, st = dec(torch.tensor([x]), st, enc_lens[b:b + 1], enc[b:b + 1].double())
      s += float(lp[0, v])
      x = v
  return s


def small_case(rnn_type, attn, V=5, Hd=8, T=6, B=2, layers=1, seed=0, eos_bias=0.0, scale=1.0):
  """A random OracleCharDecodingStep with its inputs: (dec, enc, enc_lens, prev)."""
  torch.manual_seed(seed)
  c2i = {"<PAD>": 0, "<BOS>": 1, "<EOS>": 2, "<UNK>": 3}
  for i in range(4, V):
    c2i["c%d" % i] = i
  dec = O.OracleCharDecodingStep(Hd, rnn_type, layers, 6, V, c2i, attention_type=attn,
                                 attn_hidden_size=5 if attn == "concat" else -1)
  with torch.no_grad():
    dec.output_proj.weight.mul_(scale)
    dec.output_proj.bias[EOS] += eos_bias
  enc = torch.randn(B, T, Hd)
  enc_lens = torch.tensor([T - (b % 3) for b in range(B)])
  h = torch.randn(layers, B, Hd) * 0.5
  prev = (h, torch.randn(layers, B, Hd) * 0.5) if rnn_type == "LSTM" else h
  return dec, enc, enc_lens, prev


def complete_hypotheses(V, Lmax):
  toks = [v for v in range(V) if v not in (PAD, BOS)]
  body = [v for v in toks if v != EOS]
  out = []
  for n in range(0, Lmax + 1):
    for pre in itertools.product(body, repeat=n):
      if n < Lmax + 1:
        out.append(list(pre) + [EOS])
  for pre in itertools.product(body, repeat=Lmax):
    for last in toks:
      if last != EOS:
        out.append(list(pre) + [last])
  return out


def test_enumeration_counts():
  assert len(complete_hypotheses(5, 2)) == 15
  assert len(complete_hypotheses(5, 3)) == 31


@pytest.mark.parametrize("rnn_type,attn,Lmax", [
    ("GRU", "none", 2), ("GRU", "dot", 3), ("GRU", "concat", 2), ("LSTM", "none", 3), ("LSTM", "dot", 2),
    ("LSTM", "concat", 3), ("RNN", "none", 2), ("RNN", "dot", 2), ("RNN", "concat", 3), ("GRU", "general", 2),
    ("LSTM", "1_layer_nn", 2)])
def test_restatement_equals_exhaustive_enumeration(rnn_type, attn, Lmax):
  """With K at least the number of complete hypotheses nothing is pruned: the beam is all of them, sorted."""
  dec, enc, lens, prev = small_case(rnn_type, attn, seed=3, scale=3.0)
  hyps = complete_hypotheses(5, Lmax)
  K = len(hyps)
  got = beam_ref(dec, enc, lens, prev, K, Lmax)
  for b in range(enc.shape[0]):
    want = sorted(((h, rescore(dec, enc, lens, prev, b, h)) for h in hyps), key=lambda e: -e[1])
    beam, _ = got[b]
    assert [h for h, _ in beam] == [h for h, _ in want]
    np.testing.assert_allclose([s for _, s in beam], [s for _, s in want], rtol=0, atol=1e-9)


@pytest.mark.parametrize("rnn_type,attn", [("GRU", "dot"), ("LSTM", "concat"), ("RNN", "general")])
def test_width_one_is_the_greedy_loop(rnn_type, attn):
  dec, enc, lens, prev = small_case(rnn_type, attn, V=12, T=7, B=3, seed=5, eos_bias=1.0, scale=2.0)
  Lmax = 6
  got = beam_ref(dec, enc, lens, prev, 1, Lmax)
  d = dec.double()
  for b in range(3):
    st = _states(tuple(p.double() for p in prev) if isinstance(prev, tuple) else prev.double(), dec.rnn_type)[b]
    x, toks, s = BOS, [], 0.0
    with torch.no_grad():
      while True:
        lp, st = d(torch.tensor([x]), st, lens[b:b + 1], enc[b:b + 1].double())
        lp = lp[0].numpy().copy()
        lp[[PAD, BOS]] = -np.inf
        x = int(np.argmax(lp))
        toks.append(x)
        s += float(lp[x])
        if x == EOS or len(toks) == Lmax + 1:
          break
    (beam, _), = got[b:b + 1]
    assert beam[0][0] == toks
    assert abs(beam[0][1] - s) < 1e-9


def greedy_trap():
  """A decoder where the greedy first character leads to the worse sequence.  V = 5 (PAD BOS EOS UNK 'a'), RNN,
  no attention, Hd = 4, char_dim = 5: the state is a code of the input token only (one-hot embedding, W_hh = 0),
  and output_proj reads per code:
    after BOS: P(a) = .5, P(UNK) = .4, P(EOS) = .1;   after a: EOS, UNK, a equally likely;
    after UNK: P(EOS) = .98.
  Greedy (K = 1) takes 'a' then EOS (ties go to the lower id): ~.5/3; K = 2 finds UNK EOS: ~.4 * .98."""
  c2i = {"<PAD>": 0, "<BOS>": 1, "<EOS>": 2, "<UNK>": 3, "a": 4}
  dec = O.OracleCharDecodingStep(4, "RNN", 1, 5, 5, c2i, attention_type="none")
  code = {BOS: 0, 4: 1, UNK: 2, EOS: 3}
  with torch.no_grad():
    for p in dec.parameters():
      p.zero_()
    dec.embedding.weight.copy_(torch.eye(5))
    dec.embedding.weight[PAD].zero_()
    for tok, j in code.items():
      dec.rnn.weight_ih_l0[j, tok] = 4.0
    w = dec.output_proj.weight
    w[4, 0], w[UNK, 0], w[EOS, 0] = np.log(.5), np.log(.4), np.log(.1)
    w[EOS, 2], w[UNK, 2], w[4, 2] = np.log(.98), np.log(.01), np.log(.01)
  B, T = 2, 3
  enc = torch.zeros(B, T, 4)
  lens = torch.tensor([T, 2])
  prev = torch.zeros(1, B, 4)
  return dec, enc, lens, prev


def test_beam_beats_greedy():
  dec, enc, lens, prev = greedy_trap()
  g = beam_ref(dec, enc, lens, prev, 1, 3)
  w = beam_ref(dec, enc, lens, prev, 2, 3)
  for b in range(2):
    assert g[b][0][0][0] == [4, EOS]
    assert w[b][0][0][0] == [UNK, EOS]
    assert w[b][0][0][1] > g[b][0][0][1] + 0.5


# ---- rejections, without a device ----------------------------------------------------------------------------------
def test_workspace_query_rejects_bad_sizes():
  from lipreading_amd import _C
  q = _C.lib().lr_decoder_beam_workspace_bytes
  ok = (1, 3, 1, 4, 10, 100, 75, 64, 32, 64, 0)   # LSTM, 1_layer_nn, 1 layer, B=4, K=10, Lmax=100, T=75, Hd=64
  assert q(*ok) > 0
  for i, bad in [(4, 0), (4, 33), (5, 0), (5, -1), (9, 1025), (9, 2), (3, 0), (2, 0), (2, 9), (7, 6), (0, 3),
                 (1, 5)]:
    args = list(ok)
    args[i] = bad
    assert q(*args) == 0, (i, bad)
  assert q(1, 3, 1, 4, 32, 100, 75, 64, 32, 1024, 0) > 0   # the limits themselves
  assert q(1, 4, 1, 4, 10, 100, 75, 64, 32, 64, 0) == 0     # concat without an attention size
  assert q(1, 4, 1, 4, 10, 100, 75, 64, 32, 64, 16) > 0
  assert q(1, 3, 8, 4, 10, 100, 75, 64, 32, 64, 0) > 0


def test_beam_search_entry_rejects_without_a_device():
  from lipreading_amd import _C
  L_ = _C.lib()

  def call(K=10, Lmax=100, V=64, params=None):
    return L_.lr_decoder_beam_search(1, 3, params, None, None, None, None, None, 1, 2, 0, K, Lmax, 1, None, None,
                                     None, None, None, 0, 4, 75, 64, 32, V, 0, None)
  assert call(K=0) == -1             # nonsense: invalid
  assert call(K=33) == -4            # well-formed, beyond the kernels: unsupported
  assert call(V=2000) == -4
  assert call(Lmax=0) == -1
  assert call() == -1                # NULL pointers


def test_beam_search_raises_for_cpu_tensors_and_bad_sizes():
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  enc = VideoEncoder(204, 16, rnn_type="GRU", bidirectional=False)
  dec = CharDecodingStep(enc, char_dim=8, vocab_size=64, char2idx=default_char2idx(), attention_type="dot")
  h = torch.zeros(2, 5, 16)
  lens = torch.tensor([5, 4])
  prev = torch.zeros(1, 2, 16)
  with pytest.raises(ValueError, match="GPU"):
    dec.beam_search(h, lens, prev)
  for kw in (dict(beam_width=0), dict(beam_width=33), dict(beam_width=2.0), dict(max_label_len=0),
             dict(max_label_len=-3), dict(poll_every=0)):
    with pytest.raises(ValueError):
      dec.beam_search(h, lens, prev, **kw)


# ---- driver ---------------------------------------------------------------------------------------------------------
def test_driver_attn_decode_flags_parse():
  from lipreading_amd import driver
  f = driver.parse_flags([])
  assert (f["attn_decode"], f["attn_beam_width"], f["attn_max_label_len"]) == ("teacher", 10, 100)
  f = driver.parse_flags(["--attn_decode=beam", "--attn_beam_width=4", "--attn_max_label_len=30"])
  assert (f["attn_decode"], f["attn_beam_width"], f["attn_max_label_len"]) == ("beam", 4, 30)
  for bad in ("--attn_decode=sample", "--attn_beam_width=0", "--attn_beam_width=33", "--attn_max_label_len=0"):
    with pytest.raises(SystemExit):
      driver.parse_flags([bad])


def test_driver_error_of_follows_attn_decode(monkeypatch):
  from lipreading_amd import driver, train
  calls = []
  monkeypatch.setattr(train, "eval", lambda *a, **k: (calls.append("eval"), (0.0, 3, 4, 0.0))[1])
  monkeypatch.setattr(train, "attention_cer", lambda *a, **k: (calls.append(("beam", k)), 0.25)[1])
  monkeypatch.setattr(train, "greedy_cer", lambda *a, **k: (calls.append("greedy"), 0.5)[1])
  dec = object()
  err = driver.make_error_of(driver.parse_flags([]), None, dec, None, "cpu", {})
  assert err([]) == pytest.approx(0.25) and calls == ["eval"]     # the default: teacher-forced mismatch rate
  calls.clear()
  err = driver.make_error_of(driver.parse_flags(["--attn_decode=beam", "--attn_beam_width=3"]), None, dec, None,
                             "cpu", {})
  assert err([]) == 0.25 and calls == [("beam", dict(beam_width=3, max_label_len=100))]
  calls.clear()
  err = driver.make_error_of(driver.parse_flags(["--attn_decode=beam"]), None, None, None, "cpu", {})
  assert err([]) == 0.5 and calls == ["greedy"]                  # no decoder: the CTC head's CER, as before
