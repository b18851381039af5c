"""GPU: CharDecodingStep.beam_search (lr_decoder_beam_search) against the float64 restatement of
tests/test_attn_beam_cpu.py, with one set of random weights loaded into both CharDecodingStep and
OracleCharDecodingStep.

Tolerance.  The device computes in float32 and the restatement in float64.  Where every round of the restatement
has a margin above 1e-3 (between the K-th and (K+1)-th entries of the sorted list, and between adjacent entries of the
final beam), float32 rounding cannot change which hypotheses are kept or their order: the token sequences must then
be identical, and each score within 1e-4 + 1e-6 per token — the float32 error of a sum of up to Lmax + 1
log-probabilities, each from an Hd-long dot product.  An utterance with a smaller margin (a near-tie) may
legitimately keep a different but equally good hypothesis; there the GPU's hypotheses are re-scored in float64 and
that score list must match the restatement's within the same tolerance.  Random weights put many candidates within
1e-3 of the cut at K = 10 (40-72 % of a case's utterances here; 0-25 % at K = 1 and 5), so each case allows up to
75 % near-tie utterances; those are still held to the score list.
"""
import numpy as np
import pytest
import torch

from tests.test_attn_beam_cpu import beam_ref, greedy_trap, small_case, _states, BOS, EOS, PAD

pytestmark = pytest.mark.gpu
NEAR = 1e-3


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def hip_from_oracle(odec, dev):
  """A CharDecodingStep holding the oracle's weights."""
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.encoder import VideoEncoder
  Hd = odec.hidden_size
  enc = VideoEncoder(204, Hd, rnn_type=odec.rnn_type, num_layers=odec.num_layers, bidirectional=False)
  c2i = {"<PAD>": 0, "<BOS>": 1, "<EOS>": 2, "<UNK>": 3}
  for i in range(4, odec.vocab_size):
    c2i["c%d" % i] = i
  ah = odec.attn_proj_layer1.out_features if odec.attention_type == "concat" else -1
  dec = CharDecodingStep(enc, char_dim=odec.char_dim, vocab_size=odec.vocab_size, char2idx=c2i,
                         attention_type=odec.attention_type, attn_hidden_size=ah)
  r = dec.load_state_dict({k: v.float() for k, v in odec.state_dict().items()})
  assert not (r.missing_keys or r.unexpected_keys)
  return dec.to(dev).eval()


def to_dev(prev, dev):
  return tuple(p.to(dev) for p in prev) if isinstance(prev, tuple) else prev.to(dev)


def rescore_many(odec, enc, lens, prev, b, hyps):
  """float64 scores of several token sequences of utterance b in one teacher-forced pass."""
  d = odec.double().eval()
  n, L = len(hyps), max(len(h) for h in hyps)
  st = _states(tuple(p.double() for p in prev) if isinstance(prev, tuple) else prev.double(), d.rnn_type)[b]
  st = tuple(s.expand(-1, n, -1).contiguous() for s in st) if isinstance(st, tuple) else st.expand(-1, n, -1).contiguous()
  tok = torch.full((n, L), PAD, dtype=torch.long)
  for i, h in enumerate(hyps):
    tok[i, :len(h)] = torch.tensor(h)
  x = torch.full((n,), BOS, dtype=torch.long)
  s = np.zeros(n)
  with torch.no_grad():
    for t in range(L):
      lp, st = d(x, st, lens[b:b + 1].expand(n), enc[b:b + 1].double().expand(n, -1, -1))
      for i, h in enumerate(hyps):
        if t < len(h):
          s[i] += float(lp[i, h[t]])
      x = tok[:, t]
  return s


def compare(odec, enc, lens, prev, got, K, Lmax):
  """Check the GPU's (ids, lens, scores) against the restatement; returns the number of near-tie utterances."""
  ids, glens, gsc = (t.cpu().numpy() for t in got)
  ref = beam_ref(odec, enc, lens, prev, K, Lmax)
  near = 0
  for b, (beam, margin) in enumerate(ref):
    n = len(beam)
    assert (glens[b, n:] == 0).all() and np.isneginf(gsc[b, n:]).all()
    hyps = [ids[b, k, :glens[b, k]].tolist() for k in range(n)]
    for h in hyps:
      assert 1 <= len(h) <= Lmax + 1 and (h[-1] == EOS or len(h) == Lmax + 1)
      assert EOS not in h[:-1] and PAD not in h and BOS not in h
    for k in range(n):
      assert (ids[b, k, glens[b, k]:] == PAD).all()
    tol = np.array([1e-4 + 1e-6 * len(h) for h, _ in beam])
    want = np.array([s for _, s in beam])
    if margin > NEAR:
      assert hyps == [h for h, _ in beam], b
      assert (np.abs(gsc[b, :n] - want) <= tol).all(), (b, gsc[b, :n] - want)
    else:
      near += 1
      rs = rescore_many(odec, enc, lens, prev, b, hyps)
      assert (np.abs(rs - gsc[b, :n]) <= tol).all(), (b, rs - gsc[b, :n])
      assert (np.abs(np.sort(rs)[::-1] - want) <= tol).all(), (b, np.sort(rs)[::-1] - want)
  return near


def run_case(dev, rnn_type, attn, Hd, layers, B, K, Lmax, seed, T=75, scale=16.0, eos_bias=0.0, poll=8):
  odec, enc, _, prev = small_case(rnn_type, attn, V=64, Hd=Hd, T=T, B=B, layers=layers, seed=seed, scale=scale,
                                  eos_bias=eos_bias)
  g = torch.Generator().manual_seed(seed)
  lens = torch.randint(T // 3, T + 1, (B,), generator=g)
  lens[0] = T
  hdec = hip_from_oracle(odec, dev)
  got = hdec.beam_search(enc.to(dev), lens.to(dev), to_dev(prev, dev), beam_width=K, max_label_len=Lmax,
                         poll_every=poll)
  torch.cuda.synchronize()
  assert 1 <= hdec.beam_rounds <= Lmax + 1
  return odec, enc, lens, prev, hdec, got


ATTNS = ["none", "dot", "general", "1_layer_nn", "concat"]
COVER = [(rt, at, nl) for rt in ("GRU", "LSTM") for at in ATTNS for nl in (1, 2)] + [("RNN", "dot", 1)]


@pytest.mark.parametrize("i,case", list(enumerate(COVER)))
def test_beam_matches_restatement(dev, i, case):
  rnn_type, attn, nl = case
  K = (1, 5, 10)[i % 3]
  Lmax = (100, 30, 20)[i % 3]
  B = 32 if i % 2 == 0 else 12
  odec, enc, lens, prev, _, got = run_case(dev, rnn_type, attn, 64, nl, B, K, Lmax, seed=100 + i,
                                           eos_bias=(0.0, 2.0)[i % 2])
  near = compare(odec, enc, lens, prev, got, K, Lmax)
  print("near-tie utterances: %d of %d" % (near, B))
  assert near <= (3 * B) // 4, (near, B)


@pytest.mark.parametrize("name,rnn_type,attn,Hd", [("defaults", "LSTM", "1_layer_nn", 700),
                                                   ("attn", "LSTM", "1_layer_nn", 1024),
                                                   ("ecd", "LSTM", "none", 1536)])
def test_shipped_decoder_shapes(dev, name, rnn_type, attn, Hd):
  B, K, Lmax = 32, 10, 100
  odec, enc, lens, prev, _, got = run_case(dev, rnn_type, attn, Hd, 1, B, K, Lmax, seed=7, scale=40.0,
                                           eos_bias=1.0)
  near = compare(odec, enc, lens, prev, got, K, Lmax)
  print("near-tie utterances: %d of %d" % (near, B))
  assert near <= (3 * B) // 4, near


def test_independent_of_batch_and_poll_interval(dev):
  odec, enc, lens, prev, hdec, got = run_case(dev, "GRU", "concat", 64, 1, 32, 5, 40, seed=11, poll=1)
  a = [t.cpu() for t in got]
  b = [t.cpu() for t in hdec.beam_search(enc.to(dev), lens.to(dev), to_dev(prev, dev), beam_width=5,
                                         max_label_len=40, poll_every=1000)]
  for x, y in zip(a, b):
    assert torch.equal(x, y)
  for u in (0, 5, 31):
    pu = tuple(p[:, u:u + 1] for p in prev) if isinstance(prev, tuple) else prev[:, u:u + 1]
    one = [t.cpu() for t in hdec.beam_search(enc[u:u + 1].to(dev), lens[u:u + 1].to(dev), to_dev(pu, dev),
                                             beam_width=5, max_label_len=40)]
    assert torch.equal(one[0][0], a[0][u]) and torch.equal(one[1][0], a[1][u])
    assert torch.allclose(one[2][0], a[2][u], rtol=0, atol=1e-5)


def test_beam_beats_greedy_on_the_device(dev):
  odec, enc, lens, prev = greedy_trap()
  hdec = hip_from_oracle(odec, dev)
  for K, want in ((1, [4, EOS]), (2, [3, EOS])):
    ids, ln, sc = hdec.beam_search(enc.to(dev), lens.to(dev), prev.to(dev), beam_width=K, max_label_len=3)
    for b in range(2):
      assert ids[b, 0, :ln[b, 0]].tolist() == want
    ref = beam_ref(odec, enc, lens, prev, K, 3)
    assert abs(float(sc[0, 0]) - ref[0][0][0][1]) < 1e-4


def test_inference_strings(dev):
  from lipreading_amd import analysis
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.attention_decoder import CharDecodingStep
  from oracle import torch_oracle as O
  torch.manual_seed(3)
  c2i = default_char2idx()
  enc = VideoEncoder(204, 32, rnn_type="GRU", bidirectional=False, enable_ctc=True, vocab_size=64, char2idx=c2i)
  oenc = O.OracleVideoEncoder(204, 32, rnn_type="GRU", bidirectional=False, enable_ctc=True, vocab_size=64,
                              char2idx=O.default_char2idx())
  oenc.load_state_dict(enc.state_dict())
  odec = O.OracleCharDecodingStep(32, "GRU", 1, 16, 64, c2i, attention_type="dot")
  with torch.no_grad():
    odec.output_proj.weight.mul_(16.0)
    odec.output_proj.bias[EOS] += 2.0
  dec = CharDecodingStep(enc, char_dim=16, vocab_size=64, char2idx=c2i, attention_type="dot")
  dec.load_state_dict(odec.state_dict())
  enc, dec = enc.to(dev), dec.to(dev)
  B, T = 4, 20
  frames = torch.randn(B, T, 68, 3)
  flens = torch.tensor([20, 15, 9, 20])
  for b in range(B):
    frames[b, int(flens[b]):] = 0
  chars = torch.tensor([[1, 40, 41, 2, 0], [1, 42, 2, 0, 0], [1, 43, 44, 45, 2], [1, 2, 0, 0, 0]])
  clens = torch.tensor([4, 3, 5, 2])
  outputs, gt = analysis.inference(enc, dec, frames, flens, chars, clens, dev, c2i, beam_width=5, max_label_len=12)
  idx2char = {v: k for k, v in c2i.items()}
  assert gt == [''.join(idx2char[int(c)] for c in chars[i][:int(clens[i])]) for i in range(B)]
  oenc.eval()
  with torch.no_grad():
    _, hid, state = oenc(frames, flens)
  ref = beam_ref(odec, hid, flens, state, 5, 12)
  for b in range(B):
    beam, margin = ref[b]
    want = "<BOS>" + ''.join(idx2char[i] for i in beam[0][0])
    assert outputs[b].startswith("<BOS>")
    if margin > NEAR:
      assert outputs[b] == want
  assert any(o.endswith("<EOS>") for o in outputs)


def test_attention_cer_and_driver_epoch(dev, tmp_path):
  """attention_cer on a small model trained on the synthetic nano dataview; the driver with --attn_decode=beam for one
  epoch."""
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  from lipreading_amd import train as T
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synthetic/nano", n_videos=3, captions_per_video=6, seed=1)
  tr, _, _ = DS.split_dataset(root, "synthetic/nano", 0.8, np.random.RandomState(123456))
  ds = DS.FrameCaptionDataset(root, "synthetic/nano", "train", tr)
  loader = DS.make_loader(ds, 4, make_collate_fn(dev))
  torch.manual_seed(123456)
  enc = VideoEncoder(204, 32, rnn_type="GRU", bidirectional=True, enable_ctc=True, vocab_size=len(ds.char2idx),
                     char2idx=ds.char2idx).to(dev)
  dec = CharDecodingStep(enc, char_dim=16, vocab_size=len(ds.char2idx), char2idx=ds.char2idx,
                         attention_type="1_layer_nn").to(dev)
  opt = (FusedAdam(FlatParameters(enc), lr=2e-3), FusedAdam(FlatParameters(dec), lr=2e-3))
  for _ in range(3):
    T.train(enc, dec, loader, opt, dev, ds.char2idx, grad_norm=50)
  cer = T.attention_cer(enc, dec, loader, dev, ds.char2idx, beam_width=4, max_label_len=60)
  assert np.isfinite(cer) and 0.0 <= cer <= 60.0
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=10, captions_per_video=6, seed=7)
  out = driver.run(**driver.parse_flags(["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True",
                                         "--rnn_type=GRU", "--hidden_size=32", "--char_dim=16", "--max_epochs=1",
                                         "--attn_decode=beam", "--attn_beam_width=3", "--attn_max_label_len=40"]))
  assert len(out["history"]) == 1
