"""GPU: CharDecodingStep.rescore (lr_decoder_rescore) against the float64 restatement of
tests/rescore_cases.py, with one set of random weights loaded into both CharDecodingStep and OracleCharDecodingStep.

Tolerance.  The device computes each log-probability in float32 and sums them in float64; the restatement is float64
throughout.  out_attn is held to 1e-4 + 1e-6 per scored token, the project's own bound for these sums
(tests/test_gpu_attn_beam.py).  The combined score s = (1 - lambda) a - lambda f + gamma |q| carries that error scaled
by (1 - lambda) — f and |q| are exact on both sides — and is returned in float32: 1e-6 |s| more.  Where every adjacent
gap of the restatement's sorted s exceeds NEAR = 1e-3 that error cannot change the order, which must then be identical;
in a near-tie utterance the device's order, scored by the restatement, must be non-increasing within the tolerance.
Which slots are scored, which cannot be and which are empty never depends on arithmetic: that placement is always
exact.  At most a quarter of a case's utterances may be near-ties; the seeds below were counted on the CPU with the
restatement alone (3 of 32 utterances in the three largest cases, none in the others; each case prints its count)."""
import numpy as np
import pytest
import torch

from tests.rescore_cases import EMPTY, SCORABLE, UNSCORABLE, random_lists, rescore_ref
from tests.test_attn_beam_cpu import BOS, EOS, PAD, small_case
from tests.test_gpu_attn_beam import COVER, NEAR, hip_from_oracle, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def make_case(rnn_type, attn, layers, B, N, W, T, V, seed):
  odec, enc, _, prev = small_case(rnn_type, attn, V=V, Hd=64, T=T, B=B, layers=layers, seed=seed, scale=4.0)
  g = torch.Generator().manual_seed(seed)
  lens = torch.randint(max(1, T // 3), T + 1, (B,), generator=g)
  lens[0] = T
  ids, hl, first = random_lists(B, N, W, V, seed)
  return odec, enc, lens, prev, ids, hl, first


def run(hdec, dev, enc, lens, prev, ids, hl, first, N, W, lam, gamma):
  """ids goes in as a strided view of the wider tensor."""
  wide = ids.to(dev)
  view = wide[:, :N, :W]
  got = hdec.rescore(enc.to(dev), lens.to(dev), to_dev(prev, dev), view, hl.to(dev), first.to(dev), ctc_weight=lam,
                     length_bonus=gamma)
  torch.cuda.synchronize()
  return [t.cpu() for t in got]


def compare(ref, got, lam):
  """The device's (order, scores, attn) against the restatement; returns the number of near-tie utterances."""
  order, sc, at = (t.numpy() for t in got)
  near = 0
  for b, r in enumerate(ref):
    N = len(r["cls"])
    o = order[b].tolist()
    assert sorted(o) == list(range(N)), b
    n_sc = sum(c == SCORABLE for c in r["cls"])
    assert [r["cls"][n] for n in o] == [r["cls"][n] for n in r["order"]], b   # the placement of the three classes
    assert o[n_sc:] == r["order"][n_sc:], b                                    # ... and first-pass order inside them
    assert np.isneginf(sc[b, n_sc:]).all() and np.isneginf(at[b, n_sc:]).all(), b
    tol_a = np.array([1e-4 + 1e-6 * len(r["q"][n]) for n in o[:n_sc]])
    want_a = np.array([r["a_slot"][n] for n in o[:n_sc]])
    want_s = np.array([r["s_slot"][n] for n in o[:n_sc]])
    tol_s = (1 - lam) * tol_a + 1e-6 * np.abs(want_s)
    assert (np.abs(at[b, :n_sc] - want_a) <= tol_a).all(), (b, np.abs(at[b, :n_sc] - want_a).max())
    assert (np.abs(sc[b, :n_sc] - want_s) <= tol_s).all(), (b, np.abs(sc[b, :n_sc] - want_s).max())
    gaps = -np.diff(np.array(r["s"][:n_sc]))
    if (gaps > NEAR).all():
      assert o == r["order"], b
    else:
      near += 1
      assert (np.diff(want_s) <= tol_s[1:] + tol_s[:-1]).all(), b
  return near


def shapes(i):
  """The issue's sets spread over the cases: B {1, 5, 32}, N {1, 3, 10, 32, 128}, W {1, 12, 75}, T {6, 75},
  lambda {0, 0.3, 1}, gamma {0, 0.5}."""
  z = dict(B=(1, 5, 32)[i % 3], N=(1, 3, 10, 32, 128)[i % 5], W=(12, 75, 1)[(i + i // 3) % 3], T=(6, 75)[i % 2],
           lam=(0.0, 0.3, 1.0)[(i + i // 5) % 3], gamma=(0.0, 0.5)[(i // 2) % 2])
  if z["W"] == 1 and z["N"] > 10 and z["lam"] == 0.0:
    z["lam"] = 1.0   # 32 one-token sequences over 62 tokens repeat, and equal sequences tie exactly at lambda = 0
  return z


CASES = [(i, c + (64,)) for i, c in enumerate(COVER)] + [(len(COVER), ("LSTM", "1_layer_nn", 1, 37)),
                                                         (len(COVER) + 1, ("GRU", "dot", 1, 64))]


SEEDS = {18: 518}   # 300 + i elsewhere; seed 318 puts two of the single utterance's 32 scores within NEAR


@pytest.mark.parametrize("i,case", CASES)
def test_rescore_matches_restatement(dev, i, case):
  rnn_type, attn, nl, V = case
  z = shapes(i)
  if i == len(COVER) + 1:
    z.update(B=32, N=128, W=75, T=75, lam=0.3, gamma=0.5)   # the largest of every set at once
  B, N, W, T, lam, gamma = (z[k] for k in ("B", "N", "W", "T", "lam", "gamma"))
  odec, enc, lens, prev, ids, hl, first = make_case(rnn_type, attn, nl, B, N, W, T, V, seed=SEEDS.get(i, 300 + i))
  hdec = hip_from_oracle(odec, dev)
  got = run(hdec, dev, enc, lens, prev, ids, hl, first, N, W, lam, gamma)
  ref = rescore_ref(odec, enc, lens, prev, ids[:, :N, :W].tolist(), hl.tolist(), first.tolist(), lam, gamma, many=True)
  near = compare(ref, got, lam)
  print("case %d %s: near-tie utterances: %d of %d" % (i, z, near, B))
  assert near <= B // 4, (near, B)


def test_weight_one_is_the_identity_bit_for_bit(dev):
  B, N, W = 5, 10, 12
  odec, enc, lens, prev, ids, hl, _ = make_case("LSTM", "dot", 1, B, N, W, 20, 64, seed=21)
  g = np.random.RandomState(3)
  toks = g.randint(3, 64, size=(B, N, W)).astype(np.int32) + 1     # every slot scorable: characters only
  hl = torch.from_numpy(g.randint(0, W + 1, size=(B, N)).astype(np.int32))
  first = np.sort(g.uniform(0, 50, size=(B, N)).astype(np.float32), axis=1)
  first[:, 3] = first[:, 4] = first[:, 5]                         # several equal first-pass scores
  first[:, 8] = first[:, 9]
  first = torch.from_numpy(first)
  hdec = hip_from_oracle(odec, dev)
  order, sc, at = run(hdec, dev, enc, lens, prev, torch.from_numpy(toks), hl, first, N, W, 1.0, 0.0)
  assert torch.equal(order, torch.arange(N, dtype=torch.int32).expand(B, N))
  assert torch.equal(sc, -first)
  assert torch.isfinite(at).all() and (at < 0).all()


def test_agrees_with_decode_sequence_on_tiled_inputs(dev):
  """out_attn against the gathered and summed log_probs of decode_sequence on enc / lens / state tiled N times."""
  B, N, W, T = 5, 10, 12, 20
  odec, enc, lens, prev, ids, hl, first = make_case("LSTM", "general", 2, B, N, W, T, 64, seed=22)
  hdec = hip_from_oracle(odec, dev)
  order, sc, at = run(hdec, dev, enc, lens, prev, ids, hl, first, N, W, 0.0, 0.0)
  ref = rescore_ref(odec, enc, lens, prev, ids[:, :N, :W].tolist(), hl.tolist(), first.tolist(), 0.0, 0.0, many=True)
  L = W + 1
  tokens = torch.full((B * N, L), PAD, dtype=torch.int32)
  tokens[:, 0] = BOS
  for b in range(B):
    for n in range(N):
      q = ref[b]["q"][n]
      if ref[b]["cls"][n] == SCORABLE:
        tokens[b * N + n, 1:len(q)] = torch.tensor(q[:-1], dtype=torch.int32)
  tile = lambda t, d: t.repeat_interleave(N, dim=d)
  state = tuple(tile(p, 1) for p in prev) if isinstance(prev, tuple) else tile(prev, 1)
  with torch.no_grad():
    lp = hdec.decode_sequence(tokens.to(dev), to_dev(state, dev), tile(lens, 0).to(dev), tile(enc, 0).to(dev))[0]
  lp = lp.double().cpu()
  for b in range(B):
    for r, n in enumerate(order[b].tolist()):
      if ref[b]["cls"][n] != SCORABLE:
        continue
      q = ref[b]["q"][n]
      want = sum(float(lp[b * N + n, i, v]) for i, v in enumerate(q))
      assert abs(float(at[b, r]) - want) <= 1e-4 + 1e-6 * len(q), (b, n, float(at[b, r]) - want)


def test_beam_search_output_comes_back_at_weight_zero(dev):
  """The attention beam search's own beam (K = 5), ids + 1 as classes: at lambda = 0 its scores come back within the
  bound, and its order where its margins exceed NEAR."""
  B, K, Lmax = 12, 5, 20
  odec, enc, _, prev = small_case("GRU", "1_layer_nn", V=64, Hd=64, T=30, B=B, seed=23, scale=16.0, eos_bias=2.0)
  lens = torch.tensor([30 - b for b in range(B)])
  hdec = hip_from_oracle(odec, dev)
  ids, bl, bs = hdec.beam_search(enc.to(dev), lens.to(dev), to_dev(prev, dev), beam_width=K, max_label_len=Lmax)
  assert (bl > 0).all()
  first = torch.arange(K, dtype=torch.float32, device=dev).expand(B, K).contiguous()
  order, sc, at = hdec.rescore(enc.to(dev), lens.to(dev), to_dev(prev, dev), ids + 1, bl, first, ctc_weight=0.0)
  order, sc, at, bl, bs = (t.cpu() for t in (order, sc, at, bl, bs))
  ids = ids.cpu()
  for b in range(B):
    o = order[b].long()
    # (a hypothesis the search capped without EOS gets one appended by the rule: its score is another sequence's)
    ended = torch.tensor([int(ids[b, k, int(bl[b, k]) - 1]) == EOS for k in range(K)])
    tol = 1e-4 + 1e-6 * bl[b].double()
    err = (at[b].double() - bs[b][o].double()).abs()
    assert (err[ended[o]] <= tol[o][ended[o]]).all(), b
    assert torch.equal(sc[b], at[b])
    if ended.all() and ((bs[b, :-1] - bs[b, 1:]) > NEAR).all():
      assert o.tolist() == list(range(K)), b


def test_same_call_twice_gives_the_same_bits(dev):
  odec, enc, lens, prev, ids, hl, first = make_case("GRU", "concat", 2, 32, 32, 12, 75, 64, seed=24)
  hdec = hip_from_oracle(odec, dev)
  a = run(hdec, dev, enc, lens, prev, ids, hl, first, 32, 12, 0.3, 0.5)
  b = run(hdec, dev, enc, lens, prev, ids, hl, first, 32, 12, 0.3, 0.5)
  for x, y in zip(a, b):
    assert torch.equal(x, y)
  c = run(hdec, dev, enc, lens, prev, ids[:, :32, :12].contiguous(), hl, first, 32, 12, 0.3, 0.5)   # no stride
  for x, y in zip(a, c):
    assert torch.equal(x, y)


# ---- sessions -------------------------------------------------------------------------------------------------------
def _two_pass_model(dev, rnn_type="LSTM"):
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  from tests.test_gpu_encoder_stream import _char2idx, _encoder
  enc = _encoder(dev, rnn_type=rnn_type)
  c2i = _char2idx()
  torch.manual_seed(12)
  step = CharDecodingStep(enc, char_dim=16, vocab_size=len(c2i), char2idx=c2i, attention_type="dot").to(dev).eval()
  ctc = BeamCTCDecoder(ctc_labels(c2i), beam_width=8, log_probs_input=True)
  return enc, step, ctc, c2i


def test_two_pass_transcriber_is_cut_independent(dev):
  from lipreading_amd.encoder_stream import ChunkedEncoder, TwoPassTranscriber
  enc, step, ctc, _ = _two_pass_model(dev)
  B, T, n = 3, 14, 6
  g = torch.Generator().manual_seed(6)
  frames = torch.randn(B, T, 68, 3, generator=g).to(dev)
  lens = torch.tensor([14, 9, 12], dtype=torch.int32, device=dev)
  runs = []
  for chunk in (1, 5, T):
    tp = TwoPassTranscriber(enc, step, ctc, B, T, dev)
    for t0 in range(0, T, chunk):
      t1 = min(T, t0 + chunk)
      tp.feed(frames[:, t0:t1], (lens - t0).clamp(0, t1 - t0))
    got = tp.rescored_ids(n, ctc_weight=0.4, length_bonus=0.1)
    runs.append(([t.cpu() for t in got], tp.rescored(n, ctc_weight=0.4, length_bonus=0.1), tp.result()))
  for other in runs[1:]:
    for x, y in zip(runs[0][0], other[0]):
      assert torch.equal(x, y)
    assert runs[0][1][0] == other[1][0]
  # ... and they are rescore's on the one-piece encoder pass plus decode_ids of the same model
  with torch.no_grad():
    lp, hidden, state = ChunkedEncoder(enc, T)(frames, lens, max_len=T)
  ids, off, hl, first = ctc.decode_ids(lp, lens)
  order, sc, at = step.rescore(hidden, lens, state, ids[:, :n], hl[:, :n], first[:, :n], ctc_weight=0.4,
                               length_bonus=0.1)
  o = order.long()
  got = runs[0][0]
  assert torch.equal(got[0], torch.gather(ids[:, :n], 1, o[:, :, None].expand(-1, -1, T)).cpu())
  assert torch.equal(got[2], torch.gather(hl[:, :n], 1, o).cpu())
  assert torch.equal(got[3], sc.cpu()) and torch.equal(got[4], at.cpu())
  # the strings: the first pass's n best, reordered; partial() / result() stay the first pass's
  strings, offsets = runs[0][1]
  first_pass = runs[0][2][0]
  for b in range(B):
    assert len(strings[b]) == n and sorted(strings[b]) == sorted(first_pass[b][:n])
    assert strings[b] == [first_pass[b][k] for k in order[b].tolist()]
    assert [len(x) for x in offsets[b]] == got[2][b].tolist()
  # against VideoEncoder.forward, whose recurrence is not the session's bit for bit (tests/test_gpu_encoder_stream.py
  # holds the two to 1e-4 per log-probability): the SAME hypothesis list rescored from either pass, slot by slot.
  # A slot's sum has at most T + 1 = 15 terms, each moved by the encoder's 1e-4 at the most: 1e-3 bounds it with room.
  with torch.no_grad():
    _, hidden1, state1 = enc(frames, lens, max_len=T)
  o1, _, at1 = step.rescore(hidden1, lens, state1, ids[:, :n], hl[:, :n], first[:, :n], ctc_weight=0.0)
  o0, _, at0 = step.rescore(hidden, lens, state, ids[:, :n], hl[:, :n], first[:, :n], ctc_weight=0.0)
  slot0 = torch.empty_like(at0).scatter_(1, o0.long(), at0)   # ranked -> by input slot
  slot1 = torch.empty_like(at1).scatter_(1, o1.long(), at1)
  fin = torch.isfinite(slot0)
  assert torch.equal(fin, torch.isfinite(slot1)) and fin.any()
  assert (slot1[fin] - slot0[fin]).abs().max() < 1e-3


def test_two_pass_reset_leaves_unmasked_slots(dev):
  from lipreading_amd.encoder_stream import TwoPassTranscriber
  enc, step, ctc, _ = _two_pass_model(dev, rnn_type="GRU")
  B, T, n = 3, 12, 4
  g = torch.Generator().manual_seed(7)
  frames = torch.randn(B, T, 68, 3, generator=g).to(dev)
  tp = TwoPassTranscriber(enc, step, ctc, B, T, dev)
  tp.feed(frames[:, :7])
  before = [t.cpu() for t in tp.rescored_ids(n)]
  hidden = tp.hidden.clone()
  mask = torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)
  tp.reset(mask)
  after = [t.cpu() for t in tp.rescored_ids(n)]
  for x, y in zip(before[:5], after[:5]):
    assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2])
  assert torch.equal(tp.hidden[0], hidden[0]) and torch.equal(tp.hidden[2], hidden[2]) and (tp.hidden[1] == 0).all()
  assert (after[2][1] == 0).all()                      # the reset slot holds no hypothesis with characters ...
  tp.feed(frames[:, 7:], torch.tensor([5, 5, 0], dtype=torch.int32, device=dev))
  tp.feed(frames[:, :7], torch.tensor([0, 7, 0], dtype=torch.int32, device=dev))
  last = [t.cpu() for t in tp.rescored_ids(n)]
  for x, y in zip(before[:5], last[:5]):
    assert torch.equal(x[2], y[2])                     # slot 2 was idle throughout
  assert torch.equal(tp.hidden[2], hidden[2]) and (tp.hidden[2, 7:] == 0).all()
  assert (tp.hidden[1] != 0).any(dim=1).all()          # ... and slot 1 filled its 12 frames again from frame 0
  strings, _ = tp.rescored(n)
  assert len(strings) == B and all(len(s) == n for s in strings)


# ---- rejections -----------------------------------------------------------------------------------------------------
def test_rejections_make_no_launch(dev):
  import ctypes
  from lipreading_amd import _C
  odec, enc, lens, prev, ids, hl, first = make_case("GRU", "dot", 2, 2, 3, 4, 6, 64, seed=25)
  hdec = hip_from_oracle(odec, dev)
  e, l, p = enc.to(dev), lens.to(dev), to_dev(prev, dev)
  i, h, f = ids[:, :3, :4].to(dev), hl.to(dev), first.to(dev)
  out = [torch.full((2, 3), 7, dtype=torch.int32, device=dev), torch.full((2, 3), 7.0, device=dev),
         torch.full((2, 3), 7.0, device=dev)]
  for kw in (dict(ctc_weight=1.5), dict(ctc_weight=float("nan")), dict(length_bonus=float("inf"))):
    with pytest.raises(ValueError):
      hdec.rescore(e, l, p, i, h, f, **kw)
  for bad in (dict(hyp_ids=i.cpu()), dict(hyp_ids=i.long()), dict(hyp_lens=h[:, :2]), dict(previous_state=(p, p))):
    args = dict(encoder_hidden_states=e, encoder_lens=l, previous_state=p, hyp_ids=i, hyp_lens=h, first_scores=f)
    args.update(bad)
    with pytest.raises(ValueError):
      hdec.rescore(**args)
  # the raw ABI: every rejection comes back before anything is launched, so the outputs keep their fill
  L_ = _C.lib()
  params = hdec._params()
  pstruct = _C.DecoderParams(*[_C.ptr(x) for x in params[:13]], hdec.output_mask.data_ptr())
  from lipreading_amd.attention_decoder import _upper_struct
  ustruct, NL = _upper_struct(params[13:], None)
  B, N, W, T, Hd, Cd, V = 2, 3, 4, 6, 64, hdec.char_dim, 64
  mode = _C.LR_RNN_GRU
  nbytes = L_.lr_decoder_rescore_workspace_bytes(mode, 1, NL, B, N, W, T, Hd, Cd, V, 0)
  assert nbytes > 0
  ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
  ic, l32 = i.contiguous(), l.to(torch.int32)

  def call(lam=0.5, gamma=0.0, up=ustruct, ids_ptr=None, nb=nbytes, N_=N, sb=None):
    return L_.lr_decoder_rescore(mode, 1, ctypes.byref(pstruct), ctypes.byref(up), e.data_ptr(), l32.data_ptr(),
                                 p.data_ptr(), None, ic.data_ptr() if ids_ptr is None else ids_ptr,
                                 ic.stride(0) if sb is None else sb, ic.stride(1), h.data_ptr(), f.data_ptr(), BOS, EOS,
                                 PAD, lam, gamma, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                 ws.data_ptr(), nb, B, N_, W, T, Hd, Cd, V, 0, _C.stream_handle())
  masked = _C.DecoderUpper()
  ctypes.memmove(ctypes.byref(masked), ctypes.byref(ustruct), ctypes.sizeof(masked))
  masked.drop_mask = ws.data_ptr()
  assert call(lam=-0.5) == _C.LR_ERR_INVALID_ARG
  assert call(lam=float("nan")) == _C.LR_ERR_INVALID_ARG
  assert call(gamma=float("-inf")) == _C.LR_ERR_INVALID_ARG
  assert call(up=masked) == _C.LR_ERR_INVALID_ARG
  assert call(sb=-1) == _C.LR_ERR_INVALID_ARG
  assert call(N_=129) == _C.LR_ERR_UNSUPPORTED
  assert call(nb=nbytes - 1) == _C.LR_ERR_WORKSPACE
  torch.cuda.synchronize()
  assert (out[0] == 7).all() and (out[1] == 7).all() and (out[2] == 7).all()
  assert call() == _C.LR_OK
  torch.cuda.synchronize()
  want = hdec.rescore(e, l, p, i, h, f)
  for x, y in zip(out, want):
    assert torch.equal(x, y)


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_driver_epoch_with_rescore(dev, tmp_path):
  """One tiny epoch of the driver on the synthetic nano dataview with --attn_decode=rescore: both --score routes
  report the same CER, and so does the streamed evaluation (--stream_chunk with the encoder session)."""
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=10, captions_per_video=6, seed=7)
  base = ["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True", "--rnn_type=GRU",
          "--hidden_size=32", "--char_dim=16", "--max_epochs=1", "--bidirectional=False", "--attn_decode=rescore",
          "--ctc_decoder=beam", "--beam_width=8", "--attn_rescore_nbest=5", "--attn_ctc_weight=0.4"]
  outs = [driver.run(**driver.parse_flags(base + extra))
          for extra in ([], ["--score=device"], ["--stream_chunk=5", "--stream_encoder=True"])]
  for out in outs:
    assert len(out["history"]) == 1
  cers = [out["history"][0]["val_cer"] for out in outs]
  print("val_cer host / device / streamed:", cers)
  assert np.isfinite(cers[0]) and cers[0] == cers[1] == cers[2]
