"""GPU: the attention and joint beam searches with a word language model (CharDecodingStep.beam_search(lm=...),
lr_decoder_lm_beam_search) against fused_ref, the float64 restatement of tests/lm_fusion_cases.py
(checked on the CPU in tests/test_lm_fusion_cpu.py), with one set of weights in both decoders.

Tolerance, per hypothesis.  The joint test's (1 - lambda)(1e-4 + 1e-6 per token) + 1.2e-7 |s| + 1e-9 (the float32
attention sum, the float32 rounding of the returned score), plus for every scored in-vocabulary word
|alpha| * 2^-21 * order * M, M the largest |natural-log value| (probability or backoff) of the model: the packed table
holds float32 values, within 2^-24 relative of the float64 ones, lm_score adds at most `order` of them in float32,
which costs at most as much again, and 2^-21 covers both with room.  An OOV term adds nothing: -1000 is exact and the
term alpha * lm + beta is formed in float64 (alpha and beta of the cases are exact in float32).
Where the restatement's margin on s is above 1e-3 the token sequences must be identical; a near-tie utterance's
device hypotheses are re-scored in float64 (a by teacher forcing, c by the rule, l from the string by lm_terms) and the
sorted scores must match the restatement's.  Up to 75 % of a case's utterances may be near-ties, as in the other beam
tests; tests/test_lm_fusion_cpu.py holds the restatement itself to 50 %.
"""
import numpy as np
import pytest
import torch

from tests import lm_fusion_cases as F
from tests.test_attn_beam_cpu import BOS, EOS, PAD, UNK, small_case
from tests.test_gpu_attn_beam import NEAR, rescore_many, to_dev
from tests.test_joint_beam_cpu import ctc_score, joint_score, random_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def model_dir(tmp_path_factory):
  d = tmp_path_factory.mktemp("lm_fusion")
  F.set_dir(d)
  return d


def word_lm(path, labels, alpha, beta):
  from lipreading_amd.lm import WordLM
  return WordLM(path, list(labels), alpha=alpha, beta=beta)


def run(hdec, enc, lens, prev, y, dev, K, Lmax, lam, lm, P=None, poll=8, with_y=True):
  joint = {}
  if with_y:
    joint = dict(ctc_log_probs=torch.tensor(y, dtype=torch.float32, device=dev), ctc_weight=lam)
  got = hdec.beam_search(enc.to(dev), lens.to(dev), to_dev(prev, dev), beam_width=K, max_label_len=Lmax,
                         poll_every=poll, pre_beam=P, lm=lm, **joint)
  torch.cuda.synchronize()
  return got


def compare(ref, odec, enc, lens, prev, y, got, K, Lmax, lam, labels, rlm, alpha, beta, big):
  """Check the GPU's (ids, lens, scores) against the restatement's beams; returns the number of near-tie utterances."""
  ids, glens, gsc = (t.cpu().numpy() for t in got)
  near = 0

  def tol_of(h, s):
    hits = F.lm_terms(h, labels, rlm, alpha, beta)[1]
    return ((1 - lam) * (1e-4 + 1e-6 * len(h)) + 1.2e-7 * abs(s) + 1e-9 + hits * abs(alpha) * 2.0 ** -21 * rlm.order * big)

  for b, (beam, margin) in enumerate(ref):
    n = len(beam)
    assert (glens[b, n:] == 0).all() and np.isneginf(gsc[b, n:]).all(), b
    if n == 0:
      continue   # every candidate was a structural zero: the utterance ends with an empty beam
    hyps = [ids[b, k, :glens[b, k]].tolist() for k in range(n)]
    for k, h in enumerate(hyps):
      assert 1 <= len(h) <= Lmax + 1 and (h[-1] == EOS or len(h) == Lmax + 1)
      assert EOS not in h[:-1] and PAD not in h and BOS not in h
      assert (ids[b, k, glens[b, k]:] == PAD).all()
      # the dictionary: every run of word characters, completed or not, is a prefix of a vocabulary word
      assert F.lm_terms(h, labels, rlm, alpha, beta) is not None, (b, h)
    assert np.isfinite(gsc[b, :n]).all()
    want = np.array([e[1] for e in beam])
    if margin > NEAR:
      assert hyps == [e[0] for e in beam], b
      tol = np.array([tol_of(e[0], e[1]) for e in beam])
      assert (np.abs(gsc[b, :n] - want) <= tol).all(), (b, gsc[b, :n] - want, tol)
    else:
      near += 1
      a = rescore_many(odec, enc, lens, prev, b, hyps)
      c = np.array([ctc_score(h, y[b], int(lens[b])) if lam > 0 else 0.0 for h in hyps])
      l = np.array([F.lm_terms(h, labels, rlm, alpha, beta)[0] for h in hyps])
      rs = np.array([(joint_score(x, z, lam) if lam > 0 else x) + w for x, z, w in zip(a, c, l)])
      tol = np.array([tol_of(h, s) for h, s in zip(hyps, rs)])
      assert (np.abs(rs - gsc[b, :n]) <= tol).all(), (b, rs - gsc[b, :n], tol)
      order = np.argsort(-rs, kind="stable")
      assert (np.abs(rs[order] - want) <= tol[order]).all(), (b, rs[order] - want)
  return near


@pytest.mark.parametrize("case", F.CASES, ids=[c["id"] for c in F.CASES])
def test_matches_restatement(dev, case):
  odec, enc, lens, prev, y = F.inputs(case["id"])
  path = F.arpa(case["kind"], case["order"])
  rlm, _, big = F.ref_model(path, case["labels"])
  hdec = F.hip_decoder(odec, case["labels"], dev)
  lm = word_lm(path, case["labels"], case["alpha"], case["beta"])
  got = run(hdec, enc, lens, prev, y, dev, case["K"], F.LMAX, case["lam"], lm, P=case["P"], with_y=case["with_y"])
  assert 1 <= hdec.beam_rounds <= F.LMAX + 1
  ref = F.reference(case["id"])
  near = compare(ref, odec, enc, lens, prev, y, got, case["K"], F.LMAX, case["lam"], list(case["labels"]), rlm,
                 case["alpha"], case["beta"], big)
  scored = sum(F.lm_terms(e[0], list(case["labels"]), rlm, case["alpha"], case["beta"])[1] for beam, _ in ref
               for e in beam[:1])
  print("near-tie utterances: %d of %d; scored in-vocabulary words in the best hypotheses: %d" % (near, F.B, scored))
  assert near <= (3 * F.B) // 4, (near, F.B)
  assert scored > 0


def test_poll_interval_batch_and_null_frames_change_nothing(dev):
  case = F.CASE_BY_ID["GRU-concat-0.3-K5"]
  odec, enc, lens, prev, y = F.inputs(case["id"])
  hdec = F.hip_decoder(odec, case["labels"], dev)
  lm = word_lm(F.arpa(case["kind"], case["order"]), case["labels"], case["alpha"], case["beta"])
  K, P, lam = case["K"], case["P"], case["lam"]
  a = [t.cpu() for t in run(hdec, enc, lens, prev, y, dev, K, F.LMAX, lam, lm, P=P, poll=1)]
  b = [t.cpu() for t in run(hdec, enc, lens, prev, y, dev, K, F.LMAX, lam, lm, P=P, poll=1000)]
  for x, z in zip(a, b):
    assert torch.equal(x, z)
  for u in (0, 5, 11):
    pu = tuple(p[:, u:u + 1] for p in prev) if isinstance(prev, tuple) else prev[:, u:u + 1]
    one = [t.cpu() for t in run(hdec, enc[u:u + 1], lens[u:u + 1], pu, y[u:u + 1], dev, K, F.LMAX, lam, lm, P=P)]
    assert torch.equal(one[0][0], a[0][u]) and torch.equal(one[1][0], a[1][u])
    assert torch.allclose(one[2][0], a[2][u], rtol=0, atol=1e-5)
  # no CTC frames at all is the search at weight 0 with frames it never reads
  c = [t.cpu() for t in run(hdec, enc, lens, prev, y, dev, K, F.LMAX, 0.0, lm, P=P, with_y=False)]
  d = [t.cpu() for t in run(hdec, enc, lens, prev, y, dev, K, F.LMAX, 0.0, lm, P=P, with_y=True)]
  for x, z in zip(c, d):
    assert torch.equal(x, z)
  assert not torch.equal(a[0], c[0])   # and the frames do matter at weight 0.3


def test_the_model_flips_a_non_word_on_the_device(dev, model_dir):
  odec, enc, lens, prev = F.lm_trap()
  hdec = F.hip_decoder(odec, F.TRAP_LABELS, dev)
  lm = word_lm(F.write_trap_arpa(model_dir), F.TRAP_LABELS, 1.0, 0.0)
  ids, ln, _ = hdec.beam_search(enc.to(dev), lens.to(dev), prev.to(dev), beam_width=2, max_label_len=3)
  for b in range(2):
    assert ids[b, 0, :ln[b, 0]].tolist() == F.TRAP_ALONE
  ids, ln, sc = hdec.beam_search(enc.to(dev), lens.to(dev), prev.to(dev), beam_width=2, max_label_len=3, lm=lm)
  rlm, dic, _ = F.ref_model(F.write_trap_arpa(model_dir), tuple(F.TRAP_LABELS))
  ref = F.fused_ref(odec, enc, lens, prev, None, 2, 3, 0.0, None, rlm, dic, 1.0, 0.0)
  for b in range(2):
    assert ids[b, 0, :ln[b, 0]].tolist() == F.TRAP_FUSED
    assert abs(float(sc[b, 0]) - ref[b][0][0][1]) < 1e-4


def test_no_state_leaks_into_the_plain_searches(dev):
  case = F.CASE_BY_ID["LSTM-none-0.3-K5"]
  odec, enc, lens, prev, y = F.inputs(case["id"])
  hdec = F.hip_decoder(odec, case["labels"], dev)
  lm = word_lm(F.arpa(case["kind"], case["order"]), case["labels"], case["alpha"], case["beta"])
  yd = torch.tensor(y, dtype=torch.float32, device=dev)

  def plain():
    args = (enc.to(dev), lens.to(dev), to_dev(prev, dev))
    out = list(hdec.beam_search(*args, beam_width=5, max_label_len=F.LMAX))
    out += list(hdec.beam_search(*args, beam_width=5, max_label_len=F.LMAX, ctc_log_probs=yd, ctc_weight=0.3))
    return [t.cpu() for t in out]

  before = plain()
  run(hdec, enc, lens, prev, y, dev, 5, F.LMAX, 0.3, lm)
  run(hdec, enc, lens, prev, y, dev, 5, F.LMAX, 0.0, lm, with_y=False)
  after = plain()
  for x, z in zip(before, after):
    assert torch.equal(x, z)


def test_short_utterances_with_a_model(dev):
  """enc_lens 1 .. 3 at lambda = 0.5: most prefixes are structural zeros; no NaN, empty beams where the restatement
  has them, and agreement with the restatement."""
  Bs, Ts, K, Lmax, lam, alpha, beta = 8, 12, 6, 20, 0.5, 0.5, 0.25
  odec, enc, _, prev = small_case("GRU", "dot", V=32, Hd=64, T=Ts, B=Bs, seed=31, scale=4.0, eos_bias=4.0)
  with torch.no_grad():
    odec.output_proj.bias[UNK] -= 8.0   # EOS within the pre-beam, UNK rare: hypotheses end, and end in words
  lens = torch.tensor([1, 2, 3, 12, 1, 3, 2, 12])
  y = random_frames(Bs, Ts, 33, 31)
  path = F.arpa("az", 2)
  rlm, dic, big = F.ref_model(path, tuple(F.LABELS))
  hdec = F.hip_decoder(odec, F.LABELS, dev)
  got = run(hdec, enc, lens, prev, y, dev, K, Lmax, lam, word_lm(path, F.LABELS, alpha, beta))
  ids, glens, gsc = (t.cpu().numpy() for t in got)
  assert not np.isnan(gsc).any()
  for b in range(Bs):
    for k in range(K):
      if glens[b, k]:
        assert glens[b, k] - (ids[b, k, glens[b, k] - 1] == EOS) <= lens[b]   # labels fit the frames
  ref = F.fused_ref(odec, enc, lens, prev, y, K, Lmax, lam, None, rlm, dic, alpha, beta)
  assert any(not beam for beam, _ in ref) and any(0 < len(beam) < K for beam, _ in ref)
  assert any(e[4] != 0.0 for beam, _ in ref for e in beam)   # and the model has a say
  compare(ref, odec, enc, lens, prev, y, got, K, Lmax, lam, F.LABELS, rlm, alpha, beta, big)


def test_attention_cer_and_driver_epoch_with_a_model(dev, tmp_path):
  """One tiny epoch of the driver with --attn_decode=joint --attn_lm_path on both scoring routes, and on one trained
  model the host loop's and the device loop's CER of the fused search are the same float."""
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  from lipreading_amd import train as T
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.decoder import ctc_labels
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.lm import WordLM
  from lipreading_amd.optim import FlatParameters, FusedAdam
  from tests.test_beam_lm_cpu import write_arpa
  root = str(tmp_path)
  rng = np.random.default_rng(5)
  sents = [[DS._WORDS[int(i)] for i in rng.integers(len(DS._WORDS), size=int(rng.integers(2, 7)))] for _ in range(300)]
  arpa = write_arpa(str(tmp_path / "captions.arpa"), sents, 2)
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
  lm = WordLM(arpa, ctc_labels(ds.char2idx), alpha=0.5, beta=0.25)
  kw = dict(beam_width=4, max_label_len=60, lm=lm)
  for w in (0.0, 0.3):
    host = T.attention_cer(enc, dec, loader, dev, ds.char2idx, ctc_weight=w, **kw)
    assert np.isfinite(host) and 0.0 <= host <= 60.0
    assert T.device_cer(enc, loader, dev, ds.char2idx, decoding_step=dec, ctc_weight=w, **kw) == host
  plain = T.attention_cer(enc, dec, loader, dev, ds.char2idx, beam_width=4, max_label_len=60, ctc_weight=0.3)
  print("CER with the model %r, without %r" % (host, plain))
  flags = ["--enable_ctc=True", "--attn_decode=joint", "--attn_beam_width=4", "--attn_max_label_len=60",
           "--attn_lm_path=" + arpa, "--attn_lm_alpha=0.5", "--attn_lm_beta=0.25"]
  a = driver.make_error_of(driver.parse_flags(flags), enc, dec, None, dev, ds.char2idx)
  d = driver.make_error_of(driver.parse_flags(flags + ["--score=device"]), enc, dec, None, dev, ds.char2idx)
  assert a(loader) == d(loader) == host
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=10, captions_per_video=6, seed=7)
  for route in ("host", "device"):
    out = driver.run(**driver.parse_flags(["--root=" + root, "--data=synth/micro", "--batch_size=8", "--rnn_type=GRU",
                                           "--hidden_size=32", "--char_dim=16", "--max_epochs=1", "--attn_beam_width=3",
                                           "--attn_max_label_len=40", "--score=" + route] + flags[:2] + flags[4:]))
    assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["val_cer"])
