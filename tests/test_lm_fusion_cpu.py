"""CPU: fused_ref (tests/lm_fusion_cases.py), the float64 restatement of the word-language-model fusion in the
attention and joint beam searches (lr_decoder_lm_beam_search, lipreading_amd/csrc/lr_attn_beam.hip),
checked against exhaustive enumeration with an independent string scorer, against joint_ref with a model that changes
nothing, and on a readable trap; the ABI's, beam_search's and WordLM's rejections; the driver's flags; and the margins
of the GPU cases of tests/test_gpu_lm_fusion.py, which holds the device against this restatement."""
import numpy as np
import pytest
import torch

from tests import lm_fusion_cases as F
from tests.test_attn_beam_cpu import EOS, complete_hypotheses, rescore, small_case
from tests.test_beam_lm_cpu import TOY, Dict, RefLM, write_arpa
from tests.test_gpu_attn_beam import NEAR
from tests.test_joint_beam_cpu import NEG, ctc_score, joint_ref, joint_score, random_frames


@pytest.fixture(scope="module", autouse=True)
def model_dir(tmp_path_factory):
  d = tmp_path_factory.mktemp("lm_fusion")
  F.set_dir(d)
  return d


def toy_model(tmp_path, labels):
  from lipreading_amd.lm import read_arpa
  p = tmp_path / "toy.arpa"
  p.write_text(TOY)
  lm = RefLM(read_arpa(str(p)))
  return lm, Dict(lm, labels)


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rnn_type,attn,Lmax,lam,alpha,beta", [
    ("GRU", "dot", 3, 0.0, 1.0, 0.0), ("LSTM", "concat", 2, 0.5, 0.5, -0.5), ("RNN", "none", 3, 1.0, 2.0, 1.0),
    ("GRU", "general", 2, 0.0, 0.5, -0.5), ("LSTM", "1_layer_nn", 3, 0.5, 1.0, 0.0), ("RNN", "dot", 2, 1.0, 0.5, -0.5),
    ("GRU", "none", 4, 0.0, 2.0, 1.0)])
def test_exhaustive_search(tmp_path, rnn_type, attn, Lmax, lam, alpha, beta):
  """V = 7 (the specials, ' ', 'a', 'b'), P = V - 2 and K the number of complete hypotheses: nothing is pruned, so the
  beam is every complete hypothesis the dictionary and the frames allow, each scored from its string by lm_terms."""
  labels = F.TRAP_LABELS
  lm, dic = toy_model(tmp_path, labels)   # words a, ab, bb; order 3
  dec, enc, lens, prev = small_case(rnn_type, attn, V=7, T=6, B=2, seed=4, scale=3.0)
  lens = torch.tensor([6, 4])
  y = random_frames(2, 6, 8, 12, peak=1.0)
  hyps = complete_hypotheses(7, Lmax)
  K = len(hyps)
  got = F.fused_ref(dec, enc, lens, prev, y if lam > 0 else None, K, Lmax, lam, 5, lm, dic, alpha, beta)
  forbidden = zeros = 0
  for b in range(2):
    want = []
    for h in hyps:
      t = F.lm_terms(h, labels, lm, alpha, beta)
      if t is None:
        forbidden += 1
        continue
      a = rescore(dec, enc, lens, prev, b, h)
      c = ctc_score(h, y[b], int(lens[b])) if lam > 0 else 0.0
      if c == NEG:
        zeros += 1
        continue
      want.append((h, (joint_score(a, c, lam) if lam > 0 else a) + t[0], t[0]))
    want.sort(key=lambda e: -e[1])
    beam, _ = got[b]
    assert [h for h, *_ in beam] == [h for h, *_ in want], b
    np.testing.assert_allclose([e[1] for e in beam], [s for _, s, _ in want], rtol=0, atol=1e-9)
    np.testing.assert_allclose([e[4] for e in beam], [l for _, _, l in want], rtol=0, atol=1e-9)
    assert any(l <= -1000 * alpha + 50 for _, _, l in want) and any(l > -50 for _, _, l in want)   # OOV and in-vocabulary
  assert forbidden > 0 and (zeros > 0 or lam == 0)


@pytest.mark.parametrize("lam", [0.0, 0.4, 1.0])
def test_a_model_that_changes_nothing_gives_the_joint_search(tmp_path, lam):
  """alpha = beta = 0 and every word over {a, b} that a hypothesis can spell (up to Lmax + 1 letters: the cap lets a
  hypothesis grow to Lmax + 1 tokens) in the vocabulary: no term, no exclusion, so fused_ref is joint_ref exactly."""
  import itertools
  from lipreading_amd.lm import read_arpa
  Lmax = 3
  words = ["".join(w) for n in range(1, Lmax + 2) for w in itertools.product("ab", repeat=n)]
  path = write_arpa(str(tmp_path / "all.arpa"), [[w] for w in words], 2)
  lm = RefLM(read_arpa(path))
  dic = Dict(lm, F.TRAP_LABELS)
  dec, enc, lens, prev = small_case("LSTM", "dot", V=7, T=6, B=3, seed=6, scale=2.0, eos_bias=0.5)
  y = random_frames(3, 6, 8, 7)
  for K, P in ((1, 5), (3, 5), (4, 4)):
    want = joint_ref(dec, enc, lens, prev, y, K, Lmax, lam, P=P)
    got = F.fused_ref(dec, enc, lens, prev, y, K, Lmax, lam, P, lm, dic, 0.0, 0.0)
    for (wb, wm), (gb, gm) in zip(want, got):
      assert [h for h, *_ in wb] == [h for h, *_ in gb]
      assert [s for _, s, _, _ in wb] == [e[1] for e in gb] and wm == gm
      assert all(e[4] == 0.0 for e in gb)


def test_the_model_flips_a_non_word(tmp_path):
  from lipreading_amd.lm import read_arpa
  dec, enc, lens, prev = F.lm_trap()
  lm = RefLM(read_arpa(F.write_trap_arpa(tmp_path)))
  dic = Dict(lm, F.TRAP_LABELS)
  y = random_frames(2, 3, 8, 1)
  alone = joint_ref(dec, enc, lens, prev, y, 2, 3, 0.0)
  fused = F.fused_ref(dec, enc, lens, prev, None, 2, 3, 0.0, None, lm, dic, 1.0, 0.0)
  for b in range(2):
    assert alone[b][0][0][0] == F.TRAP_ALONE
    assert fused[b][0][0][0] == F.TRAP_FUSED
    # 'ab' after <s>: the listed bigram, ln 10 * -0.1
    assert fused[b][0][0][4] == pytest.approx(-0.1 * np.log(10.0), abs=1e-12)


# ---- rejections, without a device ----------------------------------------------------------------------------------
OK = (1, 3, 1, 4, 10, 100, 75, 64, 32, 64, 0, 65, 15)   # the joint query's arguments


def test_lm_workspace_query_rejects_bad_sizes():
  from lipreading_amd import _C
  q = _C.lib().lr_decoder_lm_beam_workspace_bytes
  assert q(*OK) > _C.lib().lr_decoder_joint_beam_workspace_bytes(*OK)
  for i, bad in [(4, 0), (4, 33), (9, 1025), (11, 64), (11, 66), (12, 9), (12, 63), (6, 65536), (5, 0), (3, 0)]:
    args = list(OK)
    args[i] = bad
    assert q(*args) == 0, (i, bad)
  assert q(1, 3, 1, 4, 10, 100, 75, 64, 32, 255, 0, 256, 15) > 0    # V + 1 = 256: the limit
  assert q(1, 3, 1, 4, 10, 100, 75, 64, 32, 256, 0, 257, 15) == 0
  assert _C.lib().lr_decoder_joint_beam_workspace_bytes(1, 3, 1, 4, 10, 100, 75, 64, 32, 256, 0, 257, 15) > 0


def test_lm_entry_rejects_without_a_device():
  import ctypes
  from lipreading_amd import _C
  L_ = _C.lib()
  buf = ctypes.create_string_buffer(64)   # a non-NULL pointer the entry never gets to read
  some = ctypes.addressof(buf)

  def call(V=64, lam=0.3, y=some, lm=some, roles=some, alpha=0.5, beta=0.0, K=10, P=15):
    C = V + 1
    return L_.lr_decoder_lm_beam_search(1, 3, None, None, None, None, None, None, y, 75 * C, C, C, 0, lam, P, lm,
                                        roles, alpha, beta, 1, 2, 0, K, 100, 1, None, None, None, None, None, 0, 4, 75,
                                        64, 32, V, 0, None)
  assert call(lm=None) == -1 and call(roles=None) == -1
  assert call(alpha=float("inf")) == -1 and call(beta=float("nan")) == -1
  assert call(y=None, lam=0.3) == -1
  assert call(lam=1.5) == -1
  assert call(V=256) == -4 and call(V=255) == -1     # beyond the trie key; within it, only the NULL params are wrong
  assert call(P=9) == -4 and call(K=33) == -4
  assert call(y=None, lam=0.0) == -1                 # allowed: it reaches the search's own NULL checks


@pytest.fixture
def az_lm(model_dir):
  from lipreading_amd.lm import WordLM
  return WordLM(F.arpa("az", 2), F.LABELS, alpha=0.5, beta=0.25)


def small_decoder(labels):
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.encoder import VideoEncoder
  enc = VideoEncoder(204, 16, rnn_type="GRU", bidirectional=False)
  return CharDecodingStep(enc, char_dim=8, vocab_size=len(labels) - 1, char2idx=F.char2idx(labels),
                          attention_type="dot")


def test_beam_search_lm_raises_for_bad_inputs(az_lm, model_dir):
  from lipreading_amd.lm import WordLM
  dec = small_decoder(F.LABELS)
  h, lens, prev = torch.zeros(2, 5, 16), torch.tensor([5, 4]), torch.zeros(1, 2, 16)
  with pytest.raises(ValueError, match="GPU"):
    dec.beam_search(h, lens, prev, lm=az_lm)
  with pytest.raises(ValueError, match="pre_beam"):
    dec.beam_search(h, lens, prev, lm=az_lm, pre_beam=9)
  with pytest.raises(ValueError, match="pre_beam"):
    dec.beam_search(h, lens, prev, lm=az_lm, pre_beam=31)
  foreign = WordLM(F.arpa("az", 2), F.LABELS[:1] + F.LABELS[2:5] + F.LABELS[1:2] + F.LABELS[5:])
  with pytest.raises(ValueError, match="ctc_labels"):
    dec.beam_search(h, lens, prev, lm=foreign)
  with pytest.raises(ValueError, match="ctc_labels"):
    small_decoder(F.LABELS_WIDE).beam_search(h, lens, prev, lm=az_lm)


def test_word_lm_checks_and_packs(az_lm, model_dir):
  from lipreading_amd import lm as LM
  from lipreading_amd.decoder import ctc_labels
  assert az_lm.labels == ctc_labels(F.char2idx(F.LABELS)) and az_lm.roles == LM.class_roles(F.LABELS, 0)
  assert (az_lm.alpha, az_lm.beta) == (0.5, 0.25) and az_lm.blob.dtype == np.uint8 and az_lm.blob.size > 128
  with pytest.raises(ValueError, match="' ' label"):
    LM.WordLM(F.arpa("az", 2), [l for l in F.LABELS if l != " "])
  with pytest.raises(ValueError, match="finite"):
    LM.WordLM(F.arpa("az", 2), F.LABELS, alpha=float("nan"))
  with pytest.raises(NotImplementedError):
    LM.WordLM(str(model_dir / "model.binary"), F.LABELS)


# ---- driver ---------------------------------------------------------------------------------------------------------
def test_driver_lm_flags_parse():
  from lipreading_amd import driver
  f = driver.parse_flags([])
  assert (f["attn_lm_path"], f["attn_lm_alpha"], f["attn_lm_beta"]) == ("", 0.0, 0.0)
  f = driver.parse_flags(["--attn_decode=beam", "--attn_lm_path=x.arpa", "--attn_lm_alpha=0.5", "--attn_lm_beta=-1"])
  assert (f["attn_lm_path"], f["attn_lm_alpha"], f["attn_lm_beta"]) == ("x.arpa", 0.5, -1.0)
  driver.parse_flags(["--attn_decode=joint", "--enable_ctc=True", "--attn_lm_path=x.arpa"])
  for bad in (["--attn_lm_path=x.arpa"], ["--attn_decode=teacher", "--attn_lm_path=x.arpa"]):
    with pytest.raises(SystemExit):
      driver.parse_flags(bad)
  with pytest.raises(SystemExit):
    driver.parse_flags(["--lm_path=x.arpa", "--attn_decode=beam"])   # the CTC decoder's check stays


@pytest.mark.parametrize("score", ["host", "device"])
def test_driver_error_of_passes_the_model_on(monkeypatch, model_dir, score):
  from lipreading_amd import driver, train
  from lipreading_amd.lm import WordLM
  calls = []
  monkeypatch.setattr(train, "attention_cer", lambda *a, **k: (calls.append(k), 0.25)[1])
  monkeypatch.setattr(train, "device_scores", lambda *a, **k: (calls.append(k), {"cer": 0.25})[1])
  f = driver.parse_flags(["--attn_decode=joint", "--enable_ctc=True", "--attn_ctc_weight=0.4", "--attn_beam_width=3",
                          "--attn_lm_path=" + F.arpa("az", 2), "--attn_lm_alpha=0.5", "--attn_lm_beta=0.25",
                          "--score=" + score])
  err = driver.make_error_of(f, None, object(), None, "cpu", F.char2idx(F.LABELS))
  assert err([]) == 0.25 and err([]) == 0.25
  assert len(calls) == 2 and calls[0]["lm"] is calls[1]["lm"]      # one WordLM for every call
  lm = calls[0].pop("lm")
  assert isinstance(lm, WordLM) and (lm.alpha, lm.beta, lm.labels) == (0.5, 0.25, F.LABELS)
  calls[0].pop("decoding_step", None)
  assert calls[0] == dict(beam_width=3, max_label_len=100, ctc_weight=0.4)


# ---- the GPU cases have margin and exercise the model ----------------------------------------------------------------
@pytest.mark.parametrize("case", F.CASES, ids=[c["id"] for c in F.CASES])
def test_gpu_case_has_margin_and_uses_the_model(case):
  """At most half of a case's utterances are near-ties of the restatement itself (the device test allows the
  project's 75 %), and in at least half the model changes the best hypothesis."""
  ref = F.reference(case["id"])
  odec, enc, lens, prev, y = F.inputs(case["id"])
  near = sum(1 for _, margin in ref if margin <= NEAR)
  plain = joint_ref(odec, enc, lens, prev, y, case["K"], F.LMAX, case["lam"], P=case["P"])
  moved = sum(1 for (fb, _), (pb, _) in zip(ref, plain) if fb and (not pb or fb[0][0] != pb[0][0]))
  print("near-tie utterances %d, best hypothesis changed in %d of %d" % (near, moved, F.B))
  assert near <= F.B // 2, near
  assert moved >= F.B // 2, moved
  assert all(EOS not in h[:-1] for beam, _ in ref for h, *_ in beam)
