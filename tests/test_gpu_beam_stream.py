"""GPU: resumable beam search sessions (lr_ctc_beam_stream_*, BeamCTCDecoder.stream) against the one-shot entries on
the same device, bit for bit, and once against the restatement stream_ref of tests/beam_stream_cases.py.

The one-shot entries are not code under test here: tests/test_gpu_beam.py, test_gpu_beam_lm.py and
test_gpu_beam_bias.py hold them to the float64 restatements.  Scores are compared as raw bits."""
import re
import warnings

import numpy as np
import pytest
import torch

from tests import beam_bias_cases as K
from tests import beam_stream_cases as S
from tests.test_beam_lm_cpu import TOY, Dict, RefLM, write_arpa

pytestmark = pytest.mark.gpu

B, T, C = S.B, S.T, S.C
VARIANTS = ["plain", "lm", "bias", "lm_bias"]
ALPHA, BETA = 0.8, 1.0


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "gpu tests need an MI355X"
  return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
  """The parity frames on the host and the device, and the two ARPA files."""
  d = tmp_path_factory.mktemp("stream")
  words = write_arpa(str(d / "words.arpa"), S.lm_sentences(), 2)
  toy = d / "toy.arpa"
  toy.write_text(TOY)
  p = S.parity_frames()
  return dict(p=p, pd=torch.tensor(p, device=dev), words=words, toy=str(toy), ref={})


def decoder(world, variant, W, n, **kw):
  from lipreading_amd.decoder import BeamCTCDecoder
  if variant in ("lm", "lm_bias", "toy"):
    kw.update(lm_path=world["toy" if variant == "toy" else "words"], alpha=ALPHA, beta=BETA)
  if variant in ("bias", "lm_bias"):
    kw.update(hotwords=S.HOT)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    return BeamCTCDecoder(S.LABELS, beam_width=W, cutoff_top_n=n, **kw)


def whole(x, cuts):
  """x (B, T, C) cut along the frames: [(view, None)]."""
  out, t = [], 0
  for c in cuts:
    out.append((x[:, t:t + c], None))
    t += c
  return out


def fed(dec, chunks, dev, max_frames=T, batch=B):
  st = dec.stream(batch, max_frames, dev)
  for x, sz in chunks:
    st.feed(x, sz)
  return st


def same_bits(got, want, what=""):
  """ids, offsets, lens equal and scores equal as raw bits."""
  for name, g, w in zip(("ids", "offsets", "lens"), got[:3], want[:3]):
    assert g.shape == w.shape and torch.equal(g, w), (what, name)
  assert torch.equal(w_bits(got[3]), w_bits(want[3])), (what, "scores")


def w_bits(x):
  return x.contiguous().view(torch.int32)


def sizes_t(v, dev):
  return torch.tensor(np.asarray(v, np.int32), device=dev)


# ---- 1. any chunking equals the one-shot search ----------------------------------------------------------------------
def check_all_chunkings(world, dev, dec, x=None, what=""):
  x = world["pd"] if x is None else x
  W = dec.beam_width
  want = dec.decode_ids(x)
  for name, cuts in S.CHUNKINGS.items():
    st = fed(dec, whole(x, cuts), dev)
    got = st.read_ids(W, T)
    same_bits(got, want, (what, name))
    assert got[5].tolist() == [T] * B and got[6].tolist() == [0] * B
  ragged = [(torch.tensor(a, device=dev), sizes_t(s, dev)) for a, s in S.ragged_chunks(x.cpu().numpy())]
  got = fed(dec, ragged, dev).read_ids(W, T)
  same_bits(got, dec.decode_ids(x, sizes_t(S.RAGGED_TOTALS, dev)), (what, "ragged"))
  assert got[5].tolist() == S.RAGGED_TOTALS and got[6].tolist() == [0] * B
  return want


@pytest.mark.parametrize("W,n", [(1, 1), (4, 4), (16, 8), (128, 64)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_any_chunking_equals_the_one_shot_search(dev, world, variant, W, n):
  want = check_all_chunkings(world, dev, decoder(world, variant, W, n), what=(variant, W, n))
  if W >= 16:   # the inputs exercise the search: more than one live hypothesis, non-empty transcripts
    assert int((want[2][:, 1] > 0).sum()) >= B // 2 and int((want[2][:, 0] > 3).sum()) >= B // 2


@pytest.mark.parametrize("variant,kw", [
    ("plain", dict(cutoff_prob=0.95)), ("lm_bias", dict(cutoff_prob=0.95)), ("plain", dict(log_probs_input=True)),
    ("lm_bias", dict(log_probs_input=True)), ("toy", {})])
def test_chunking_with_cutoff_prob_log_input_and_the_toy_model(dev, world, variant, kw):
  """cutoff_prob < 1 and log-probabilities at (16, 8); under the toy model's three-word dictionary most hypotheses
  die, so the live count shrinks in mid-stream."""
  x = world["pd"].log() if kw.get("log_probs_input") else world["pd"]
  check_all_chunkings(world, dev, decoder(world, variant, 16, 8, **kw), x, what=(variant, kw))


def test_chunking_with_another_blank_index(dev, world):
  from lipreading_amd.decoder import BeamCTCDecoder
  perm = list(range(C))
  perm[0], perm[C - 1] = C - 1, 0          # the blank's column goes last, <EOS>'s first
  labels = [S.LABELS[i] for i in perm]
  dec = BeamCTCDecoder(labels, beam_width=16, cutoff_top_n=8, blank_index=C - 1)
  want = check_all_chunkings(world, dev, dec, world["pd"][:, :, perm].contiguous(), what="blank")
  plain = decoder(world, "plain", 16, 8).decode_ids(world["pd"])
  assert torch.equal(want[2], plain[2]) and torch.equal(want[1], plain[1])   # the same search, columns renamed


# ---- 2. a read in mid-stream ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_read_in_mid_stream_equals_the_one_shot_search_on_the_frames_so_far(dev, world, variant):
  dec = decoder(world, variant, 16, 8)
  st = dec.stream(B, T, dev)
  t = 0
  for x, _ in whole(world["pd"], S.CHUNKINGS["mixed"]):
    st.feed(x)
    t += x.shape[1]
    got = st.read_ids(16, T)
    same_bits(got, dec.decode_ids(world["pd"], sizes_t([t] * B, dev)), (variant, t))
    assert got[5].tolist() == [t] * B
    # stable is the common prefix of the hypotheses the read itself returns
    ids, lens = got[0].cpu().tolist(), got[2].cpu().tolist()
    sc = got[3].cpu().tolist()
    for b in range(B):
      live = [tuple(ids[b][r][:lens[b][r]]) for r in range(16) if sc[b][r] != float("inf")]
      assert int(got[4][b]) == S.common_prefix(live), (variant, t, b)


@pytest.mark.parametrize("variant", ["plain", "lm_bias"])
def test_reads_against_the_restatement(dev, world, variant):
  """tests/test_gpu_beam.py's agreement rules at every chunk border: top-1 ids and offsets identical where the
  restatement's rank-1/rank-2 margin exceeds 1e-3, shared strings' scores within 2e-4 (+ 1e-6 relative with the
  language model); stable identical wherever the device holds the restatement's set of strings."""
  from lipreading_amd.lm import read_arpa
  W, n = 16, 8
  kw, rel = {}, 0.0
  if variant == "lm_bias":
    lm = RefLM(read_arpa(world["words"]))
    kw, rel = dict(lm=lm, dic=Dict(lm, S.LABELS), alpha=ALPHA, beta=BETA, bias=K.Bias(S.hot_phrases(), 1)), 1e-6
  cuts = [c for c in S.CHUNKINGS["mixed"] if c]
  want = [S.stream_ref(world["p"][b], cuts, W, n, **kw) for b in range(B)]
  dec = decoder(world, variant, W, n)
  st = dec.stream(B, T, dev)
  top = sets = 0
  for k, (x, _) in enumerate(whole(world["pd"], cuts)):
    st.feed(x)
    ids, off, lens, sc, stable, frames, _ = (g.cpu().tolist() for g in st.read_ids(W, T))
    for b in range(B):
      t, ref, ref_stable = want[b][k]
      assert frames[b] == t
      got = [(tuple(ids[b][r][:lens[b][r]]), tuple(off[b][r][:lens[b][r]]), sc[b][r]) for r in range(W)
             if sc[b][r] != float("inf")]
      assert len(got) == len(ref), (b, t)
      if (ref[1][2] - ref[0][2] if len(ref) > 1 else np.inf) > 1e-3:
        assert got[0][:2] == ref[0][:2], (b, t)
        top += 1
      by_ids = {r[0]: r[2] for r in ref}
      for g in got:
        if g[0] in by_ids:
          assert abs(g[2] - by_ids[g[0]]) < 2e-4 + rel * abs(by_ids[g[0]]), (b, t, g)
      if {g[0] for g in got} == set(by_ids):
        assert stable[b] == ref_stable, (b, t)
        sets += 1
  assert top >= B * len(cuts) // 2 and sets >= B * len(cuts) // 2, (top, sets)
  assert sum(want[b][-1][2] >= 1 for b in range(B)) >= B // 2   # and there is a stable prefix to agree on


# ---- 3. reads change nothing, feeds are deterministic -----------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "lm_bias"])
def test_read_is_non_destructive_and_feed_is_deterministic(dev, world, variant):
  dec = decoder(world, variant, 16, 8)
  chunks = whole(world["pd"], S.CHUNKINGS["mixed"])
  quiet = fed(dec, chunks, dev)
  again = fed(dec, chunks, dev)
  assert torch.equal(quiet.state, again.state)
  read = dec.stream(B, T, dev)
  for x, _ in chunks:
    read.feed(x)
    before = read.state.clone()
    a, b = read.read_ids(16, T), read.read_ids(16, T)
    assert all(torch.equal(w_bits(u), w_bits(v)) for u, v in zip(a, b))
    assert torch.equal(read.state, before)
    read.partial()
  assert torch.equal(read.state, quiet.state)


# ---- 4. slots are independent -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "lm_bias"])
def test_a_masked_reset_restarts_those_slots_only(dev, world, variant):
  dec = decoder(world, variant, 16, 8)
  pd = world["pd"]
  mask = [1, 0, 1, 0, 0, 1]
  st = fed(dec, [(pd[:, :13], None)], dev)
  st.reset(sizes_t(mask, dev))
  st.feed(pd[:, 13:])
  got = st.read_ids(16, T)
  full = dec.decode_ids(pd)
  tail = dec.decode_ids(pd[:, 13:])     # offsets count from the reset
  for b in range(B):
    if mask[b]:
      assert int(got[5][b]) == T - 13
      assert torch.equal(got[0][b, :, :T - 13], tail[0][b]) and torch.equal(got[1][b, :, :T - 13], tail[1][b])
      assert bool((got[0][b, :, T - 13:] == -1).all()) and bool((got[1][b, :, T - 13:] == -1).all())
      assert torch.equal(got[2][b], tail[2][b]) and torch.equal(w_bits(got[3][b]), w_bits(tail[3][b]))
    else:
      assert int(got[5][b]) == T
      same_bits([g[b] for g in got[:4]], [f[b] for f in full], b)
  # a bool mask and None (all slots)
  st.reset(torch.tensor(mask, device=dev) > 0)
  assert st.read_ids(1, 1)[5].tolist() == [0 if m else T for m in mask]
  st.reset()
  got = st.read_ids(2, 4)
  assert got[5].tolist() == [0] * B and got[2].tolist() == [[0, 0]] * B and got[4].tolist() == [0] * B
  assert got[3][:, 0].tolist() == [0.0] * B and bool(torch.isinf(got[3][:, 1]).all())


def test_permuting_the_batch_permutes_the_results(dev, world):
  dec = decoder(world, "lm_bias", 16, 8)
  perm = [3, 5, 0, 4, 1, 2]
  a = fed(dec, whole(world["pd"], S.CHUNKINGS["mixed"]), dev).read_ids(16, T)
  b = fed(dec, whole(world["pd"][perm].contiguous(), S.CHUNKINGS["mixed"]), dev).read_ids(16, T)
  assert all(torch.equal(w_bits(u[perm]), w_bits(v)) for u, v in zip(a, b))


# ---- 5. views and widths ----------------------------------------------------------------------------------------------
def test_views_equal_contiguous_copies(dev, world):
  dec = decoder(world, "plain", 16, 8)
  pd = world["pd"]
  cuts = S.CHUNKINGS["mixed"]
  views = fed(dec, whole(pd, cuts), dev)
  copies = fed(dec, [(x.contiguous().clone(), s) for x, s in whole(pd, cuts)], dev)
  tb = pd.transpose(0, 1).contiguous().transpose(0, 1)      # (T, B, C) memory seen as (B, T, C)
  assert not tb.is_contiguous()
  strided = fed(dec, whole(tb, cuts), dev)
  assert torch.equal(views.state, copies.state) and torch.equal(views.state, strided.state)


def test_a_narrow_read_keeps_true_lengths_and_stays_in_its_rows(dev, world):
  dec = decoder(world, "plain", 16, 8)
  st = fed(dec, whole(world["pd"], [T]), dev)
  full = st.read_ids(8, T)
  G, n_out, width = 64, 8, 3
  guard = 0x5a5a5a5a
  sizes = [B * n_out * width, B * n_out * width, B * n_out, B * n_out, B, B, B]
  bufs = [torch.full((G + s + G,), guard, dtype=torch.int32, device=dev) for s in sizes]
  outs = [buf[G:G + s] for buf, s in zip(bufs, sizes)]
  ids, off = outs[0].view(B, n_out, width), outs[1].view(B, n_out, width)
  lens, scores = outs[2].view(B, n_out), outs[3].view(torch.float32).view(B, n_out)
  st._read_into(n_out, width, ids, off, lens, scores, outs[4], outs[5], outs[6])
  torch.cuda.synchronize()
  for buf, s in zip(bufs, sizes):
    assert bool((buf[:G] == guard).all()) and bool((buf[G + s:] == guard).all())
  assert torch.equal(lens, full[2]) and int(lens.max()) > width      # the true lengths
  assert torch.equal(ids, full[0][:, :, :width]) and torch.equal(off, full[1][:, :, :width])
  assert torch.equal(w_bits(scores), w_bits(full[3]))
  assert torch.equal(outs[4], full[4]) and outs[5].tolist() == [T] * B and outs[6].tolist() == [0] * B


# ---- 6. traps ---------------------------------------------------------------------------------------------------------
def test_overflow_and_mismatch_set_their_bits_and_nothing_else(dev, world):
  from lipreading_amd import _C
  pd = world["pd"]
  dec = decoder(world, "lm_bias", 16, 8)
  # frames past max_frames are not consumed
  st = fed(dec, whole(pd, [20, 20]), dev, max_frames=25)
  got = st.read_ids(16, 25)
  assert got[5].tolist() == [25] * B and got[6].tolist() == [_C.LR_BEAM_STREAM_OVERFLOW] * B
  want = dec.decode_ids(pd, sizes_t([25] * B, dev))
  same_bits(got, [want[0][:, :, :25], want[1][:, :, :25], want[2], want[3]], "overflow")
  assert bool((want[0][:, :, 25:] == -1).all())
  with pytest.raises(_C.LipReadingHipError, match="slot 0.*overflow"):
    st.partial()
  with pytest.raises(_C.LipReadingHipError, match="overflow"):
    st.result()
  # an advance with another beam width, then with another variant: the session's own arguments swapped for the call
  st = fed(dec, whole(pd, [20]), dev)
  before = st.state.clone()
  status_words = [b * 8 + 7 for b in range(B)]
  for other in (decoder(world, "lm_bias", 8, 8), decoder(world, "plain", 16, 8)):
    wrong = dec.stream(B, T, dev)
    wrong.state = st.state
    wrong.decoder = other
    if other._word_lm is None:
      wrong._lm = wrong._bias = False
      wrong._blob = wrong._roles = wrong._biasblob = None
    wrong.feed(pd[:, 20:])
    after = st.state.clone()
    words = after.view(torch.int32)
    assert words[status_words].tolist() == [_C.LR_BEAM_STREAM_MISMATCH] * B
    words[status_words] = 0
    assert torch.equal(after, before)
  assert st.read_ids(1, 1)[5].tolist() == [20] * B
  with pytest.raises(_C.LipReadingHipError, match="slot 0.*mismatch"):
    st.partial()
  st.reset()
  assert st.partial() == [("", 0)] * B


def test_feed_rejects_on_the_host(dev, world):
  from lipreading_amd import _C
  st = decoder(world, "plain", 16, 8).stream(B, T, dev)
  before = st.state.clone()
  with pytest.raises(_C.LipReadingHipError, match="no CPU fallback"):
    st.feed(torch.zeros(B, 5, C))
  with pytest.raises(ValueError, match="utterances"):
    st.feed(world["pd"][:4, :5])
  with pytest.raises(ValueError, match="classes"):
    st.feed(world["pd"][:, :5, :C - 1])
  with pytest.raises(KeyError):
    st.feed(torch.zeros(B, 5, C + 1, device=dev))
  with pytest.raises(ValueError, match="sizes"):
    st.feed(world["pd"][:, :5], sizes_t([5] * (B - 1), dev))
  with pytest.raises(ValueError, match="n_out"):
    st.read_ids(17)
  assert torch.equal(st.state, before)


# ---- 7. the front door ------------------------------------------------------------------------------------------------
def test_result_equals_decode_and_partial_strings_are_final(dev, world):
  dec = decoder(world, "lm_bias", 16, 8)
  st = dec.stream(B, T, dev)
  partials = []
  for x, _ in whole(world["pd"], [5] * 8):
    partials.append(st.feed(x).partial())
  strings, offsets = st.result()
  want_s, want_o = dec.decode(world["pd"])
  assert strings == want_s
  assert all(a.dtype == b.dtype and torch.equal(a, b) for u, v in zip(offsets, want_o) for a, b in zip(u, v))
  assert [len(u) for u in offsets] == [len(v) for v in want_o]
  for k, row in enumerate(partials):
    for b, (text, final) in enumerate(row):
      assert 0 <= final <= len(text)
      assert all(later[b][0].startswith(text[:final]) for later in partials[k:]), (k, b)
      assert strings[b][0].startswith(text[:final])
  assert [p[0] for p in partials[-1]] == [s[0] for s in strings]
  assert sum(final > 0 for _, final in partials[-1]) >= B // 2
  assert sum(s[0] == t for s, t in zip(strings, S.TEXTS)) >= B // 2   # and the search reads the clean frames


# ---- 8. the driver ----------------------------------------------------------------------------------------------------
def test_driver_evaluation_in_chunks_reports_the_same_errors_and_the_commit_delay(dev, tmp_path, capsys):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=10, captions_per_video=6, seed=7)
  common = ["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True", "--ctc_only=True",
            "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=0", "--ctc_decoder=beam", "--beam_width=8"]
  seen = {}
  for name, extra in (("one_shot", []), ("chunks", ["--stream_chunk=5"])):
    for score in ("host", "device"):
      f = driver.parse_flags(common + extra + ["--score=" + score])
      capsys.readouterr()
      out = driver.run(**f)
      text = capsys.readouterr().out
      cer = float(re.search(r"\tCER:\s+(\S+)", text).group(1))
      # the same encoder and loader through the driver's own error measure, for the WER of the device's scores
      from lipreading_amd.decoder import BeamCTCDecoder, ChunkedBeamDecoder, ctc_labels
      beam = BeamCTCDecoder(ctc_labels(out["char2idx"]), beam_width=8, log_probs_input=True)
      error_of = driver.make_error_of(f, out["encoder"], None, ChunkedBeamDecoder(beam, 5) if extra else beam, dev,
                                      out["char2idx"])
      assert error_of(out["loaders"][1]) == cer
      seen[(name, score)] = (cer, error_of.last_scores["wer"] if score == "device" else None)
      line = re.search(r"Commit delay \(chunks of 5 frames\): mean (\S+) frames, p90 (\d+), (\S+)% of (\d+) characters",
                       text)
      assert (line is not None) == bool(extra), text
      if extra:
        assert out["commit_delay"]["chars"] == int(line.group(4)) > 0
        assert 0 <= out["commit_delay"]["mean"] <= 200 and 0.0 <= out["commit_delay"]["end_share"] <= 1.0
      else:
        assert "commit_delay" not in out
  assert seen[("one_shot", "host")] == seen[("chunks", "host")]
  assert seen[("one_shot", "device")] == seen[("chunks", "device")]
  assert seen[("one_shot", "host")][0] == seen[("one_shot", "device")][0] and seen[("chunks", "device")][1] >= 0.0
