"""Chunk-limited attention and transformer sessions, the parts that need no device: the theorem the
session rests on — the chunk-masked one-shot encoder equals the same layers fed chunk by chunk from a key / value cache —
in float64, the count rule, the driver's flags and the constructors' refusals."""
import pytest
import torch

from tests import tfm_stream_cases as S


@pytest.fixture(scope="module")
def refs():
  return {name: S.make_ref(S.FRAME_DIM, dm, nh, S.LAYERS, S.FF, seed=3).double() for name, (dm, nh) in S.MODELS.items()}


@pytest.mark.parametrize("Lc", S.LEFTS)
@pytest.mark.parametrize("C", S.CHUNKS)
@pytest.mark.parametrize("T", S.LENGTHS)
@pytest.mark.parametrize("model", sorted(S.MODELS))
def test_the_cached_stream_is_the_masked_encoder_in_float64(refs, model, T, C, Lc):
  """stream_ref == masked_ref to 1e-12 of the tensor's largest entry on rows < len, for every feeding plan: the session
  only ever computes whole chunks, a chunk sees only its window, and the window's keys and values do not change once
  their chunk is complete."""
  ref = refs[model]
  lens = S.ragged_lens(T, C)
  g = torch.Generator().manual_seed(T * 100 + C * 10 + Lc)
  x = torch.randn(len(lens), T, S.FRAME_DIM, generator=g, dtype=torch.float64)
  with torch.no_grad():
    lp_m, h_m = S.masked_ref(ref, x, lens, C, Lc)
  assert torch.isfinite(h_m).all()
  for b, n in enumerate(lens):
    for name, pieces in S.plans(n, C).items():
      lp_s, h_s, counts = S.stream_ref(ref, x[b, :n], pieces, C, Lc)
      assert sum(counts) == n and lp_s.shape[0] == n, (name, counts)
      if n == 0:
        continue
      for got, want in ((lp_s, lp_m[b, :n]), (h_s, h_m[b, :n])):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (model, T, C, Lc, b, name)


def test_a_full_attention_model_is_not_what_a_cache_computes(refs):
  """The reason the mask exists: without it (C = 0 in the one-shot model) the chunk-by-chunk evaluation is another
  function."""
  ref = refs["d64"]
  x = torch.randn(1, 21, S.FRAME_DIM, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
  with torch.no_grad():
    _, h_full = S.masked_ref(ref, x, [21], 0, 0)
  _, h_s, _ = S.stream_ref(ref, x[0], [21], 5, 1)
  assert float((h_s - h_full[0]).abs().max()) > 1e-3 * float(h_full.abs().max())


def test_counts_follow_the_rule_on_random_plans(refs):
  from lipreading_amd.transformer_stream import count_rule
  ref = refs["d64"]
  g = torch.Generator().manual_seed(11)
  for trial in range(40):
    C = int(torch.randint(1, 33, (1,), generator=g))
    n = int(torch.randint(0, 60, (1,), generator=g))
    pieces, left = [], n
    while left > 0:
      k = min(left, int(torch.randint(0, 2 * C + 2, (1,), generator=g)))
      pieces.append(k)
      left -= k
    x = torch.randn(n, S.FRAME_DIM, generator=g, dtype=torch.float64)
    _, _, counts = S.stream_ref(ref, x, pieces, C, 1)
    seen = 0
    for i, (k, c) in enumerate(zip(pieces or [0], counts)):
      ended = i == len(pieces or [0]) - 1
      assert c == count_rule(seen + k, ended, C) - count_rule(seen, False, C), (trial, i)
      assert count_rule(seen + k, ended, C) == S.count_rule(seen + k, ended, C)
      seen += k
    assert sum(counts) == n


def test_batch_plan_ends_every_slot_once():
  adv = S.batch_plan([[3, 2], [5], [1, 1, 1]])
  assert adv == [([3, 5, 1], [0, 1, 0]), ([2, 0, 1], [1, 0, 0]), ([0, 0, 1], [0, 0, 1])]


# ---- the driver's flags ------------------------------------------------------------------------------------------------

def test_driver_flag_defaults_change_nothing():
  from lipreading_amd import driver
  new = {"tfm_chunk": 0, "tfm_left_chunks": 0, "stream_tfm": False}
  for k, v in new.items():
    assert driver.DEFAULTS[k] == v and type(driver.DEFAULTS[k]) is type(v)
  parsed = driver.parse_flags([])
  assert parsed == driver.DEFAULTS
  assert {k: v for k, v in parsed.items() if k not in new} == {k: v for k, v in driver.DEFAULTS.items() if k not in new}
  for argv in (["--encoder=transformer"], ["--frontend=conv3d", "--encoder=transformer"]):
    got = driver.parse_flags(argv)
    assert (got["tfm_chunk"], got["tfm_left_chunks"], got["stream_tfm"]) == (0, 0, False)


def test_driver_flags_parse():
  from lipreading_amd import driver
  f = driver.parse_flags(["--encoder=transformer", "--tfm_chunk=8", "--tfm_left_chunks=3"])
  assert (f["tfm_chunk"], f["tfm_left_chunks"], f["stream_tfm"]) == (8, 3, False)
  f = driver.parse_flags(["--encoder=transformer", "--tfm_chunk=8", "--stream_tfm=True", "--stream_chunk=5",
                          "--ctc_decoder=beam"])
  assert f["stream_tfm"] is True
  f = driver.parse_flags(["--frontend=conv3d", "--encoder=transformer", "--tfm_chunk=4", "--stream_tfm=True",
                          "--stream_chunk=5", "--ctc_decoder=beam"])
  assert f["stream_tfm"] is True and f["frontend"] == "conv3d"


@pytest.mark.parametrize("argv,needle", [
    (["--tfm_chunk=8"], "--tfm_chunk needs --encoder=transformer"),
    (["--tfm_left_chunks=2"], "--tfm_left_chunks needs --encoder=transformer"),
    (["--encoder=transformer", "--tfm_left_chunks=2"], "--tfm_left_chunks needs --tfm_chunk>0"),
    (["--encoder=transformer", "--tfm_chunk=-1"], "--tfm_chunk must be >= 0"),
    (["--encoder=transformer", "--tfm_chunk=4", "--tfm_left_chunks=-1"], "--tfm_left_chunks must be >= 0"),
    (["--stream_tfm=True"], "--stream_tfm needs --encoder=transformer"),
    (["--encoder=transformer", "--stream_tfm=True", "--stream_chunk=5", "--ctc_decoder=beam"],
     "--stream_tfm needs --tfm_chunk>0"),
    (["--encoder=transformer", "--tfm_chunk=8", "--stream_tfm=True"], "--stream_tfm needs --stream_chunk>0"),
    (["--encoder=transformer", "--tfm_chunk=8", "--stream_tfm=True", "--stream_chunk=5", "--ctc_decoder=beam",
      "--stream_encoder=True", "--bidirectional=False"], "--stream_encoder needs --encoder=rnn and --frontend=none"),
    (["--frontend=conv3d", "--encoder=transformer", "--tfm_chunk=8", "--stream_frontend=True", "--stream_chunk=5",
      "--ctc_decoder=beam"], "there is no session for the transformer encoder"),
])
def test_driver_flag_refusals(argv, needle):
  from lipreading_amd import driver
  with pytest.raises(SystemExit) as e:
    driver.parse_flags(argv)
  assert needle in str(e.value)


def test_stream_tfm_needs_the_beam_decoder():
  from lipreading_amd import driver
  with pytest.raises(SystemExit) as e:
    driver.tfm_chunk_check(dict(driver.DEFAULTS, encoder="transformer", tfm_chunk=8, stream_tfm=True, stream_chunk=5))
  assert "--stream_tfm needs --ctc_decoder=beam" in str(e.value)
  driver.tfm_chunk_check(dict(driver.DEFAULTS))   # off: nothing to check


# ---- constructors ------------------------------------------------------------------------------------------------------

def _encoder(**kw):
  from lipreading_amd.data import default_char2idx
  from lipreading_amd.transformer import TransformerVideoEncoder
  return TransformerVideoEncoder(12, d_model=16, nhead=2, num_layers=1, dim_feedforward=32, enable_ctc=True,
                                 vocab_size=S.VOCAB, char2idx=default_char2idx(), **kw)


def test_encoder_keeps_the_chunk_as_plain_attributes():
  plain, chunked = _encoder(), _encoder(attn_chunk=8, attn_left_chunks=3)
  assert (plain.attn_chunk, plain.attn_left_chunks) == (0, 0)
  assert (chunked.attn_chunk, chunked.attn_left_chunks) == (8, 3)
  assert list(plain.state_dict()) == list(chunked.state_dict())   # not in the state_dict: checkpoints interchange
  for kw in (dict(attn_chunk=-1), dict(attn_chunk=4, attn_left_chunks=-2)):
    with pytest.raises(ValueError, match="must be >= 0"):
      _encoder(**kw)


def test_a_session_refuses_what_it_cannot_run():
  from lipreading_amd import _C
  from lipreading_amd.transformer_stream import (ChunkedTransformerEncoder, TransformerLiveTranscriber,
                                                 TransformerStream)
  full, chunked = _encoder(), _encoder(attn_chunk=4, attn_left_chunks=1)
  for make in (lambda: TransformerStream(full, 2, "cuda"), lambda: full.stream(2, "cuda"),
               lambda: ChunkedTransformerEncoder(full, 5),
               lambda: TransformerLiveTranscriber(full, object(), 2, 50, "cuda")):
    with pytest.raises(ValueError, match="a full-attention model cannot be cached"):
      make()
  with pytest.raises(TypeError, match="TransformerVideoEncoder"):
    TransformerStream(torch.nn.Linear(2, 2), 2, "cuda")
  with pytest.raises(_C.LipReadingHipError, match="no CPU fallback"):
    TransformerStream(chunked, 2, "cpu")
  with pytest.raises(ValueError, match="batch must be >= 1"):
    TransformerStream(chunked, 0, "cuda")
  with pytest.raises(ValueError, match="chunk must be >= 1"):
    ChunkedTransformerEncoder(chunked, 0)

  class Probs(object):
    log_probs_input = False
  with pytest.raises(ValueError, match="log-probabilities"):
    TransformerLiveTranscriber(chunked, Probs(), 2, 50, "cuda")
  with pytest.raises(ValueError, match="height and width go with a PixelLipReader"):
    Probs.log_probs_input = True
    TransformerLiveTranscriber(chunked, Probs(), 2, 50, "cuda", height=32, width=32)
