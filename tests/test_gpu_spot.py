"""GPU: lr_ctc_spot / spot.KeywordSpotter against the float32 restatement of tests/spot_cases.py — every comparison
with it is `==`, on all outputs, with the end trace —, on planted clips, against the greedy decoder, on strided layouts
and bad inputs, and through train.spot_loader and the driver's --spot."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

from lipreading_amd import _C
from lipreading_amd.data import default_char2idx
from lipreading_amd.decoder import ctc_labels
from tests import spot_cases as S

pytestmark = pytest.mark.gpu

LABELS = ctc_labels(default_char2idx())     # 65 classes, blank at 0; classes 5.. are single characters
C = len(LABELS)
FIRST_CHAR = 5
OUTPUTS = ("hit_score", "hit_start", "hit_end", "n_hits", "status", "end_score", "end_start")
HIT_OUTPUTS = OUTPUTS[:5]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda")


def plan(B, T, K, W, H=4, classes=C):
  p = (ctypes.c_int32 * 11)()
  assert _C.lib().lr_ctc_spot_plan(B, T, classes, K, W, H, ctypes.addressof(p)) == 0
  names = ("segment", "threads", "side_by_side", "groups", "rows_in_lds", "trace_at", "lds_bytes", "per_workgroup",
           "len16", "len32", "workgroups")
  return dict(zip(names, list(p)))


def raw_spot(dev, lp, sizes, kw, lens, thr=None, H=4, trace=True, guard=0):
  """The entry point itself, keywords in the caller's order: dict of host arrays (without the trace when trace=False).
  guard > 0: every output buffer has that many guard words either side, checked untouched.  The workspace is NULL
  wherever the header says it is not needed: with the caller's trace, and with the trace in LDS."""
  lib = _C.lib()
  B, T, classes = lp.shape
  K, W = kw.shape
  d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  lp_d, sz_d, kw_d, ln_d, th_d = d(lp), d(sizes), d(kw), d(lens), d(thr)
  shapes = dict(hit_score=(B, K, H), hit_start=(B, K, H), hit_end=(B, K, H), n_hits=(B, K), status=(B, K))
  if trace:
    shapes.update(end_score=(B, K, T), end_start=(B, K, T))
  bufs = {}
  for k, shp in shapes.items():
    dt = torch.float32 if k.endswith("score") else torch.int32
    bufs[k] = torch.full((int(np.prod(shp)) + 2 * guard,), 12345, dtype=dt, device=dev)
  ptr = lambda k: bufs[k].data_ptr() + 4 * guard if k in bufs else None
  nbytes = lib.lr_ctc_spot_workspace_bytes(B, T, classes, K, W, H)
  assert nbytes > 0
  ws = None if trace or nbytes == 16 else torch.empty(nbytes, dtype=torch.uint8, device=dev)
  _C.check(lib.lr_ctc_spot(lp_d.data_ptr(), T * classes, classes, _C.ptr(sz_d), kw_d.data_ptr(), W, ln_d.data_ptr(),
                           _C.ptr(th_d), 0, H, *[ptr(k) for k in OUTPUTS], _C.ptr(ws), nbytes if ws is not None else 0, B, T,
                           classes, K,
                           _C.stream_handle()), "lr_ctc_spot")
  got = {}
  for k, shp in shapes.items():
    host = bufs[k].cpu().numpy()
    if guard:
      assert (host[:guard] == 12345).all() and (host[-guard:] == 12345).all(), k
      host = host[guard:-guard]
    got[k] = host.reshape(shp)
  return got


def assert_equal(got, want, what="", keys=OUTPUTS):
  for k in keys:
    assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
    bad = np.argwhere(got[k] != want[k])
    assert bad.size == 0, (what, k, bad[:5].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def clips(rng, T, classes=C, ragged=True):
  """One clip per value family and a ragged twin of it: lp (6, T, classes), sizes (6,)."""
  lps, sizes = [], []
  for _, family in S.FAMILIES:
    for short in (False, True):
      lps.append(family(rng, (T, classes)))
      sizes.append(int(rng.randint(1, T + 1)) if short and ragged else T)
  return np.stack(lps), np.array(sizes, np.int32)


def check_both_ways(dev, lp, sizes, kw, lens, thr=None, H=4, what=""):
  """With the trace (every output) and without (the hits: the trace then lives in LDS or the workspace)."""
  want = S.expected(lp, sizes, kw, lens, 0, thr, H)
  assert_equal(raw_spot(dev, lp, sizes, kw, lens, thr, H, trace=True), want, what)
  assert_equal(raw_spot(dev, lp, sizes, kw, lens, thr, H, trace=False), want, what, HIT_OUTPUTS)
  return want


# ---- 1: crossed shapes --------------------------------------------------------------------------------------------
ALL_LENS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32)


@pytest.mark.parametrize("T", (1, 2, 16, 17, 33, 75, 76))
def test_crossed_shapes_equal_the_restatement(dev, T):
  """Every keyword length, plain and doubled, in ONE call and in an order that mixes the segment widths inside a wave's
  slot of four; the three value families; ragged sizes; junk ids past the lengths.  Integer values put ties
  everywhere."""
  rng = np.random.RandomState(1000 + T)
  lp, sizes = clips(rng, T)
  lens = [L for L in ALL_LENS for _ in range(2)]
  order = rng.permutation(len(lens))
  kw, ln = S.keyword_batch(rng, [lens[i] for i in order], C, 0, stride=32)
  want = check_both_ways(dev, lp, sizes, kw, ln, what=T)
  finite = int(np.isfinite(want["end_score"]).sum())
  print("T=%d: %d pairs, %d finite trace cells, %d hits" % (T, want["status"].size, finite, int(want["n_hits"].sum())))
  assert (want["status"] == 0).all() and finite > 0
  # the same keywords sorted by length (what spot.py hands over): the same answers, keyword by keyword
  by_len = np.argsort(ln, kind="stable")
  again = raw_spot(dev, lp, sizes, kw[by_len], ln[by_len])
  for k in OUTPUTS:
    assert np.array_equal(again[k], want[k][:, by_len]), k


@pytest.mark.parametrize("K", ("1", "3", "capacity+1", "3*capacity+5"))
def test_keyword_counts_around_a_workgroup(dev, K):
  """K = 1, 3, one past what a workgroup serves (a second workgroup with one keyword), and four workgroups per sample
  with the last one's slots partly filled."""
  B, T = 6, 33
  per = plan(B, T, 17, 10)["per_workgroup"]
  if K == "capacity+1":
    K = per + 1
    assert plan(B, T, K, 10)["workgroups"] == 2 * B
  elif K == "3*capacity+5":
    K = 3 * per + 5
    assert plan(B, T, K, 10)["workgroups"] == 4 * B
  else:
    K = int(K)
  rng = np.random.RandomState(K)
  lp, sizes = clips(rng, T, classes=9)
  kw, ln = S.keyword_batch(rng, [int(rng.randint(1, 11)) for _ in range(K)], 9, 0, stride=10)
  check_both_ways(dev, lp, sizes, kw, ln, what=K)


def test_packing_boundaries_and_neighbours(dev):
  """At each boundary the plan reports: the last length of the narrower segment and the first of the wider one, each
  alone in its call and packed with neighbours of its own segment width — the outputs of the keyword are equal, and
  equal to the restatement."""
  p = plan(1, 40, 1, 32)
  assert (p["len16"], p["len32"]) == (8, 16)
  assert plan(1, 40, 1, p["len16"])["segment"] == 16 and plan(1, 40, 1, p["len16"] + 1)["segment"] == 32
  assert plan(1, 40, 1, p["len32"])["segment"] == 32 and plan(1, 40, 1, p["len32"] + 1)["segment"] == 64
  rng = np.random.RandomState(77)
  lp, sizes = clips(rng, 40)
  for L in (p["len16"], p["len16"] + 1, p["len32"], p["len32"] + 1):
    for doubled in (1, 2):
      kw, ln = S.keyword_batch(rng, [L] * 4, C, 0, stride=32, doubled_every=doubled)
      packed = check_both_ways(dev, lp, sizes, kw, ln, what=("packed", L))
      assert np.isfinite(packed["end_score"]).any()
      for i in range(4):
        alone = raw_spot(dev, lp, sizes, kw[i:i + 1], ln[i:i + 1])
        for k in OUTPUTS:
          assert np.array_equal(alone[k][:, 0], packed[k][:, i]), (L, i, k)
      # a shorter and a longer neighbour in the same slot
      mixed_kw, mixed_ln = kw.copy(), ln.copy()
      mixed_ln[0], mixed_ln[2] = 1, min(L + 7, 32)
      mixed_kw[2, :mixed_ln[2]] = S.random_target(rng, int(mixed_ln[2]), C, 0)
      mixed = raw_spot(dev, lp, sizes, mixed_kw, mixed_ln)
      for k in OUTPUTS:
        assert np.array_equal(mixed[k][:, [1, 3]], packed[k][:, [1, 3]]), (L, k)


# ---- 2: placement -------------------------------------------------------------------------------------------------
def threshold(key, B, K, W):
  """The first T at which the plan's `key` changes from its value at T = 1."""
  first = plan(B, 1, K, W)[key]
  for T in range(2, S.MAX_T + 1):
    if plan(B, T, K, W)[key] != first:
      return T
  return None


def placed_case(T, seed, W=12):
  rng = np.random.RandomState(seed)
  lp = np.stack([S.quantised(rng, (T, C)), S.integers(rng, (T, C))])
  sizes = np.array([T, max(T - 7, 1)], np.int32)
  kw, ln = S.keyword_batch(rng, [W, 3, 1, min(9, W), max(W - 1, 1)], C, 0, stride=W)
  return lp, sizes, kw, ln


@pytest.mark.parametrize("where", ("rows_lds_last", "rows_global_first", "trace_lds_last", "trace_ws_first"))
def test_each_side_of_the_placement_thresholds(dev, where):
  lib = _C.lib()
  t_rows, t_trace = threshold("rows_in_lds", 2, 5, 12), threshold("trace_at", 2, 5, 12)
  assert t_rows is not None and t_trace is not None and 1 < t_trace < t_rows
  assert plan(2, t_rows - 1, 5, 12)["rows_in_lds"] == 1 and plan(2, t_rows, 5, 12)["rows_in_lds"] == 0
  assert plan(2, t_trace - 1, 5, 12)["trace_at"] == 0 and plan(2, t_trace, 5, 12)["trace_at"] == 1
  assert lib.lr_ctc_spot_workspace_bytes(2, t_trace - 1, C, 5, 12, 4) == 16
  assert lib.lr_ctc_spot_workspace_bytes(2, t_trace, C, 5, 12, 4) == 2 * 5 * t_trace * 8
  T = dict(rows_lds_last=t_rows - 1, rows_global_first=t_rows, trace_lds_last=t_trace - 1, trace_ws_first=t_trace)[where]
  print("%s: T = %d, plan %r" % (where, T, plan(2, T, 5, 12)))
  lp, sizes, kw, ln = placed_case(T, seed=T)
  thr = np.array([-40.0, -6.0, -0.5, -30.0, -40.0], np.float32)
  want = check_both_ways(dev, lp, sizes, kw, ln, thr=thr, H=16, what=where)
  assert want["n_hits"].max() > 4


def test_the_longest_clip_and_the_longest_keyword(dev):
  """T = 2048, L = 32, B = 2, K = 5: rows from global memory, the trace in the workspace."""
  T = 2048
  assert plan(2, T, 5, 32) == dict(plan(2, T, 5, 32), segment=64, rows_in_lds=0, trace_at=1)
  lp, sizes, kw, ln = placed_case(T, seed=2048, W=32)
  check_both_ways(dev, lp, sizes, kw, ln, H=4, what="2048x32")


# ---- 3: planted clips and the greedy decoder ------------------------------------------------------------------------
def test_planted_keywords_are_found_where_they_were_planted(dev):
  """The blank boosted by +12 on every frame, a frame-level spelling of y = [5, 9, 9, 12] (doubled letter, interior
  blanks) boosted by +12 at frames 20 and 50: exactly those two spans, score 0.0; nothing for a keyword not planted."""
  from lipreading_amd.spot import KeywordSpotter
  T = 75
  y = [5, 9, 9, 12]
  spelling = [5, 5, 0, 9, 0, 9, 9, 12]
  rng = np.random.RandomState(12)
  logits = rng.randn(2, T, C).astype(np.float32)
  planted = np.zeros((2, T), np.int64)
  for at in (20, 50):
    planted[0, at:at + len(spelling)] = spelling
  for b in range(2):
    logits[b, np.arange(T), planted[b]] += 12.0
  lp = torch.log_softmax(torch.from_numpy(logits), dim=-1).to(dev)
  word, other = ''.join(LABELS[c] for c in y), ''.join(LABELS[c] for c in (40, 41, 42))
  sp = KeywordSpotter(LABELS, [other, word], min_confidence=math.exp(-1.0 / 4), max_hits=4)
  assert abs(float(sp.min_scores[1]) + 1.0) < 1e-6
  out = {k: v.cpu().numpy() for k, v in sp.spot_ids(lp).items()}
  assert out["n_hits"].tolist() == [[0, 2], [0, 0]] and (out["status"] == 0).all()
  got = [(float(out["hit_score"][0, 1, h]), int(out["hit_start"][0, 1, h]), int(out["hit_end"][0, 1, h]))
         for h in range(2)]
  assert got == [(0.0, 20, 28), (0.0, 50, 58)]
  assert (out["hit_score"][0, 1, 2:] == -np.inf).all() and (out["hit_start"][0, 1, 2:] == -1).all()
  recs = sp.spot(lp)
  assert recs[1] == [] and [(r["keyword"], r["index"], r["start"], r["end"], r["score"], r["confidence"])
                            for r in recs[0]] == [(word, 1, 20, 28, 0.0, 1.0), (word, 1, 50, 58, 0.0, 1.0)]
  assert all(type(r["start"]) is int and type(r["end"]) is int for r in recs[0])
  assert sp.seconds(recs[0][1]["start"]) == 50 / 29.97


def test_a_hit_that_scores_zero_is_what_the_greedy_decoder_reads_there(dev):
  from lipreading_amd.decoder import GreedyDecoder
  from lipreading_amd.spot import KeywordSpotter
  labels = ['_', 'a', 'b', 'c', ' ']
  words = ["a", "b", "ab", "ba", "cc", "a b", "abc", "bb"]
  rng = np.random.RandomState(31)
  T, B = 40, 4
  lp_h = S.log_softmax(rng, (B, T, len(labels)))
  lp_h[1] = S.integers(rng, (T, len(labels)))          # ties in the arg-max: zero ratios on several classes
  sizes_h = np.array([T, T, 25, 1], np.int32)
  lp, sizes = torch.from_numpy(lp_h).to(dev), torch.from_numpy(sizes_h).to(dev)
  sp = KeywordSpotter(labels, words, max_hits=8)
  recs = sp.spot(lp, sizes)
  zero = [(b, r) for b in (0, 2, 3) for r in recs[b] if r["score"] == 0.0]   # (clip 1 has no unique greedy path)
  assert len(zero) >= 8 and any(len(r["keyword"]) > 1 for _, r in zero)
  width = max(r["end"] - r["start"] for _, r in zero)
  spans = torch.zeros(len(zero), width, len(labels), device=dev)
  for i, (b, r) in enumerate(zero):
    spans[i, :r["end"] - r["start"]] = lp[b, r["start"]:r["end"]]
  lens_d = torch.tensor([r["end"] - r["start"] for _, r in zero], dtype=torch.int32, device=dev)
  ids, _, lens = GreedyDecoder(labels).decode_ids(spans, lens_d)
  ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
  for i, (b, r) in enumerate(zero):
    assert ''.join(labels[c] for c in ids[i, :lens[i]]) == r["keyword"], (b, r)
  # and the records are the restatement's hits, confidence included
  want = S.expected(lp_h, sizes_h, sp.ids, sp.lengths, 0, None, 8)
  for b in range(B):
    flat = [(k, float(want["hit_score"][b, k, h]), int(want["hit_start"][b, k, h]), int(want["hit_end"][b, k, h]))
            for k in range(len(words)) for h in range(want["n_hits"][b, k])]
    assert [(r["index"], r["score"], r["start"], r["end"]) for r in recs[b]] == flat
    assert all(r["confidence"] == math.exp(r["score"] / len(r["keyword"])) for r in recs[b])


# ---- 4: layouts and bad inputs --------------------------------------------------------------------------------------
def spotter_case(seed, T=33, min_confidence=None):
  """A KeywordSpotter over LABELS with keywords of every segment width in an unsorted order, clips, and the
  restatement's answer."""
  from lipreading_amd.spot import KeywordSpotter
  rng = np.random.RandomState(seed)
  lp, sizes = clips(rng, T)
  words = []
  for k, L in enumerate((9, 1, 17, 3, 32, 8, 16, 2, 5)):
    y = [FIRST_CHAR + c % (C - FIRST_CHAR) for c in S.random_target(rng, L, C, 0, doubled=k % 2 == 1)]
    words.append(''.join(LABELS[c] for c in y))
  sp = KeywordSpotter(LABELS, words, max_hits=3, min_confidence=min_confidence)
  want = S.expected(lp, sizes, sp.ids, sp.lengths, 0, sp.min_scores, 3)
  return sp, lp, sizes, want


def test_strided_layouts_and_trace_or_not(dev):
  sp, lp, sizes, want = spotter_case(9, min_confidence=0.02)
  assert not sp._sorted and 0 < want["n_hits"].sum() < want["n_hits"].size * 3
  B, T = lp.shape[:2]
  d = lambda a: torch.from_numpy(a).to(dev)
  tbc = d(lp).transpose(0, 1).contiguous()                       # (T, B, C) in memory
  big = torch.randn(2 * B + 1, T + 5, C + 3, device=dev)         # a slice with odd strides on both axes
  big[1::2, :T, :C][:B] = d(lp)
  views = dict(plain=d(lp), transposed=tbc.transpose(0, 1), sliced=big[1::2, :T, :C][:B])
  assert views["transposed"].stride() == (C, B * C, 1) and views["sliced"].stride(0) == 2 * (T + 5) * (C + 3)
  for name, v in views.items():
    full = {k: x.cpu().numpy() for k, x in sp.spot_ids(v, d(sizes), trace=True).items()}
    assert sorted(full) == sorted(OUTPUTS)
    assert_equal(full, want, name)
    bare = {k: x.cpu().numpy() for k, x in sp.spot_ids(v, d(sizes)).items()}
    assert sorted(bare) == sorted(HIT_OUTPUTS)
    assert_equal(bare, want, name, HIT_OUTPUTS)
  # sizes=None is T
  whole = S.expected(lp, None, sp.ids, sp.lengths, 0, sp.min_scores, 3)
  assert_equal({k: x.cpu().numpy() for k, x in sp.spot_ids(d(lp), None, trace=True).items()}, whole, "no sizes")


def test_bad_pairs_touch_only_themselves_and_guards_stay(dev):
  rng = np.random.RandomState(3)
  T = 40
  lp, sizes = clips(rng, T)
  kw, ln = S.keyword_batch(rng, [3, 8, 12, 1, 5, 9, 20, 4, 6], C, 0, stride=20)
  kw[1, 0] = 0          # the blank inside the length
  kw[2, 11] = C         # past the classes
  kw[4, 2] = -3
  ln[3], ln[7] = 0, 21
  sizes[1], sizes[4] = 0, T + 1
  want = S.expected(lp, sizes, kw, ln, 0, None, 4)
  assert want["status"][0].tolist() == [0, -1, -1, -2, -1, 0, 0, -2, 0] and (want["status"][[1, 4]] == -2).all()
  assert_equal(raw_spot(dev, lp, sizes, kw, ln, guard=64), want)
  assert_equal(raw_spot(dev, lp, sizes, kw, ln, trace=False, guard=64), want, keys=HIT_OUTPUTS)


def test_limits_raise_before_any_launch(dev):
  from lipreading_amd.spot import KeywordSpotter
  sp = KeywordSpotter(LABELS, ["the"])
  with pytest.raises(ValueError, match="T=2049.*2048"):
    sp.spot_ids(torch.zeros(1, 2049, C, device=dev))
  with pytest.raises(ValueError):
    sp.spot_ids(torch.zeros(1, 10, C, device=dev), torch.ones(2, dtype=torch.int32, device=dev))
  with pytest.raises(KeyError):
    sp.spot_ids(torch.zeros(1, 10, C + 1, device=dev))
  lib = _C.lib()
  one = torch.zeros(64, device=dev)
  args = lambda T, W, H: (one.data_ptr(), 0, 0, None, one.data_ptr(), W, one.data_ptr(), None, 0, H) + \
      (one.data_ptr(),) * 5 + (None, None, one.data_ptr(), 16, 1, T, C, 1, _C.stream_handle())
  assert lib.lr_ctc_spot(*args(2049, 4, 4)) == _C.LR_ERR_UNSUPPORTED
  assert lib.lr_ctc_spot(*args(75, 33, 4)) == _C.LR_ERR_UNSUPPORTED
  assert lib.lr_ctc_spot(*args(75, 4, 17)) == _C.LR_ERR_UNSUPPORTED


def test_spot_ids_reads_nothing_back(dev):
  probe = torch.ones(1, device=dev)
  torch.cuda.set_sync_debug_mode("error")
  try:
    try:
      probe.item()
      honoured = False
    except RuntimeError:
      honoured = True
  finally:
    torch.cuda.set_sync_debug_mode("default")
  if not honoured:
    pytest.skip("this torch build does not honour set_sync_debug_mode('error') on ROCm")
  sp, lp, sizes, want = spotter_case(6)
  lp_d, sz_d = torch.from_numpy(lp).to(dev), torch.from_numpy(sizes).to(dev)
  first = sp.spot_ids(lp_d, sz_d, trace=True)     # the tables' upload and the workspace happen once per device / shape
  sz_long = sz_d.long()
  torch.cuda.set_sync_debug_mode("error")
  try:
    again = sp.spot_ids(lp_d, sz_d, trace=True)
    longs = sp.spot_ids(lp_d, sz_long)
  finally:
    torch.cuda.set_sync_debug_mode("default")
  for k in first:
    assert torch.equal(first[k], again[k]), k
  for k in longs:
    assert torch.equal(first[k], longs[k]), k
  assert_equal({k: v.cpu().numpy() for k, v in first.items()}, want)


# ---- 5: loader and driver -------------------------------------------------------------------------------------------
KEYWORDS = ["the", "a", "you", "thank you", "welcome", "fox"]


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
  """A GRU-32 + CTC head trained for one epoch on a synthetic dataview, and its loader (batches of 4)."""
  from lipreading_amd import dataset as DS
  from lipreading_amd import train as T
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  root = str(tmp_path_factory.mktemp("spot"))
  DS.write_synthetic_dataview(root, "synthetic/nano", n_videos=3, captions_per_video=6, seed=1)
  tr, _, _ = DS.split_dataset(root, "synthetic/nano", 0.8, np.random.RandomState(123456))
  ds = DS.FrameCaptionDataset(root, "synthetic/nano", "train", tr)
  loader = DS.make_loader(ds, 4, make_collate_fn(dev))
  torch.manual_seed(123456)
  enc = VideoEncoder(204, 32, rnn_type="GRU", bidirectional=True, enable_ctc=True, vocab_size=len(ds.char2idx),
                     char2idx=ds.char2idx).to(dev)
  T.train(enc, None, loader, FusedAdam(FlatParameters(enc), lr=4e-3), dev, ds.char2idx, grad_norm=50)
  return enc, loader, ds.char2idx


def by_hand(enc, loader, dev, c2i, keywords, **kw):
  from lipreading_amd.spot import KeywordSpotter
  sp = KeywordSpotter(ctc_labels(c2i), keywords, **kw)
  recs = []
  enc.eval()
  with torch.no_grad():
    for frames, frame_lens, chars, char_lens in loader:
      lens_d = frame_lens.to(dev)
      lp = enc(frames.to(dev), lens_d, max_len=int(frame_lens.max()))[0]
      for b, found in enumerate(sp.spot(lp, lens_d)):
        recs.append(dict(index=len(recs), frames=int(frame_lens[b]), hits=found))
  return recs


def test_spot_loader_equals_spotting_each_batch_by_hand(dev, trained):
  from lipreading_amd import analysis
  from lipreading_amd import train as T
  enc, loader, c2i = trained
  got = list(T.spot_loader(enc, loader, dev, c2i, KEYWORDS, max_hits=2))
  want = by_hand(enc, loader, dev, c2i, KEYWORDS, max_hits=2)
  n = sum(len(b[3]) for b in loader)
  assert got == want and len(got) == n > 0 and [r["index"] for r in got] == list(range(n))
  assert any(r["hits"] for r in got)
  for r in got:
    assert [h["index"] for h in r["hits"]] == sorted(h["index"] for h in r["hits"])
    for h in r["hits"]:
      assert 0 <= h["start"] < h["end"] <= r["frames"] and h["score"] <= 0 and 0 < h["confidence"] <= 1
      assert h["keyword"] == KEYWORDS[h["index"]] and h["end"] - h["start"] >= len(h["keyword"])
  report = analysis.keyword_report(enc, loader, dev, c2i, KEYWORDS, max_hits=2)
  assert [r["keyword"] for r in report] == KEYWORDS
  inv = {v: k for k, v in c2i.items()}
  captions = [''.join(inv[int(c)] for c in chars[b, 1:int(cl[b]) - 1])
              for _, _, chars, cl in loader for b in range(len(cl))]
  assert report == analysis.keyword_counts(captions, [r["hits"] for r in got], KEYWORDS)
  assert sum(r["utterances"] for r in report) > 0
  for r in report:
    assert 0 <= r["hit"] <= r["utterances"] <= n and r["false_hits"] >= 0
  with pytest.raises(ValueError):
    enc.enable_ctc = False
    try:
      next(T.spot_loader(enc, loader, dev, c2i, KEYWORDS))
    finally:
      enc.enable_ctc = True


def test_driver_writes_one_line_per_validation_utterance(dev, tmp_path):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=10, captions_per_video=6, seed=7)
  path = str(tmp_path / "val_spot.jsonl")
  words = tmp_path / "keywords.txt"
  words.write_text('\n'.join(KEYWORDS) + '\n')
  out = driver.run(**driver.parse_flags(["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True",
                                         "--ctc_only=True", "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=1",
                                         "--spot=" + path, "--keywords=" + str(words), "--spot_max_hits=2",
                                         "--spot_confidence=0.001"]))
  val = out["loaders"][1]
  n = sum(len(b[3]) for b in val)
  with open(path) as f:
    lines = [json.loads(l) for l in f]
  assert len(lines) == n > 0 and [l["index"] for l in lines] == list(range(n))
  assert out["spot"] == dict(path=path, utterances=n, keywords=len(KEYWORDS), hits=sum(len(l["hits"]) for l in lines))
  for l in lines:
    assert set(l) == {"index", "frames", "hits"}
    for h in l["hits"]:
      assert set(h) == {"keyword", "start", "end", "start_s", "end_s", "score", "confidence"}
      assert 0 <= h["start"] < h["end"] <= l["frames"] and h["keyword"] in KEYWORDS
      assert h["start_s"] == h["start"] / 29.97 and h["end_s"] == h["end"] / 29.97
      assert h["confidence"] >= 0.001 * (1 - 1e-6)      # (the threshold is float32(L * log p))
  # the file is what a direct KeywordSpotter.spot call gives on the same model and loader
  want = by_hand(out["encoder"], val, dev, out["char2idx"], KEYWORDS, max_hits=2, min_confidence=0.001)
  assert [(l["index"], l["frames"]) for l in lines] == [(r["index"], r["frames"]) for r in want]
  for l, r in zip(lines, want):
    assert [(h["keyword"], h["start"], h["end"], h["score"], h["confidence"]) for h in l["hits"]] == \
        [(h["keyword"], h["start"], h["end"], h["score"], h["confidence"]) for h in r["hits"]]
