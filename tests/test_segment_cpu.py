"""No GPU: the restatement of lr_ctc_segment (tests/segment_cases.py) against the aligner's restatement, against
exhaustive enumeration and on planted streams; the host-only half of the C ABI; the driver's --segment flag, the
segmenter's encode / records and the whole-video plumbing around them."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

from lipreading_amd import _C, analysis, driver
from lipreading_amd.data import EOS, default_char2idx
from lipreading_amd.decoder import ctc_labels
from tests import align_cases as A
from tests import segment_cases as S

LABELS = ctc_labels(default_char2idx())
C = len(LABELS)
ALL_FLAGS = (0, S.FREE_START, S.FREE_END, S.FREE_START | S.FREE_END)


# ---- 1: with both flags clear the recursion is the aligner's ------------------------------------------------------------
@pytest.mark.parametrize("n,L", ((1, 0), (1, 1), (5, 2), (40, 13), (64, 32), (200, 90)))
@pytest.mark.parametrize("name,family", A.FAMILIES)
def test_fixed_ends_equal_the_aligner_bit_for_bit(n, L, name, family):
  rng = np.random.RandomState(100 * n + L)
  lp = family(rng, (n, 8))
  y = A.random_target(rng, L, 8, 0, doubled=True)
  total, path = A.viterbi(lp, y, 0)
  got_total, got_path, first = S.viterbi(lp, y, 0, 0)
  assert got_total.dtype == np.float32 and got_total.tobytes() == total.tobytes()
  assert path is not None and got_path == path and first == 0
  want, got = A.align_one(lp, y, 0), S.segment_one(lp, y, 0, 0)
  assert got["span"] == (0, n) and got["frame_token"] == want["frame_token"]
  assert [(s, e, p.tobytes()) for s, e, p in got["tok"]] == [(s, e, p.tobytes()) for s, e, p in want["tok"]]


def test_fixed_ends_agree_on_what_is_infeasible():
  lp = A.integers(np.random.RandomState(3), (4, 5))
  assert A.viterbi(lp, [2, 2, 2], 0)[1] is None
  assert S.segment_one(lp, [2, 2, 2], 0, 0)["status"] == S.INFEASIBLE
  assert S.segment_one(lp, [2, 2, 2], 0, S.FREE_START | S.FREE_END)["status"] == S.INFEASIBLE


# ---- 2: exhaustive enumeration ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_total_is_the_best_over_every_span_and_every_sequence(flags):
  rng = np.random.RandomState(17 + flags)
  seen = 0
  for n in range(1, 7):
    for L in range(0, 4):
      for rep in range(2):
        lp = A.integers(rng, (n, 3))
        y = A.random_target(rng, L, 3, 0, doubled=bool(rep))
        want = S.best_by_enumeration(lp, y, 0, flags)
        got = S.segment_one(lp, y, 0, flags)
        if want is None:
          assert got["status"] == S.INFEASIBLE, (n, y)
          continue
        seen += 1
        assert got["status"] == 0 and float(got["total"]) == want, (n, y, flags)
        a, b = got["span"]
        assert 0 <= a < b <= n and (flags & S.FREE_START or a == 0) and (flags & S.FREE_END or b == n)
        # the path's own frames score the total, and collapse to the target
        seq = [0 if i < 0 else y[i] for i in got["frame_token"][a:b]]
        assert sum(float(lp[a + k, c]) for k, c in enumerate(seq)) == want
  assert seen > 20


# ---- 3: planted streams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(60))
def test_planted_utterances_are_found(seed):
  lp, y, utts, planted = S.planted_stream(seed)
  free = S.segment_one(lp, y, 0, S.FREE_START | S.FREE_END, utts)
  assert free["status"] == 0
  for (s, e, frames, _, worst), (ps, pe), (f, c) in zip(free["utts"], planted, utts):
    # inside the planted span, missing at most a run (3 frames) ... plus one blank at the end
    assert ps <= s <= ps + 3 and pe - 3 <= e <= pe, (seed, (s, e), (ps, pe))
    assert 0 < frames <= e - s and f <= worst < f + c
  # The reason for the flags.  Every frame scores at most log(e^8 / (e^8 + 11)) < 0, and the planted path exists, so the
  # free total is above -250 * 0.0037 > -2.  With both ends fixed, frame 0 sits in state 0 or 1 and the last frame in
  # state 2L-1 or 2L, whose classes (blank, first token, last token) the junk frames avoid: at most -8 each.
  assert free["total"] > -2.0
  fixed = S.segment_one(lp, y, 0, 0, utts)
  assert fixed["status"] == 0 and fixed["total"] < -16.0


# ---- 4: the host-only half of the ABI ---------------------------------------------------------------------------------------
def plan_of(B, T, Cn, W):
  plan = (ctypes.c_int32 * _C.LR_SEG_PLAN_WORDS)()
  return _C.lib().lr_ctc_segment_plan(B, T, Cn, W, ctypes.addressof(plan)), list(plan)


def documented_bytes(B, T, W, own):
  states = -(-(2 * W + 1) // own) * own
  return B * ((-(-T // 16) + 2) * states * 4 + 64)


def test_workspace_and_plan_are_decided_on_the_host():
  lib = _C.lib()
  assert (_C.LR_SEG_MAX_T, _C.LR_SEG_MAX_TOKENS, _C.LR_SEG_FREE_START, _C.LR_SEG_FREE_END) == (65536, 16384, 1, 2)
  assert (_C.LR_SEG_INFEASIBLE, _C.LR_SEG_BAD_ID, _C.LR_SEG_BAD_LENGTH, _C.LR_SEG_BAD_UTTERANCE) == (1, -1, -2, -3)
  ok, plan = plan_of(8, 65536, 65, 16384)
  own, frames, launches, wgs, threads, lds = plan
  assert ok == _C.LR_OK and own > 0 and frames > 0 and threads % 64 == 0 and 0 < threads <= 1024 and 0 <= lds <= 65536
  assert launches * frames >= 65536 > (launches - 1) * frames
  assert wgs == 8 * -(-(2 * 16384 + 1) // own)
  big = lib.lr_ctc_segment_workspace_bytes(8, 65536, 65, 16384)
  assert big > 2 ** 32 and big == documented_bytes(8, 65536, 16384, own)
  for B, T, W in ((1, 1, 0), (3, 2500, 300), (2, 4097, 1)):
    ok, plan = plan_of(B, T, 8, W)
    assert ok == _C.LR_OK and plan[2] * plan[1] >= T > (plan[2] - 1) * plan[1]
    assert lib.lr_ctc_segment_workspace_bytes(B, T, 8, W) == documented_bytes(B, T, W, plan[0])
  assert _C.LR_SEG_MAX_B == 65535 and plan_of(65535, 16, 8, 1)[0] == _C.LR_OK      # a sample is a row of the grids
  for args, status in (((1, 65537, 65, 4), _C.LR_ERR_UNSUPPORTED), ((1, 64, 65, 16385), _C.LR_ERR_UNSUPPORTED),
                       ((65536, 16, 8, 1), _C.LR_ERR_UNSUPPORTED),
                       ((0, 64, 65, 4), _C.LR_ERR_INVALID_ARG), ((1, 0, 65, 4), _C.LR_ERR_INVALID_ARG),
                       ((1, 64, 1, 4), _C.LR_ERR_INVALID_ARG), ((1, 64, 65, -1), _C.LR_ERR_INVALID_ARG)):
    assert lib.lr_ctc_segment_workspace_bytes(*args) == 0 and plan_of(*args)[0] == status, args


def test_the_entry_rejects_bad_arguments_before_any_launch():
  lib = _C.lib()
  buf = ctypes.create_string_buffer(256)
  p = ctypes.addressof(buf)

  def call(T=64, W=4, lp=p, n_utts=None, utt=None, flags=3, ws_bytes=1 << 40, blank=0, stride=4):
    return lib.lr_ctc_segment(lp, T * 65, 65, None, p, stride, p, utt, utt, 2, n_utts, blank, flags, p, p, p, p, utt, utt,
                              utt, utt, utt, p, p, p, p, ws_bytes, 1, T, 65, W, None)

  assert call(T=65537) == _C.LR_ERR_UNSUPPORTED and call(W=16385, stride=4) == _C.LR_ERR_UNSUPPORTED
  assert call(lp=None) == _C.LR_ERR_INVALID_ARG
  assert call(n_utts=p) == _C.LR_ERR_INVALID_ARG            # utterance counts without the utterance buffers
  assert call(flags=4) == _C.LR_ERR_INVALID_ARG and call(blank=65) == _C.LR_ERR_INVALID_ARG
  assert call(stride=5) == _C.LR_ERR_INVALID_ARG            # target_stride > max_tokens
  assert call(ws_bytes=16) == _C.LR_ERR_WORKSPACE


# ---- 5: flags, encode, records, whole-video plumbing --------------------------------------------------------------------------
def test_segment_flag_parses_and_needs_a_ctc_head(tmp_path):
  assert driver.DEFAULTS["segment"] == "" and driver.parse_flags([])["segment"] == ""
  f = driver.parse_flags(["--enable_ctc=True", "--segment=/tmp/x.jsonl"])
  assert f["segment"] == "/tmp/x.jsonl" and f["align"] == "" and f["spot"] == ""
  assert driver.parse_flags(["--frontend=conv3d", "--segment=s.jsonl"])["enable_ctc"] is True
  with pytest.raises(ValueError, match="--segment=s.jsonl needs a CTC head"):
    driver.parse_flags(["--segment=s.jsonl"])
  with pytest.raises(ValueError, match="CTC head"):
    driver.segment_check(dict(segment="s.jsonl", enable_ctc=False))
  driver.segment_check(dict(segment="", enable_ctc=False))
  driver.segment_check(dict(segment="s.jsonl", enable_ctc=True))


def test_encode_lays_utterances_end_to_end_with_their_tail():
  from lipreading_amd.segment import CTCSegmenter
  sg = CTCSegmenter(LABELS)
  eos = LABELS.index(EOS)
  tg, tl, uf, uc, nu = sg.encode([["ab", "", "c a"], [], ["b"]], tail=EOS)
  ids = lambda s: [LABELS.index(ch) for ch in s]
  assert tl.tolist() == [8, 0, 2] and nu.tolist() == [3, 0, 1] and tg.shape == (3, 8) and uf.shape == uc.shape == (3, 3)
  assert tg[0].tolist() == ids("ab") + [eos] + [eos] + ids("c a") + [eos] and tg[2, :2].tolist() == ids("b") + [eos]
  assert uf[0].tolist() == [0, 3, 4] and uc[0].tolist() == [3, 1, 4] and (uf[2, 0], uc[2, 0]) == (0, 2)
  assert all(t.dtype == torch.int32 for t in (tg, tl, uf, uc, nu))
  tg, tl, uf, uc, nu = sg.encode([["ab", ""]])
  assert tl.tolist() == [2] and uc[0].tolist() == [2, 0] and uf[0].tolist() == [0, 2]
  assert sg.encode([[]])[0].shape == (1, 1)
  with pytest.raises(KeyError, match="'é'"):
    sg.encode([["café"]])
  with pytest.raises(KeyError, match="tail"):
    sg.encode([["a"]], tail="<NOPE>")
  with pytest.raises(KeyError, match="tail"):
    sg.encode([["a"]], tail=LABELS[0])
  with pytest.raises(_C.LipReadingHipError, match="no CPU fallback"):
    sg.segment(torch.zeros(1, 4, C), None, [["a"]])


def test_records_are_assembled_from_the_device_dict():
  from lipreading_amd.segment import CTCSegmenter
  sg = CTCSegmenter(LABELS, fps=25.0)
  texts = [["hi", "", "yo"], ["a"]]
  tg = sg.encode(texts, tail=EOS)[0]
  i32 = lambda rows: torch.tensor(rows, dtype=torch.int32)
  out = dict(utt_start=i32([[10, -1, 40], [-1, -1, -1]]), utt_end=i32([[20, -1, 55], [-1, -1, -1]]),
             utt_frames=i32([[8, 0, 0], [0, 0, 0]]), utt_worst=i32([[1, -1, 4], [-1, -1, -1]]),
             utt_logp=torch.tensor([[-4.0, 0.0, -1.5], [0.0, 0.0, 0.0]]), span=i32([[10, 55], [-1, -1]]),
             status=i32([0, 1]), total=torch.tensor([-5.5, float("-inf")]))
  recs = sg.records(out, texts, tg)
  assert recs[1] == dict(status=1, total=float("-inf"), span=(-1, -1), utterances=[])
  assert (recs[0]["status"], recs[0]["total"], recs[0]["span"]) == (0, -5.5, (10, 55))
  hi, empty, yo = recs[0]["utterances"]
  assert hi == dict(text="hi", start=10, end=20, start_s=0.4, end_s=0.8, logp=-4.0, frames=8,
                    confidence=math.exp(-4.0 / 8), worst="i")
  assert empty == dict(text="", start=-1, end=-1, start_s=None, end_s=None, logp=0.0, frames=0, confidence=None,
                       worst=None)
  assert yo["confidence"] is None and yo["worst"] == "y" and (yo["start_s"], yo["end_s"]) == (1.6, 2.2)


def test_video_clips_keep_start_order_and_times(tmp_path):
  from lipreading_amd import dataset as DS
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/nano", n_videos=2, captions_per_video=5, seed=3)
  vids = sorted(DS.gen_vid_ids(root, "synth/nano", np.random.RandomState(0)))
  c2i = DS.build_vocab(root, "synth/nano")
  clips = DS.VideoClips(vids[0], c2i)
  s_e = list(np.load(vids[0] + "s_e.npy", allow_pickle=True))
  caps = list(np.load(vids[0] + "cap.npy", allow_pickle=True))
  lmk = list(np.load(vids[0] + "face_lmk_seq.npy", allow_pickle=True))
  assert len(clips) == len(clips.kept) > 0 and clips.kept == sorted(clips.kept, key=lambda i: s_e[i][0])
  # the filter of FrameCaptionDataset, in the video's own order
  f, c = DS.filter_occlusions(lmk, caps, s_e)
  assert clips.captions == c and all(a is b or np.array_equal(a, b) for a, b in zip(clips.frames, f))
  assert clips.s_e == [tuple(map(float, s_e[i])) for i in clips.kept]
  frames, ids = clips[1]
  assert frames.shape == lmk[clips.kept[1]].shape and ids.tolist() == DS.parse_caption(c2i, clips.captions[1]).tolist()
  assert len(DS.VideoClips(vids[0], c2i, threshold=50.0)) == 0       # a video may keep nothing


def test_video_clips_serve_the_pixel_regime(tmp_path):
  from lipreading_amd import dataset as DS
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/pix", n_videos=1, captions_per_video=3, seed=4, frames=True, frame_hw=16,
                              min_seconds=0.5, max_seconds=0.8)
  vid = DS.gen_vid_ids(root, "synth/pix", np.random.RandomState(0))[0]
  clips = DS.VideoClips(vid, DS.build_vocab(root, "synth/pix"), pixels=True)
  pix = list(np.load(vid + "face_frames_seq.npy", allow_pickle=True))
  assert len(clips) > 0
  for i in range(len(clips)):
    (p, lmk), ids = clips[i]
    assert p.dtype == np.uint8 and np.array_equal(p, pix[clips.kept[i]]) and lmk.shape == (p.shape[0], 68, 3)
    assert len(ids) == len(clips.captions[i]) + 2


def test_stream_positions_and_caption_shifts():
  from lipreading_amd import train as T
  offsets = [0, 30, 75]
  assert [T.stream_position(offsets, t) for t in (0, 29, 30, 74, 75, 200)] == [(0, 0), (0, 29), (1, 0), (1, 44), (2, 0),
                                                                               (2, 125)]
  cap = lambda os_, oe, ns, ne, conf: dict(old_start_s=os_, old_end_s=oe, new_start_s=ns, new_end_s=ne, confidence=conf)
  recs = [dict(video="a", status=0, captions=[cap(0, 1, 0.25, 1, 0.9), cap(1, 2, 1, 2.5, 0.2), cap(2, 3, 2, 3, None)]),
          dict(video="b", status=2, captions=[dict(old_start_s=0, old_end_s=1)]),
          dict(video="c", status=0, captions=[cap(0, 1, 0, 1, 0.5), cap(1, 2, 1.5, 2, 0.6)])]
  recs = json.loads(json.dumps(recs))
  assert analysis.caption_shifts(recs, min_confidence=0.5) == [
      dict(video="a", status=0, captions=3, median_shift_s=0.25, max_shift_s=0.5, low_confidence=2),
      dict(video="b", status=2, captions=1, median_shift_s=None, max_shift_s=None, low_confidence=1),
      dict(video="c", status=0, captions=2, median_shift_s=0.25, max_shift_s=0.5, low_confidence=0)]
