"""GPU: lr_edit_distance / scoring.EditScorer against the plain-Python restatement of tests/test_edit_cpu.py, and the
device scoring loops (train.device_cer / device_scores, the driver's --score=device, analysis.confusion_matrix) against
the host loops they replace.  Everything is integer-exact: every comparison is `==`."""
import random

import numpy as np
import pytest
import torch

from tests.test_edit_cpu import (LABELS, align, confusion_ref, expand, random_ids, score_ref, special_classes, table)

pytestmark = pytest.mark.gpu

EOS = '<EOS>'
# one character per class (longest spelling 1): token lengths ARE character lengths, up to the kernel's limits
SIMPLE = ['_', ' ', 'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', EOS]
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256]
FIELDS = ("distance", "ref_len", "hyp_len", "hits", "sub", "ins", "dele")
JUNK = 10 ** 6   # what lies past a row's length: never read


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def pack(seqs, width, dev):
  ids = torch.full((len(seqs), max(width, 1)), JUNK, dtype=torch.int32)
  for b, s in enumerate(seqs):
    ids[b, :len(s)] = torch.tensor(s, dtype=torch.int32)
  return ids.to(dev), torch.tensor([len(s) for s in seqs], dtype=torch.int32, device=dev)


def run(sc, hyps, refs, dev, unit='char', align_=False, gate=None):
  """-> {field: list over pairs} read back from one score() call."""
  h, hl = pack(hyps, max(len(s) for s in hyps), dev)
  r, rl = pack(refs, max(len(s) for s in refs), dev)
  out = sc.score(h, hl, r, rl, unit=unit, align=align_, gate=gate)
  return {k: v.cpu().tolist() for k, v in out.items()}


def want_rows(hyps, refs, labels, unit, align_):
  rows, steps = [], []
  for h, r in zip(hyps, refs):
    w, st = score_ref(h, r, labels, unit)
    if not align_:
      w.update(hits=0, sub=0, ins=0, dele=0)
    rows.append(w)
    steps.append(st)
  return rows, steps


def check(got, rows):
  assert got["status"] == [0] * len(rows)
  for f in FIELDS:
    assert got[f] == [w[f] for w in rows], f


def mutated(rng, ref, n_classes, length):
  """A hypothesis that resembles `ref`: realistic alignments (runs of hits between the errors)."""
  out = []
  for c in ref:
    u = rng.random()
    if u < 0.1:
      continue
    out.append(rng.randrange(n_classes) if u < 0.2 else c)
    if u > 0.93:
      out.append(rng.randrange(n_classes))
  while len(out) < length:
    out.append(rng.randrange(n_classes))
  return out[:length]


def crossed_pairs(labels, seed):
  rng = random.Random(seed)
  sp = special_classes(labels) if '<UNK>' in labels else [labels.index(' '), labels.index(EOS)]
  hyps, refs = [], []
  for k, n in enumerate(LENGTHS):
    for m in LENGTHS:
      ref = random_ids(rng, len(labels), m, sp)
      hyp = mutated(rng, ref, len(labels), n) if (k + m) % 2 else random_ids(rng, len(labels), n, sp)
      hyps.append(hyp)
      refs.append(ref)
  return hyps, refs


@pytest.mark.parametrize("labels", [LABELS, SIMPLE], ids=["ctc65", "simple"])
@pytest.mark.parametrize("unit,align_", [("char", False), ("char", True), ("word", False)])
def test_crossed_lengths_match_the_restatement(dev, labels, unit, align_):
  """Lengths {0, 1, 2, 63, ..., 256} on both sides crossed, in one launch.  The 65 CTC labels (longest spelling 5,
  capacity 1280 per side) take the four-wavefront kernel and, with the alignment, the walk-back table in the
  workspace; the one-character labels the single-wavefront kernel with the table in LDS."""
  from lipreading_amd.scoring import EditScorer
  hyps, refs = crossed_pairs(labels, 11)
  sc = EditScorer(labels)
  rows, steps = want_rows(hyps, refs, labels, unit, align_)
  check(run(sc, hyps, refs, dev, unit, align_), rows)
  if align_:
    conf, symbols = sc.confusion()
    assert conf.cpu().tolist() == confusion_ref(steps, symbols)


def table_np(h, r):
  """test_edit_cpu.table, a row at a time: D[i][j] = min_k<=j (cand[k] + j - k) with cand the diagonal / upper moves."""
  h, r = np.asarray(h), np.asarray(r)
  n, m = len(h), len(r)
  D = np.zeros((n + 1, m + 1), dtype=np.int32)
  j = np.arange(m + 1, dtype=np.int32)
  D[0] = j
  cand = np.empty(m + 1, dtype=np.int32)
  for i in range(1, n + 1):
    cand[0] = i
    cand[1:] = np.minimum(D[i - 1, :-1] + (r != h[i - 1]), D[i - 1, 1:] + 1)
    D[i] = np.minimum.accumulate(cand - j) + j
  return D


def test_pairs_at_the_stated_limits(dev):
  """One pair at the limit of each mode (one-character labels): 4096 x 4096 characters, 4096 characters of words per
  side, 2048 x 2048 with the alignment.  The table of a pair this size comes from the row-at-a-time form of the
  restatement (checked against it first); the walk back is the restatement's own."""
  from lipreading_amd.scoring import EditScorer
  rng = random.Random(5)
  for _ in range(20):
    a = [rng.randrange(4) for _ in range(rng.randint(0, 30))]
    b = [rng.randrange(4) for _ in range(rng.randint(0, 30))]
    assert table_np(a, b).tolist() == table(a, b)
  sc = EditScorer(SIMPLE)
  letters = list(range(2, 10))   # classes 'a'..'h'

  def letter_pair(n):
    ref = [rng.randrange(8) for _ in range(n)]
    hyp = mutated(rng, ref, 8, n)
    return [c + 2 for c in hyp], [c + 2 for c in ref]

  hyp, ref = letter_pair(4096)
  got = run(sc, [hyp], [ref], dev)
  assert got["status"] == [0] and got["distance"] == [int(table_np(hyp, ref)[-1, -1])]
  assert got["ref_len"] == [4096] and got["hyp_len"] == [4096]
  # words: letter, space, letter, space, ... = 2048 one-letter words in 4096 characters; and longer words
  for wl in (1, 3):
    def words(n_chars):
      out = []
      while len(out) < n_chars:
        out += [rng.choice(letters[:3]) for _ in range(wl)] + [1]
      return out[:n_chars]
    h, r = words(4096), words(4096)
    want, _ = score_ref(h, r, SIMPLE, 'word') if wl == 3 else (None, None)
    hw = [w for w in expand(h, SIMPLE).split(' ') if w]
    rw = [w for w in expand(r, SIMPLE).split(' ') if w]
    code = {w: i for i, w in enumerate(sorted(set(hw + rw)))}
    d = int(table_np([code[w] for w in hw], [code[w] for w in rw])[-1, -1])
    if want is not None:
      assert want["distance"] == d
    got = run(sc, [h], [r], dev, unit='word')
    assert (got["status"], got["distance"], got["ref_len"], got["hyp_len"]) == ([0], [d], [len(rw)], [len(hw)])
  hyp, ref = letter_pair(2048)
  hs, rs = expand(hyp, SIMPLE), expand(ref, SIMPLE)
  d, hits, sub, ins, dele, steps = align(hs, rs, table_np([ord(c) for c in hs], [ord(c) for c in rs]))
  sc.reset()
  got = run(sc, [hyp], [ref], dev, align_=True)
  assert [got[f][0] for f in FIELDS] == [d, 2048, 2048, hits, sub, ins, dele]
  assert sc.confusion()[0].cpu().tolist() == confusion_ref([steps], sc.symbols)


def test_one_past_the_limit_is_unsupported_before_any_launch(dev):
  from lipreading_amd import _C
  from lipreading_amd.scoring import EditScorer
  lib = _C.lib()
  sc = EditScorer(SIMPLE)
  off, sym, totals, conf = sc._state(dev)
  lens = torch.zeros(1, dtype=torch.int32, device=dev)
  out = torch.full((1, 8), -77, dtype=torch.int32, device=dev)
  ws = torch.empty(1 << 21, dtype=torch.uint8, device=dev)
  for wh, wr, mode in ((4097, 8, 0), (8, 4097, 1), (2049, 8, 2), (8, 2049, 2)):
    ids_h = torch.zeros((1, wh), dtype=torch.int32, device=dev)
    ids_r = torch.zeros((1, wr), dtype=torch.int32, device=dev)
    st = lib.lr_edit_distance(ids_h.data_ptr(), wh, lens.data_ptr(), 1, ids_r.data_ptr(), wr, lens.data_ptr(), 1,
                              off.data_ptr(), sym.data_ptr(), len(SIMPLE), 1, sc.space_sym, mode, out.data_ptr(),
                              totals.data_ptr(), conf.data_ptr(), sc.K, None, ws.data_ptr(), ws.numel(), 1, wh, wr,
                              _C.stream_handle())
    assert st == _C.LR_ERR_UNSUPPORTED
    with pytest.raises(_C.LipReadingHipError, match="hyp_width=%d ref_width=%d" % (wh, wr)):
      sc.score(ids_h, lens, ids_r, lens, unit='word' if mode == 1 else 'char', align=mode == 2)
  assert out.cpu().tolist() == [[-77] * 8]          # nothing ran
  assert sc.result()["pairs"] == 0 and sc.result()["word_pairs"] == 0
  # a workspace smaller than the query's answer is refused too
  ids = torch.zeros((1, 2048), dtype=torch.int32, device=dev)
  st = lib.lr_edit_distance(ids.data_ptr(), 2048, lens.data_ptr(), 1, ids.data_ptr(), 2048, lens.data_ptr(), 1,
                            off.data_ptr(), sym.data_ptr(), len(SIMPLE), 1, sc.space_sym, 2, out.data_ptr(),
                            totals.data_ptr(), conf.data_ptr(), sc.K, None, ws.data_ptr(), 1024, 1, 2048, 2048,
                            _C.stream_handle())
  assert st == _C.LR_ERR_WORKSPACE


def test_identical_disjoint_prefix_pairs_and_strided_views(dev):
  """Hypotheses as `ids[:, 0]` of a (B, W, T) tensor with lengths `lens[:, 0]` of (B, W), references as a shifted view
  `chars[:, 1:]` — the forms the decoders and the loaders hand over."""
  from lipreading_amd.scoring import EditScorer
  rng = random.Random(3)
  sp = special_classes(LABELS)
  base = [random_ids(rng, len(LABELS), n, sp) for n in (0, 1, 17, 40, 75)]
  a, b = LABELS.index('a'), LABELS.index('b')
  hyps = base + [[a] * 30, [a] * 9, base[3][:20], base[4]]
  refs = base + [[b] * 30, [b] * 31, base[3], base[4][:33]]
  sc = EditScorer(LABELS)
  B, W, T = len(hyps), 3, 80
  ids = torch.full((B, W, T), JUNK, dtype=torch.int32)
  lens = torch.full((B, W), 10 ** 5, dtype=torch.int32)
  chars = torch.full((B, 81), JUNK, dtype=torch.int64)
  for k, (h, r) in enumerate(zip(hyps, refs)):
    ids[k, 0, :len(h)] = torch.tensor(h, dtype=torch.int32)
    lens[k, 0] = len(h)
    chars[k, 1:1 + len(r)] = torch.tensor(r, dtype=torch.int64)
  ids, lens, chars = ids.to(dev), lens.to(dev), chars.to(dev).to(torch.int32)
  ref_lens = torch.tensor([len(r) for r in refs], dtype=torch.int32, device=dev)
  assert ids[:, 0].stride(0) == W * T and lens[:, 0].stride(0) == W
  for unit, al in (("char", True), ("char", False), ("word", False)):
    out = sc.score(ids[:, 0], lens[:, 0], chars[:, 1:], ref_lens, unit=unit, align=al)
    check({k: v.cpu().tolist() for k, v in out.items()}, want_rows(hyps, refs, LABELS, unit, al)[0])
  rows = want_rows(hyps, refs, LABELS, "char", True)[0]
  for k in range(len(base)):
    assert rows[k]["distance"] == 0 and rows[k]["hits"] == rows[k]["ref_len"]       # identical
  assert rows[5]["sub"] == 30 and rows[6]["sub"] == 9 and rows[6]["dele"] == 22     # disjoint
  assert rows[7]["hits"] == rows[7]["hyp_len"] and rows[8]["hits"] == rows[8]["ref_len"]   # prefixes


def test_bad_ids_and_lengths_mark_the_pair_only(dev):
  from lipreading_amd.scoring import EditScorer
  sc = EditScorer(LABELS)
  a = LABELS.index('a')
  ids = torch.tensor([[a, a, a, a], [a, 65, a, a], [a, -1, a, a], [a, a, a, JUNK]], dtype=torch.int32, device=dev)
  lens = torch.tensor([4, 4, 4, 3], dtype=torch.int32, device=dev)
  ref = torch.tensor([[a, a, a, a]] * 4, dtype=torch.int32, device=dev)
  rl = torch.tensor([4, 4, 4, 5], dtype=torch.int32, device=dev)
  out = {k: v.cpu().tolist() for k, v in sc.score(ids, lens, ref, rl).items()}
  assert out["status"] == [0, -1, -1, -2]
  assert out["distance"] == [0, 0, 0, 0] and out["ref_len"] == [4, 0, 0, 0]
  res = sc.result()
  assert (res["pairs"], res["ref_len"], res["distance"]) == (1, 4, 0)


def test_a_pair_scores_the_same_alone_and_inside_larger_batches(dev):
  from lipreading_amd.scoring import EditScorer
  rng = random.Random(17)
  sp = special_classes(LABELS)
  refs = [random_ids(rng, len(LABELS), rng.randint(0, 48), sp) for _ in range(1000)]
  hyps = [mutated(rng, r, len(LABELS), rng.randint(0, 64)) if k % 3 else random_ids(rng, len(LABELS), rng.randint(0, 64), sp)
          for k, r in enumerate(refs)]
  sc = EditScorer(LABELS)
  h, hl = pack(hyps, 64, dev)
  r, rl = pack(refs, 48, dev)
  for unit, al in (("char", True), ("word", False)):
    big = torch.stack([sc.score(h, hl, r, rl, unit=unit, align=al)[f] for f in ("status",) + FIELDS], 1)
    mid = torch.stack([sc.score(h[:64], hl[:64], r[:64], rl[:64], unit=unit, align=al)[f] for f in ("status",) + FIELDS], 1)
    one = torch.cat([torch.stack([sc.score(h[k:k + 1], hl[k:k + 1], r[k:k + 1], rl[k:k + 1], unit=unit, align=al)[f]
                                  for f in ("status",) + FIELDS], 1) for k in range(64)])
    assert torch.equal(one, mid) and torch.equal(one, big[:64])
    rows = want_rows(hyps, refs, LABELS, unit, al)[0]
    check({f: big[:, i].cpu().tolist() for i, f in enumerate(("status",) + FIELDS)}, rows)


def test_totals_and_confusion_accumulate_and_the_gate_holds_them(dev):
  from lipreading_amd.scoring import EditScorer
  rng = random.Random(23)
  sp = special_classes(LABELS)
  sc = EditScorer(LABELS)
  sums = {u: dict.fromkeys(FIELDS + ("pairs",), 0) for u in ("char", "word")}
  all_steps = []
  for call in range(3):
    refs = [random_ids(rng, len(LABELS), rng.randint(0, 40), sp) for _ in range(20 + call)]
    hyps = [mutated(rng, r, len(LABELS), rng.randint(0, 50)) for r in refs]
    for unit, al in (("char", True), ("word", False)):
      got = run(sc, hyps, refs, dev, unit, al)
      rows, steps = want_rows(hyps, refs, LABELS, unit, al)
      check(got, rows)
      for f in FIELDS:
        sums[unit][f] += sum(got[f])
      sums[unit]["pairs"] += len(refs)
      all_steps += steps
  res = sc.result()
  for f in FIELDS + ("pairs",):
    assert res[f] == sums["char"][f], f
  for f in ("distance", "ref_len", "hyp_len", "pairs"):
    assert res["word_" + f] == sums["word"][f], f
  assert res["cer"] == sums["char"]["distance"] / sums["char"]["ref_len"]
  assert res["wer"] == sums["word"]["distance"] / sums["word"]["ref_len"]
  conf = sc.confusion()[0].cpu()
  K = sc.K
  assert conf.tolist() == confusion_ref(all_steps, sc.symbols)
  assert int(conf.sum()) == res["hits"] + res["sub"] + res["ins"] + res["dele"]
  assert int(conf[:K].sum()) == res["ref_len"] and int(conf[:, :K].sum()) == res["hyp_len"]
  # a non-zero gate word: per-pair outputs as before, totals and confusion matrix untouched
  gate = torch.tensor([-1], dtype=torch.int32, device=dev)
  for unit, al in (("char", True), ("word", False)):
    check(run(sc, hyps, refs, dev, unit, al, gate=gate), want_rows(hyps, refs, LABELS, unit, al)[0])
  assert sc.result() == res and torch.equal(sc.confusion()[0].cpu(), conf)
  # and a zero gate word lets them through
  gate.zero_()
  run(sc, hyps, refs, dev, "char", True, gate=gate)
  assert sc.result()["pairs"] == res["pairs"] + len(refs)
  sc.reset()
  assert sc.result()["pairs"] == 0 and int(sc.confusion()[0].sum()) == 0


# ---- the loops ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
  """A small encoder (CTC head) + attention decoder trained briefly on the synthetic nano dataview, its loader
  (3 batches of 4), and an UNTRAINED encoder of the same shape.  The synthetic landmarks are noise, so the trained CTC
  head collapses to the blank (empty transcripts, CER exactly 1) while the attention decoder memorises the captions
  (about a quarter of the characters wrong); the untrained head emits long wrong transcripts.  Between them the
  comparisons see empty, partly right and garbage hypotheses."""
  from lipreading_amd import dataset as DS
  from lipreading_amd import train as T
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  root = str(tmp_path_factory.mktemp("edit"))
  DS.write_synthetic_dataview(root, "synthetic/nano", n_videos=3, captions_per_video=6, seed=1)
  tr, _, _ = DS.split_dataset(root, "synthetic/nano", 0.8, np.random.RandomState(123456))
  ds = DS.FrameCaptionDataset(root, "synthetic/nano", "train", tr)
  loader = DS.make_loader(ds, 4, make_collate_fn(dev))
  assert len(loader) >= 3
  torch.manual_seed(123456)
  enc = VideoEncoder(204, 64, rnn_type="GRU", bidirectional=True, enable_ctc=True, vocab_size=len(ds.char2idx),
                     char2idx=ds.char2idx).to(dev)
  dec = CharDecodingStep(enc, char_dim=16, vocab_size=len(ds.char2idx), char2idx=ds.char2idx,
                         attention_type="1_layer_nn").to(dev)
  opt = (FusedAdam(FlatParameters(enc), lr=4e-3), FusedAdam(FlatParameters(dec), lr=4e-3))
  for _ in range(40):
    T.train(enc, dec, loader, opt, dev, ds.char2idx, grad_norm=50)
  torch.manual_seed(99)
  raw = VideoEncoder(204, 64, rnn_type="GRU", bidirectional=True, enable_ctc=True, vocab_size=len(ds.char2idx),
                     char2idx=ds.char2idx).to(dev)
  return enc, dec, loader, ds.char2idx, raw


def host_wer(enc, loader, dev, char2idx):
  """Sum of Decoder.wer over the host's greedy strings / reference word count."""
  from lipreading_amd.decoder import GreedyDecoder, ctc_labels
  dec = GreedyDecoder(ctc_labels(char2idx))
  inv = {v: k for k, v in char2idx.items()}
  dist = words = 0
  enc.eval()
  with torch.no_grad():
    for frames, frame_lens, chars, char_lens in loader:
      lp, _, _ = enc(frames.to(dev), frame_lens.to(dev), max_len=int(frame_lens.max()))
      strings, _ = dec.decode(lp, frame_lens.to(dev))
      for b in range(len(strings)):
        ref = ''.join(inv[int(c)] for c in chars[b, 1:int(char_lens[b]) - 1])
        dist += dec.wer(strings[b][0].replace(EOS, ''), ref)
        words += len(ref.split())
  return dist / max(words, 1)


def test_device_loops_equal_the_host_loops(dev, trained):
  from lipreading_amd import train as T
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  enc, dec, loader, c2i, raw = trained
  n = len(loader)
  beam = BeamCTCDecoder(ctc_labels(c2i), beam_width=16, cutoff_top_n=8, log_probs_input=True)
  for name, e in (("trained", enc), ("untrained", raw)):
    scores = T.device_scores(e, loader, dev, c2i)
    print("greedy, %s encoder: %r" % (name, scores))
    assert T.last_device_score_stats == {"batches": n, "gated": 0, "rescored": 0}
    assert scores["cer"] == T.greedy_cer(e, loader, dev, c2i)
    assert T.device_cer(e, loader, dev, c2i) == scores["cer"]
    assert scores["wer"] == host_wer(e, loader, dev, c2i)
    assert scores["pairs"] == scores["word_pairs"] == sum(len(b[3]) for b in loader)
    got = T.device_scores(e, loader, dev, c2i, decoder=beam, units=('char',))
    print("ctc beam, %s encoder: %r" % (name, got))
    assert got["cer"] == T.ctc_cer(e, loader, dev, c2i, beam)
    assert T.device_cer(e, loader, dev, c2i, decoder=beam) == got["cer"]
    if name == "untrained":
      assert scores["hyp_len"] > 0 and got["hyp_len"] > 0 and scores["distance"] > 0    # transcripts to score at all
  for w in (0.0, 0.3):
    got = T.device_scores(enc, loader, dev, c2i, decoding_step=dec, beam_width=4, max_label_len=60, ctc_weight=w,
                          units=('char',))
    print("attention, ctc_weight %.1f: %r" % (w, got))
    assert got["cer"] == T.attention_cer(enc, dec, loader, dev, c2i, beam_width=4, max_label_len=60, ctc_weight=w)
    assert T.device_cer(enc, loader, dev, c2i, decoding_step=dec, beam_width=4, max_label_len=60,
                        ctc_weight=w) == got["cer"]
    if w == 0.0:
      # neither a perfect nor a useless transcript: the comparison bites
      assert 0 < got["distance"] < got["ref_len"]


def test_a_gated_batch_is_rescored_once(dev, trained, monkeypatch):
  """The re-score path without any fault on the GPU: the host-side function that exports the fault word writes a
  non-zero word behind the export for batch 1 (a plain device store), so lr_edit_distance gates that batch out, the
  gate vector records it, and after the one read exactly that batch is encoded again with recurrence='f32'.  The host
  loop gets the same treatment through its own reader (_fault_keep), so both re-decode batch 1 the same way."""
  from lipreading_amd import train as T
  _, _, loader, c2i, enc = trained      # the untrained encoder: non-empty transcripts
  before = enc.recurrence
  assert before != 'f32'
  seen = {"gate": 0, "keep": 0, "regated": []}
  real_gate, real_keep, real_batch = T._fault_gate, T._fault_keep, T._device_batch

  def gate(flag2):
    g = real_gate(flag2)
    if seen["gate"] == 1:
      flag2[1] = -1
    seen["gate"] += 1
    return g

  def keep(flag2):
    k = real_keep(flag2)
    seen["keep"] += 1
    return torch.zeros_like(k) if seen["keep"] == 2 else k

  def batch(ctx, k, *a, **kw):
    if kw.get("gated") is False:
      seen["regated"].append((k, getattr(ctx.encoder, "recurrence", None)))
    return real_batch(ctx, k, *a, **kw)

  monkeypatch.setattr(T, "_fault_gate", gate)
  monkeypatch.setattr(T, "_fault_keep", keep)
  monkeypatch.setattr(T, "_device_batch", batch)
  got = T.device_scores(enc, loader, dev, c2i)
  assert T.last_device_score_stats == {"batches": len(loader), "gated": 1, "rescored": 1}
  assert seen["regated"] == [(1, 'f32')]
  assert got["pairs"] == sum(len(b[3]) for b in loader)
  want = T.greedy_cer(enc, loader, dev, c2i)
  assert seen["keep"] == len(loader)
  assert got["cer"] == want
  assert enc.recurrence == before


@pytest.mark.parametrize("arm", ["greedy", "ctc_beam", "attention", "joint"])
def test_every_host_loop_retries_a_timed_out_batch_once(dev, trained, monkeypatch, arm):
  """greedy_cer, ctc_cer and attention_cer (plain and joint) share one retry: with the host-side reader of the fault
  word answering 'timed out' for batch 1 (no fault on the GPU, as above), each reads the word once per batch, runs
  exactly batch 1 again with recurrence='f32', restores the mode, and returns the CER of a by-hand loop that encodes
  batch 1 on the per-step kernels."""
  from lipreading_amd import analysis, train as T
  from lipreading_amd import decoder as D
  trained_enc, step, loader, c2i, raw = trained
  inv = {v: k for k, v in c2i.items()}
  attn = dict(beam_width=4, max_label_len=60, ctc_weight=0.3 if arm == "joint" else 0.0)
  if arm in ("greedy", "ctc_beam"):
    enc = raw                            # the untrained encoder: non-empty transcripts
    ctc = (D.GreedyDecoder(D.ctc_labels(c2i), blank_index=0) if arm == "greedy" else
           D.BeamCTCDecoder(D.ctc_labels(c2i), beam_width=16, cutoff_top_n=8, log_probs_input=True))
    loop = ((lambda: T.greedy_cer(enc, loader, dev, c2i)) if arm == "greedy" else
            (lambda: T.ctc_cer(enc, loader, dev, c2i, ctc)))
  else:
    enc = trained_enc
    loop = lambda: T.attention_cer(enc, step, loader, dev, c2i, **attn)   # noqa: E731
  before = enc.recurrence
  assert before != 'f32'
  seen = {"keep": 0, "modes": []}
  real_keep, real_fwd = T._fault_keep, enc.forward

  def keep(flag2):
    k = real_keep(flag2)
    seen["keep"] += 1
    return torch.zeros_like(k) if seen["keep"] == 2 else k

  def fwd(*a, **kw):
    seen["modes"].append(enc.recurrence)
    return real_fwd(*a, **kw)

  monkeypatch.setattr(T, "_fault_keep", keep)
  monkeypatch.setattr(enc, "forward", fwd)
  got = loop()
  n = len(loader)
  assert seen["keep"] == n
  assert seen["modes"] == [before, before, 'f32'] + [before] * (n - 2)
  assert enc.recurrence == before
  monkeypatch.undo()

  dist = total = 0
  enc.eval()
  step.eval()
  with torch.no_grad():
    for k, (frames, frame_lens, chars, char_lens) in enumerate(loader):
      enc.recurrence = 'f32' if k == 1 else before
      try:
        lens_d = frame_lens.to(dev)
        out = enc(frames.to(dev), lens_d, max_len=int(frame_lens.max()))
      finally:
        enc.recurrence = before
      if arm in ("greedy", "ctc_beam"):
        hyps = [s[0].replace(EOS, '') for s in ctc.decode(out[0], lens_d)[0]]
      else:
        best = analysis.best_ids(step, out[1], lens_d, out[2], attn["beam_width"], attn["max_label_len"],
                                 ctc_log_probs=out[0] if arm == "joint" else None, ctc_weight=attn["ctc_weight"])
        hyps = [''.join(inv[i] for i in h if i != c2i[EOS]) for h in best]
      for b, hyp in enumerate(hyps):
        ref = ''.join(inv[int(c)] for c in chars[b, 1:int(char_lens[b]) - 1]).replace(' ', '')
        dist += D._edit_distance(hyp.replace(' ', ''), ref)
        total += len(ref)
  print("%s: cer %r (%d / %d)" % (arm, got, dist, total))
  assert total > 0 and got == dist / total


def test_driver_error_with_device_scoring_equals_host_scoring(dev, trained):
  from lipreading_amd import driver
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  trained_enc, dec, loader, c2i, raw = trained
  beam = BeamCTCDecoder(ctc_labels(c2i), beam_width=8, cutoff_top_n=8, log_probs_input=True)
  for flags, step, ctc in ((["--ctc_only=True", "--enable_ctc=True"], None, None),
                           (["--ctc_only=True", "--enable_ctc=True", "--ctc_decoder=beam"], None, beam),
                           (["--attn_decode=beam", "--attn_beam_width=3", "--attn_max_label_len=50"], dec, None),
                           (["--enable_ctc=True", "--attn_decode=joint", "--attn_beam_width=3",
                             "--attn_max_label_len=50"], dec, None),
                           (["--enable_ctc=True"], dec, None)):     # teacher forcing: not an edit distance, untouched
    enc = raw if step is None else trained_enc   # the CTC errors on non-empty transcripts
    host = driver.make_error_of(driver.parse_flags(flags), enc, step, ctc, dev, c2i)
    devi = driver.make_error_of(driver.parse_flags(flags + ["--score=device"]), enc, step, ctc, dev, c2i)
    if "--attn_decode" not in ' '.join(flags) and step is not None:
      torch.manual_seed(7)
      a = host(loader)
      torch.manual_seed(7)
      assert devi(loader) == a and devi.last_scores is None
      continue
    assert devi(loader) == host(loader), flags
    assert host.last_scores is None and 0.0 <= devi.last_scores["wer"]


def test_confusion_matrix_equals_the_restatement(dev, trained):
  from lipreading_amd import analysis
  from lipreading_amd.decoder import GreedyDecoder, ctc_labels
  _, _, loader, c2i, enc = trained      # the untrained encoder: non-empty transcripts
  labels = ctc_labels(c2i)
  dec = GreedyDecoder(labels)
  steps = []
  enc.eval()
  with torch.no_grad():
    for frames, frame_lens, chars, char_lens in loader:
      lp, _, _ = enc(frames.to(dev), frame_lens.to(dev), max_len=int(frame_lens.max()))
      ids, _, lens = dec.decode_ids(lp, frame_lens.to(dev))
      ids, lens = ids.cpu().tolist(), lens.cpu().tolist()
      for b in range(len(lens)):
        ref = [int(c) + 1 for c in chars[b, 1:int(char_lens[b]) - 1]]
        steps.append(score_ref(ids[b][:lens[b]], ref, labels)[1])
  names = analysis.VISEME_ORDER
  assert sorted(names) == list("abcdefghijklmnopqrstuvwxyz")
  want = np.zeros((26, 26), dtype=np.int64)
  for st in steps:
    for r, h in st:
      if r in names and h in names:
        want[names.index(r), names.index(h)] += 1
  got = analysis.confusion_matrix(enc, loader, dev, c2i)
  assert got.shape == (26, 26) and got.dtype == np.int64
  assert (got == want).all() and got.sum() > 0
  cut = analysis.confusion_matrix(enc, loader, dev, c2i, class_names=['e', 'a', '~'])
  assert (cut[:2, :2] == want[np.ix_([1, 0], [1, 0])]).all() and cut[2].sum() == 0 and cut[:, 2].sum() == 0


def test_no_host_read_per_batch(dev, trained, monkeypatch):
  """The batch body of device_scores — from after the batch's upload to after the scoring launches — under torch's
  sync debug mode 'error', for the greedy and the CTC beam paths.  (The attention searches poll the device for
  completion by design; for them the claim is only that scoring adds no read of its own.)"""
  from lipreading_amd import train as T
  from lipreading_amd.decoder import BeamCTCDecoder, ctc_labels
  _, _, loader, c2i, enc = trained
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
    pytest.skip("this torch build does not honour set_sync_debug_mode('error') on ROCm: see the copy counts of the "
                "rocprofv3 traces in DESIGN.md §17")
  real = T._device_batch
  bodies = []

  def guarded(*a, **kw):
    torch.cuda.set_sync_debug_mode("error")
    try:
      real(*a, **kw)
    finally:
      torch.cuda.set_sync_debug_mode("default")
    bodies.append(1)

  monkeypatch.setattr(T, "_device_batch", guarded)
  want = T.greedy_cer(enc, loader, dev, c2i)
  assert T.device_cer(enc, loader, dev, c2i) == want
  beam = BeamCTCDecoder(ctc_labels(c2i), beam_width=16, cutoff_top_n=8, log_probs_input=True)
  T.device_scores(enc, loader, dev, c2i, decoder=beam)
  assert len(bodies) == 2 * len(loader)


def test_driver_epoch_with_device_scoring_reports_val_wer(dev, tmp_path):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/micro", n_videos=10, captions_per_video=6, seed=7)
  common = ["--root=" + root, "--data=synth/micro", "--batch_size=8", "--enable_ctc=True", "--ctc_only=True",
            "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=1"]
  out = driver.run(**driver.parse_flags(common + ["--score=device"]))
  (epoch,) = out["history"]
  assert 0.0 <= epoch["val_wer"] and np.isfinite(epoch["val_cer"]) and np.isfinite(epoch["train_cer"])
  host = driver.run(**driver.parse_flags(common))
  assert "val_wer" not in host["history"][0]
