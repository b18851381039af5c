"""CPU: the ARPA reader (lipreading_amd/lm.py), a float64 lm_score written from the backoff formula, and beam_lm_ref,
a float64 restatement of lr_ctc_beam_lm_decode's specification (lipreading_amd/csrc/lr_ctc_beam.hip) checked
against exhaustive enumeration; then the host-side rejections of BeamCTCDecoder, the C ABI and the driver (no
device needed).  tests/test_gpu_beam_lm.py holds the GPU against this restatement."""
import collections
import ctypes
import gzip
import itertools
import math

import numpy as np
import pytest

from tests.test_beam_cpu import enumerate_labellings, prune, softmax_frames

NEG_INF = -np.inf
LN10 = math.log(10.0)
OOV = -1000.0
SPECIAL = ("<s>", "</s>", "<unk>")

TOY = """some header text lmplz would not write
\\data\\
ngram 1=6
ngram 2=5
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-2.0\t</s>
-1.5\t<unk>
-0.7\ta\t-0.3
-0.9\tab\t-0.2
-1.2\tbb

\\2-grams:
-0.4\t<s> a\t-0.1
-0.6\ta ab\t-0.25
-0.5\tab bb\t-0.35
-0.8\ta a
-1.1\t<s> bb

\\3-grams:
-0.2\t<s> a ab
-0.05\tab bb a

\\end\\
"""


# ------------------------------------------------------------------------------------------------------------------
# the specification's LM term, straight from the backoff formula
# ------------------------------------------------------------------------------------------------------------------
class RefLM(object):
  """ARPA tables as dicts of word-string tuples: float64, log10."""

  def __init__(self, model):
    self.order = model.order
    self.vocab = set(model.vocab)
    self.p, self.bow = {}, {}
    row, at = 0, 0
    for k, cnt in enumerate(model.counts, 1):
      for _ in range(cnt):
        key = tuple(model.vocab[w] for w in model.words[at:at + k])
        self.p[key] = float(model.log10_prob[row])
        self.bow[key] = float(model.log10_backoff[row])
        row += 1
        at += k

  def log10p(self, ctx, w):
    if ctx + (w,) in self.p:
      return self.p[ctx + (w,)]
    return self.bow.get(ctx, 0.0) + self.log10p(ctx[1:], w)

  def lm_score(self, prev, w):
    """lm(w | ctx): ctx = the last order-1 words of `prev`, padded with <s>; OOV = -1000 (no ln 10)."""
    m = self.order - 1
    ctx = (("<s>",) * m + tuple(prev))[len(prev):] if m else ()
    if w not in self.vocab or any(c not in self.vocab for c in ctx):
      return OOV
    return LN10 * self.log10p(ctx, w)


def load(path):
  from lipreading_amd.lm import read_arpa
  return RefLM(read_arpa(path))


# ------------------------------------------------------------------------------------------------------------------
# beam_lm_ref: the restatement
# ------------------------------------------------------------------------------------------------------------------
def roles_of(labels, blank=0):
  return [2 if l == " " else (1 if len(l) == 1 and i != blank else 0) for i, l in enumerate(labels)]


class Dict(object):
  """The vocabulary trie over class ids: child[node, class] (-1 = leaves the vocabulary), word[node]."""

  def __init__(self, lm, labels, blank=0):
    roles = roles_of(labels, blank)
    cls_of = {l: i for i, l in enumerate(labels) if roles[i] == 1}
    nodes = {"": 0}
    edges = []
    words = {}
    for w in sorted(lm.vocab):
      if w in SPECIAL or any(ch not in cls_of for ch in w):
        continue
      for j in range(1, len(w) + 1):
        if w[:j] not in nodes:
          nodes[w[:j]] = len(nodes)
          edges.append((nodes[w[:j - 1]], cls_of[w[j - 1]], nodes[w[:j]]))
      words[nodes[w]] = w
    self.child = np.full((len(nodes), len(labels)), -1, np.int64)
    for a, c, b in edges:
      self.child[a, c] = b
    self.word = [None] * len(nodes)
    for nd, w in words.items():
      self.word[nd] = w
    self.prefixes = set(nodes)
    self.roles = roles


def beam_lm_ref(v, size, beam_width, cutoff_top_n, lm, dic, alpha, beta, cutoff_prob=1.0, blank=0,
                log_input=False):
  """beam_ref of tests/test_beam_cpu.py plus the LM: per hypothesis (trie node, completed words, cached term of the
  current word).  Returns [(ids, offsets, -(log mass + final term))], best first."""
  roles = dic.roles

  def term(node, ctx):
    return alpha * lm.lm_score(ctx, dic.word[node]) + beta if node else 0.0

  # (prefix, log p_blank, log p_nonblank, offsets, node, completed words, term)
  beam = [((), 0.0, NEG_INF, (), 0, (), 0.0)]
  for t in range(size):
    keep, lp = prune(v[t], cutoff_top_n, cutoff_prob, log_input)
    c2k = {int(c): k for k, c in enumerate(keep)}
    W = len(beam)
    pb = np.array([h[1] for h in beam])
    pnb = np.array([h[2] for h in beam])
    score = np.logaddexp(pb, pnb)
    last = np.array([h[0][-1] if h[0] else -1 for h in beam])
    own_pb = score + lp[c2k[blank]] if blank in c2k else np.full(W, NEG_INF)
    own_pnb = np.full(W, NEG_INF)
    for i in range(W):
      if last[i] in c2k:
        own_pnb[i] = pnb[i] + lp[c2k[int(last[i])]]
    ext = np.where(keep[None, :] == last[:, None], pb[:, None], score[:, None]) + lp[None, :]
    ext[:, keep == blank] = NEG_INF
    # the LM: terms on space extensions, the dictionary on word-character extensions
    kr = np.array([roles[int(c)] for c in keep])
    nodes = np.array([h[4] for h in beam])
    child = dic.child[nodes][:, keep]
    ext = np.where((kr[None, :] == 1) & (child < 0), NEG_INF, ext)
    ext = ext + np.where(kr[None, :] == 2, np.array([h[6] for h in beam])[:, None], 0.0)
    rank = {h[0]: i for i, h in enumerate(beam)}
    for q, h in enumerate(beam):
      if h[0] and h[0][-1] in c2k and h[0][:-1] in rank:
        i, k = rank[h[0][:-1]], c2k[h[0][-1]]
        own_pnb[q] = np.logaddexp(own_pnb[q], ext[i, k])
        ext[i, k] = NEG_INF
    own = np.logaddexp(own_pb, own_pnb)
    sc = np.concatenate([own, ext.ravel()])
    par = np.concatenate([np.arange(W), np.repeat(np.arange(W), len(keep))])
    tb = np.concatenate([np.zeros(W, np.int64), np.tile(1 + keep.astype(np.int64), W)])
    valid = np.nonzero(sc > NEG_INF)[0]
    order = valid[np.lexsort((tb[valid], par[valid], -sc[valid]))][:beam_width]
    nxt = []
    for s in order:
      i = int(par[s])
      pre, _, _, off, node, ctx, tm = beam[i]
      if s < W:
        nxt.append((pre, own_pb[i], own_pnb[i], off, node, ctx, tm))
        continue
      c = int(keep[(s - W) % len(keep)])
      if roles[c] == 1:
        nd = int(dic.child[node, c])
        nxt.append((pre + (c,), NEG_INF, sc[s], off + (t,), nd, ctx, term(nd, ctx)))
      else:   # a space completes a non-empty word; a transparent class drops the run
        ctx2 = ctx + (dic.word[node] or "\0oov",) if roles[c] == 2 and node else ctx
        nxt.append((pre + (c,), NEG_INF, sc[s], off + (t,), 0, ctx2, 0.0))
    beam = nxt
  fin = [float(np.logaddexp(h[1], h[2])) + h[6] for h in beam]
  order = sorted(range(len(beam)), key=lambda r: (-fin[r], r))
  return [(beam[r][0], beam[r][3], -fin[r]) for r in order]


def enumerate_lm(v, labels, lm, dic, alpha, beta, log_input=False, blank=0):
  """Every labelling that stays in the dictionary, scored ln P_ctc + sum(alpha * lm + beta) over its completed words
  and its final word: [(labelling, -score)] best first."""
  out = []
  for lab, nlp in enumerate_labellings(v, log_input, blank):
    s, ok = -nlp, True
    done, run = [], ""
    for c in lab:
      l = labels[c]
      if l == " ":
        if run:
          s += alpha * lm.lm_score(done, run if run in lm.vocab and run not in SPECIAL else "\0oov") + beta
          done.append(run if run in lm.vocab else "\0oov")
        run = ""
      elif len(l) == 1 and c != blank:
        run += l
        if run not in dic.prefixes:
          ok = False
          break
      else:
        run = ""
    if not ok:
      continue
    if run:
      s += alpha * lm.lm_score(done, run if run in lm.vocab and run not in SPECIAL else "\0oov") + beta
    out.append((lab, -s))
  return sorted(out, key=lambda kv: kv[1])


# ------------------------------------------------------------------------------------------------------------------
# a small absolute-discounting ARPA writer for synthetic corpora
# ------------------------------------------------------------------------------------------------------------------
def write_arpa(path, sentences, order, discount=0.5):
  """Interpolated absolute discounting, written as ARPA backoff: P(w|h) = max(c(hw)-D, 0)/c(h) + l(h) P(w|h[1:]) for
  listed (h, w), backoff(h) = l(h) = D * N1+(h.) / c(h).  Unigrams add one over the vocabulary; <s> is -99."""
  grams = [collections.Counter() for _ in range(order + 1)]
  for s in sentences:
    toks = ["<s>"] + list(s) + ["</s>"]
    for k in range(1, order + 1):
      for j in range(len(toks) - k + 1):
        grams[k][tuple(toks[j:j + k])] += 1
  vocab = sorted({w for (w,) in grams[1]} | {"<unk>"})
  total = sum(c for (w,), c in grams[1].items() if w != "<s>")
  logp = {}
  for w in vocab:
    logp[(w,)] = -99.0 if w == "<s>" else math.log10((grams[1].get((w,), 0) + 1.0) / (total + len(vocab)))
  ctx_count, ctx_types, bow = collections.Counter(), collections.Counter(), {}
  for k in range(2, order + 1):
    for g, c in grams[k].items():
      ctx_count[g[:-1]] += c
      ctx_types[g[:-1]] += 1
  for h in ctx_count:
    bow[h] = math.log10(discount * ctx_types[h] / ctx_count[h])

  def lower(h, w):
    if h + (w,) in logp:
      return 10.0 ** logp[h + (w,)]
    return 10.0 ** bow.get(h, 0.0) * lower(h[1:], w)

  for k in range(2, order + 1):
    for g in sorted(grams[k]):
      h, w = g[:-1], g[-1]
      logp[g] = math.log10(max(grams[k][g] - discount, 0.0) / ctx_count[h] + 10.0 ** bow[h] * lower(h[1:], w))
  with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
    f.write("\\data\\\n")
    keys = [[(w,) for w in vocab]] + [sorted(grams[k]) for k in range(2, order + 1)]
    for k in range(1, order + 1):
      f.write("ngram %d=%d\n" % (k, len(keys[k - 1])))
    for k in range(1, order + 1):
      f.write("\n\\%d-grams:\n" % k)
      for g in keys[k - 1]:
        f.write("%.7f\t%s" % (logp[g], " ".join(g)))
        if g in bow and k < order:
          f.write("\t%.7f" % bow[g])
        f.write("\n")
    f.write("\n\\end\\\n")
  return path


def pseudo_corpus(seed, n_words=3000, n_sent=4000, alphabet="abcdefghijklmnopqrstuvwxyz", zipf=1.2):
  """A seeded corpus of lower-case pseudo-words, Zipf-distributed."""
  rng = np.random.default_rng(seed)
  words = set()
  while len(words) < n_words:
    words.add("".join(rng.choice(list(alphabet), int(rng.integers(1, 8)))))
  words = sorted(words)
  rng.shuffle(words)
  p = 1.0 / np.arange(1, len(words) + 1) ** zipf
  p /= p.sum()
  sents = []
  for _ in range(n_sent):
    sents.append([words[i] for i in rng.choice(len(words), int(rng.integers(2, 12)), p=p)])
  return words, sents


# ------------------------------------------------------------------------------------------------------------------
# the ARPA reader
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def toy(tmp_path):
  p = tmp_path / "toy.arpa"
  p.write_text(TOY)
  return str(p)


def test_reader_values_and_missing_backoffs(toy):
  from lipreading_amd.lm import read_arpa
  m = read_arpa(toy)
  assert m.order == 3 and m.counts == [6, 5, 2]
  assert m.vocab == ["<s>", "</s>", "<unk>", "a", "ab", "bb"]
  assert m.words[:6].tolist() == list(range(6))
  assert m.words[6:8].tolist() == [0, 3]                 # <s> a
  assert m.words[-3:].tolist() == [4, 5, 3]              # ab bb a
  np.testing.assert_array_equal(m.log10_prob[:6], [-99, -2.0, -1.5, -0.7, -0.9, -1.2])
  np.testing.assert_array_equal(m.log10_backoff[:6], [-0.5, 0, 0, -0.3, -0.2, 0])
  np.testing.assert_array_equal(m.log10_backoff[6:11], [-0.1, -0.25, -0.35, 0, 0])
  np.testing.assert_array_equal(m.log10_prob[11:], [-0.2, -0.05])


def test_reader_gz(toy, tmp_path):
  from lipreading_amd.lm import read_arpa
  gz = tmp_path / "toy.arpa.gz"
  with gzip.open(gz, "wt") as f:
    f.write(TOY)
  a, b = read_arpa(toy), read_arpa(str(gz))
  assert a.vocab == b.vocab and a.counts == b.counts
  np.testing.assert_array_equal(a.words, b.words)
  np.testing.assert_array_equal(a.log10_prob, b.log10_prob)


@pytest.mark.parametrize("edit,match", [
    (lambda s: s.replace("\\data\\\n", ""), "no .data. section"),
    (lambda s: s.replace("\\end\\\n", ""), "no .end."),
    (lambda s: s.replace("ngram 2=5", "ngram 2=6"), "holds 5 entries, .data. declares 6"),
    (lambda s: s.replace("-1.1\t<s> bb\n", "-1.1\t<s> bb\n-1.3\ta ab\n").replace("ngram 2=5", "ngram 2=6"),
     "duplicate 2-gram"),
    (lambda s: s.replace("-0.05\tab bb a", "-0.05\tbb ab a"), "context 'bb ab' of this 3-gram is not listed"),
    (lambda s: s.replace("ngram 3=2\n", "ngram 3=2\nngram 4=0\nngram 5=0\nngram 6=0\nngram 7=0\n"),
     "order 7 > 6"),
    (lambda s: s.replace("-0.8\ta a", "-0.8\ta zz"), "not a unigram"),
])
def test_reader_rejections(tmp_path, edit, match):
  from lipreading_amd.lm import read_arpa
  p = tmp_path / "bad.arpa"
  p.write_text(edit(TOY))
  with pytest.raises(ValueError, match=match) as e:
    read_arpa(str(p))
  assert ":%s" % "" in str(e.value) and str(p) in str(e.value)   # names the file and a line


def test_reader_names_the_line(tmp_path):
  from lipreading_amd.lm import read_arpa
  p = tmp_path / "bad.arpa"
  lines = TOY.split("\n")
  bad = lines.index("-0.05\tab bb a") + 1
  p.write_text(TOY.replace("-0.05\tab bb a", "-0.05\tbb ab a"))
  with pytest.raises(ValueError, match=":%d:" % bad):
    read_arpa(str(p))


def test_kenlm_binary_and_non_arpa_paths_raise_not_implemented(tmp_path, toy):
  from lipreading_amd.decoder import BeamCTCDecoder
  labels = ["_", " ", "a", "b"]
  for name in ("lm.binary", "lm.bin", "lm.trie", "lm.arpa.bz2"):
    with pytest.raises(NotImplementedError, match="KenLM.*ARPA"):
      BeamCTCDecoder(labels, lm_path=str(tmp_path / name))   # decided before the (absent) file is opened
  fake = tmp_path / "really_binary.arpa"
  fake.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\0\0\0")
  with pytest.raises(NotImplementedError, match="KenLM.*ARPA"):
    BeamCTCDecoder(labels, lm_path=str(fake))
  dec = BeamCTCDecoder(labels, lm_path=toy, alpha=0.5, beta=1.0)
  assert dec.lm.order == 3 and dec.alpha == 0.5 and dec.beta == 1.0


# ------------------------------------------------------------------------------------------------------------------
# lm_score against values worked out by hand
# ------------------------------------------------------------------------------------------------------------------
def test_lm_score_by_hand(toy):
  lm = load(toy)
  cases = [
      ((), "a", -0.4),                      # (<s> <s> a) no; (<s> <s>) no -> 0; (<s> a) -0.4
      (("a",), "ab", -0.2),                 # (<s> a ab) listed
      (("a", "ab"), "bb", -0.25 - 0.5),     # backoff(a ab) + (ab bb)
      (("a", "ab"), "a", -0.25 - 0.2 - 0.7),   # backoff(a ab) + backoff(ab) + P(a): a chain of two
      (("ab", "bb"), "a", -0.05),           # (ab bb a) listed
      (("bb",), "bb", -1.2),                # (<s> bb) listed, no backoff -> 0; (bb bb) no, bb no backoff; P(bb)
      (("a", "a"), "ab", -0.6),             # (a a) listed without backoff -> 0, then (a ab) -0.6
      (("bb", "a"), "bb", -0.3 - 1.2),      # (bb a) not listed -> 0; backoff(a) + P(bb)
  ]
  for prev, w, want10 in cases:
    assert abs(lm.lm_score(prev, w) - LN10 * want10) < 1e-12, (prev, w)
  assert lm.lm_score(("a",), "zz") == OOV              # OOV word
  assert lm.lm_score(("zz", "a"), "ab") == OOV         # OOV in the context
  assert lm.lm_score(("zz", "a", "ab"), "bb") == LN10 * (-0.25 - 0.5)   # only the last order-1 words count


# ------------------------------------------------------------------------------------------------------------------
# the restatement against exhaustive enumeration
# ------------------------------------------------------------------------------------------------------------------
LABELS = ["_", " ", "a", "b", "<EOS>"]


def two_gram(tmp_path):
  return write_arpa(str(tmp_path / "two.arpa"), [["a", "ab"], ["bb", "a"], ["ab"], ["a", "a", "bb"]], 2)


@pytest.mark.parametrize("which", ["toy3", "two2"])
@pytest.mark.parametrize("alpha,beta", [(0.0, 0.0), (0.5, 1.0), (1.0, -0.5), (2.0, 3.0)])
@pytest.mark.parametrize("T,seed", [(4, 0), (5, 1)])
@pytest.mark.parametrize("log_input", [False, True])
def test_restatement_matches_exhaustive_enumeration(tmp_path, toy, which, alpha, beta, T, seed, log_input):
  lm = load(toy if which == "toy3" else two_gram(tmp_path))
  dic = Dict(lm, LABELS)
  rng = np.random.default_rng(seed)
  p = softmax_frames(rng, T, len(LABELS))
  v = np.log(p) if log_input else p
  want = enumerate_lm(v, LABELS, lm, dic, alpha, beta, log_input)
  got = beam_lm_ref(v, T, len(want) + 5, len(LABELS), lm, dic, alpha, beta, log_input=log_input)
  assert len(got) == len(want)
  assert {g[0] for g in got} == {w[0] for w in want}
  ref = dict(want)
  for r, (ids, off, s) in enumerate(got):
    assert abs(s - ref[ids]) < 1e-9, (ids, s, ref[ids])
    assert len(off) == len(ids) and list(off) == sorted(off)
    sep = all(abs(want[r][1] - want[q][1]) > 1e-9 for q in (r - 1, r + 1) if 0 <= q < len(want))
    if sep:
      assert ids == want[r][0]


def test_enumeration_sees_the_language_model(toy):
  """The data of the exhaustive test exercise the feature: the dictionary drops labellings, spaces score words."""
  lm = load(toy)
  dic = Dict(lm, LABELS)
  p = softmax_frames(np.random.default_rng(0), 5, len(LABELS))
  plain = enumerate_labellings(p)
  a = enumerate_lm(p, LABELS, lm, dic, 0.0, 0.0)
  b = enumerate_lm(p, LABELS, lm, dic, 1.0, 2.0)
  assert len(a) < len(plain)
  assert not any(3 in lab[:1] and 2 in lab[1:2] for lab, _ in a)   # "ba" is no vocabulary prefix
  assert [x for x in a if x[0] == (2, 1, 3)][0][1] != [x for x in b if x[0] == (2, 1, 3)][0][1]


# ------------------------------------------------------------------------------------------------------------------
# host-side rejections
# ------------------------------------------------------------------------------------------------------------------
def test_constructor_rejections(toy, tmp_path):
  from lipreading_amd.decoder import BeamCTCDecoder
  with pytest.raises(ValueError, match="' '"):
    BeamCTCDecoder(["_", "a", "b"], lm_path=toy)
  with pytest.raises(ValueError, match="distinct"):
    BeamCTCDecoder(["_", " ", "a", "b", "a"], lm_path=toy)
  with pytest.raises(ValueError, match="distinct"):
    BeamCTCDecoder(["_", " ", "a", " "], lm_path=toy)
  with pytest.raises(ValueError, match="upper- vs lower-case"):
    BeamCTCDecoder(["_", " ", "A", "B"], lm_path=toy)
  with pytest.raises(ValueError, match="finite"):
    BeamCTCDecoder(["_", " ", "a", "b"], lm_path=toy, alpha=float("nan"))
  # without a language model nothing changes: alpha / beta are ignored, no label checks
  dec = BeamCTCDecoder(["_", "a", "a"], alpha=float("nan"), beta=2.0)
  assert dec.lm is None


def _pack(m, labels, **kw):
  from lipreading_amd import _C, lm as LM
  lib = _C.lib()
  roles = LM.class_roles(labels, 0)
  dw, off, cl = LM.dictionary(m, labels, roles)
  a = dict(order=m.order, counts=np.asarray(m.counts, np.int64), words=m.words, lp=m.log10_prob,
           bow=m.log10_backoff, bos=m.word_id.get("<s>", -1), dn=len(dw), dw=dw, off=off, cl=cl, C=len(labels))
  a.update(kw)
  vp = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
  nbytes = lib.lr_ctc_beam_lm_pack_bytes(a["order"], vp(a["counts"]), int(a["off"][-1]))
  out = np.empty(max(nbytes, 1 << 16), np.uint8)
  st = lib.lr_ctc_beam_lm_pack(vp(out), a.get("nbytes", out.size), a["order"], vp(a["counts"]), vp(a["words"]),
                               vp(a["lp"]), vp(a["bow"]), a["bos"], a["dn"], vp(a["dw"]), vp(a["off"]),
                               vp(a["cl"]), a["C"])
  return st, nbytes


def test_packer_limits_and_rejections(toy):
  from lipreading_amd import _C
  from lipreading_amd.lm import read_arpa
  lib = _C.lib()
  m = read_arpa(toy)
  st, nbytes = _pack(m, LABELS)
  assert st == _C.LR_OK and nbytes > 0
  assert _pack(m, LABELS, nbytes=16)[0] == _C.LR_ERR_WORKSPACE
  c7 = np.asarray([6, 5, 2, 0, 0, 0, 0], np.int64)
  assert lib.lr_ctc_beam_lm_pack_bytes(7, c7.ctypes.data_as(ctypes.c_void_p), 4) == 0
  assert _pack(m, LABELS, order=7, counts=c7)[0] == _C.LR_ERR_UNSUPPORTED
  big = np.asarray([1 << 24, 0], np.int64)
  assert lib.lr_ctc_beam_lm_pack_bytes(2, big.ctypes.data_as(ctypes.c_void_p), 4) == 0
  assert _pack(m, LABELS, order=2, counts=big)[0] == _C.LR_ERR_UNSUPPORTED
  # a duplicate n-gram and an unlisted prefix, passed straight to the packer
  w = m.words.copy()
  w[8:10] = w[6:8]                         # bigram 2 := bigram 0
  assert _pack(m, LABELS, words=w)[0] == _C.LR_ERR_INVALID_ARG
  w = m.words.copy()
  w[-3:] = [5, 4, 3]                       # (bb ab a): (bb ab) is not listed
  assert _pack(m, LABELS, words=w)[0] == _C.LR_ERR_INVALID_ARG
  assert _pack(m, LABELS, C=300)[0] == _C.LR_ERR_INVALID_ARG


def test_abi_rejects_bad_arguments_without_a_device():
  from lipreading_amd import _C
  lib = _C.lib()
  fake = ctypes.c_void_p(256)   # never dereferenced: every check below returns before any device call
  args = dict(probs=fake, sb=75 * 65, st=65, sizes=None, log_input=0, n=40, cp=1.0, W=100, blank=0, lm=fake,
              roles=fake, alpha=0.5, beta=1.0, ids=fake, off=fake, lens=fake, scores=fake, ws=fake, wsb=1 << 40,
              B=32, T=75, C=65)

  def call(**kw):
    a = dict(args, **kw)
    return lib.lr_ctc_beam_lm_decode(a["probs"], a["sb"], a["st"], a["sizes"], a["log_input"], a["n"], a["cp"],
                                     a["W"], a["blank"], a["lm"], a["roles"], a["alpha"], a["beta"], a["ids"],
                                     a["off"], a["lens"], a["scores"], a["ws"], a["wsb"], a["B"], a["T"], a["C"],
                                     None)

  for name in ("probs", "lm", "roles", "ids", "off", "lens", "scores", "ws"):
    assert call(**{name: None}) == _C.LR_ERR_INVALID_ARG, name
  for kw in (dict(B=0), dict(T=0), dict(C=0), dict(W=0), dict(n=0), dict(blank=65), dict(blank=-1),
             dict(cp=float("nan")), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(beta=float("-inf"))):
    assert call(**kw) == _C.LR_ERR_INVALID_ARG, kw
  for kw in (dict(W=129), dict(n=65), dict(C=257)):
    assert call(**kw) == _C.LR_ERR_UNSUPPORTED, kw
  assert call(wsb=16) == _C.LR_ERR_WORKSPACE


def test_driver_lm_flags():
  from lipreading_amd import driver
  f = driver.parse_flags([])
  assert f["lm_path"] == "" and f["lm_alpha"] == 0.0 and f["lm_beta"] == 0.0
  f = driver.parse_flags(["--ctc_decoder=beam", "--lm_path=x.arpa", "--lm_alpha=0.5", "--lm_beta=1"])
  assert f["lm_path"] == "x.arpa" and f["lm_alpha"] == 0.5 and f["lm_beta"] == 1.0
  with pytest.raises(SystemExit):
    driver.parse_flags(["--lm_path=x.arpa"])
  with pytest.raises(SystemExit):
    driver.parse_flags(["--ctc_decoder=greedy", "--lm_path=x.arpa"])


def test_synthetic_writer_is_a_readable_model(tmp_path):
  from lipreading_amd.lm import read_arpa
  words, sents = pseudo_corpus(3, n_words=200, n_sent=300)
  m = read_arpa(write_arpa(str(tmp_path / "s.arpa.gz"), sents, 3))
  assert m.order == 3 and m.counts[1] > 100 and m.counts[2] > 100
  lm = RefLM(m)
  # conditional distributions are (near) normalised over the vocabulary
  for prev in ((), (sents[0][0],), tuple(sents[1][:2])):
    tot = sum(10 ** (lm.lm_score(prev, w) / LN10) for w in m.vocab if w != "<s>")
    assert 0.9 < tot < 1.1, (prev, tot)
