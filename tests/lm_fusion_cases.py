"""Shared by tests/test_lm_fusion_cpu.py and tests/test_gpu_lm_fusion.py: the labels, the ARPA models, fused_ref (a
float64 restatement of the word-language-model fusion of lipreading_amd/csrc/lr_attn_beam.hip), an
independent scorer of a finished hypothesis's language-model terms, the readable trap and the GPU case table.

alpha and beta of every case are dyadic (exact in float32): the C entry takes them as float, so any other value would
differ from the float64 restatement by 2^-24 of every term (6e-5 * alpha on an OOV term), which is an error of the
test's inputs, not of the search."""
import functools
import math
import os

import numpy as np
import torch

from oracle import torch_oracle as O
from tests.test_attn_beam_cpu import BOS, EOS, PAD, UNK, _cat, _pick, _states, small_case
from tests.test_beam_lm_cpu import LN10, SPECIAL, Dict, RefLM, pseudo_corpus, write_arpa
from tests.test_joint_beam_cpu import NEG, empty_prefix, extend, joint_score, random_frames

SPECIALS = ["<PAD>", "<BOS>", "<EOS>", "<UNK>"]           # ids PAD, BOS, EOS, UNK = 0 .. 3
LABELS = ["_"] + SPECIALS + [" "] + list("abcdefghijklmnopqrstuvwxyz") + ["'"]   # C = 33 CTC classes, V = 32 tokens
# further single characters for the case with 64 < V <= 255: V = 80, tokens 64 .. 79 are WIDE_TAIL
LABELS_WIDE = LABELS + list("ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789#$%&()*+-=?@")
WIDE_TAIL = "".join(LABELS_WIDE[65:])
OOV_WORD = "\0oov"


def char2idx(labels):
  """The decoder vocabulary whose decoder.ctc_labels() is `labels`."""
  return {l: i for i, l in enumerate(labels[1:])}


# ---- models ----------------------------------------------------------------------------------------------------------
_DIR = [None]


def set_dir(path):
  """Where the ARPA files are written (a test's tmp_path); the first call wins, so that cached models keep their
  files."""
  if _DIR[0] is None:
    _DIR[0] = str(path)


@functools.lru_cache(maxsize=None)
def arpa(kind, order):
  """Path of a seeded pseudo-word model: 'az' over a-z, 'wide' over a-h and the sixteen characters that sit at
  tokens 64 .. 79 of LABELS_WIDE."""
  assert _DIR[0] is not None, "call set_dir(tmp_path) first"
  alphabet = "abcdefghijklmnopqrstuvwxyz" if kind == "az" else "abcdefgh" + WIDE_TAIL
  _, sents = pseudo_corpus(17 + order, n_words=400, n_sent=600, alphabet=alphabet)
  return write_arpa(os.path.join(_DIR[0], "%s%d.arpa" % (kind, order)), sents, order)


@functools.lru_cache(maxsize=None)
def ref_model(path, labels):
  """(RefLM, Dict, M) of an ARPA file for a label tuple; M = the largest |natural-log value| of the model."""
  from lipreading_amd.lm import read_arpa
  m = read_arpa(path)
  lm = RefLM(m)
  big = LN10 * max(float(np.abs(m.log10_prob).max()), float(np.abs(m.log10_backoff).max()))
  return lm, Dict(lm, list(labels)), big


# ---- the restatement -------------------------------------------------------------------------------------------------
def fused_ref(dec, enc, enc_lens, prev, y, K, Lmax, lam, P, lm, dic, alpha, beta, bos=BOS, eos=EOS, pad=PAD):
  """The fused rule in float64: joint_ref of tests/test_joint_beam_cpu.py plus, per hypothesis, the language-model sum
  l, the trie node, the completed words and the cached term of the current word.  y (B, T, V+1) CTC log-probs (may be
  None at lam = 0).  Returns, per utterance, (beam, margin): beam = [(tokens, s, a, c, l)] best first; margin as in
  joint_ref, on s."""
  dec = dec.double().eval()
  enc = enc.double()
  rnn_type = dec.rnn_type
  prev = tuple(p.double() for p in prev) if isinstance(prev, tuple) else prev.double()
  V = dec.vocab_size
  if P is None:
    P = min(V - 2, -(-3 * K // 2))
  ctc = lam > 0
  if ctc:
    y = np.asarray(y, dtype=np.float64)
  roles = dic.roles

  def term(node, ctx):
    return alpha * lm.lm_score(list(ctx), dic.word[node]) + beta if node else 0.0

  out = []
  with torch.no_grad():
    for b, st0 in enumerate(_states(prev, rnn_type)):
      Tb = int(enc_lens[b])
      gn0 = gb0 = yb = None
      if ctc:
        yb = y[b]
        gn0, gb0 = empty_prefix(yb, Tb)
      beam = [dict(h=[], st=st0, a=0.0, c=0.0, l=0.0, s=0.0, gn=gn0, gb=gb0, node=0, ctx=(), term=0.0)]
      margin = math.inf
      for _ in range(Lmax + 1):
        fin = [len(e["h"]) == Lmax + 1 or (e["h"] and e["h"][-1] == eos) for e in beam]
        if all(fin):
          break
        live = [i for i, f in enumerate(fin) if not f]
        inp = torch.tensor([beam[i]["h"][-1] if beam[i]["h"] else bos for i in live])
        n = len(live)
        lp, new_state = dec(inp, _cat([beam[i]["st"] for i in live], rnn_type), enc_lens[b:b + 1].expand(n),
                            enc[b:b + 1].expand(n, -1, -1))
        lp = lp.numpy()
        lst = []
        for i, e in enumerate(beam):
          if fin[i]:
            lst.append(e)
            continue
          j = live.index(i)
          node = e["node"]
          allowed = [v for v in range(V) if v not in (pad, bos) and
                     not (v != eos and roles[v + 1] == 1 and dic.child[node, v + 1] < 0)]
          order = sorted(allowed, key=lambda v: (-lp[j, v], v))
          last = e["h"][-1] + 1 if e["h"] else None
          for v in order[:P]:
            a = e["a"] + float(lp[j, v])
            c, gn, gb = 0.0, None, None
            if ctc:
              gn, gb, psi, full = extend(e["gn"], e["gb"], last, v + 1, yb, Tb)
              c = full if v == eos else psi
              if c == NEG:
                continue   # a structural zero
            role = roles[v + 1]
            l = e["l"] + (e["term"] if v == eos or role == 2 else 0.0)
            s = (joint_score(a, c, lam) if ctc else a) + l
            if v != eos and role == 1:
              nd = int(dic.child[node, v + 1])
              nxt = dict(node=nd, ctx=e["ctx"], term=term(nd, e["ctx"]))
            elif v != eos and role == 2 and node:
              nxt = dict(node=0, ctx=e["ctx"] + (dic.word[node] or OOV_WORD,), term=0.0)
            else:
              nxt = dict(node=0, ctx=e["ctx"], term=0.0)
            lst.append(dict(h=e["h"] + [v], st=_pick(new_state, j, rnn_type), a=a, c=c, l=l, s=s, gn=gn, gb=gb, **nxt))
        lst = sorted(lst, key=lambda x: -x["s"])   # stable
        if len(lst) > K:
          margin = min(margin, lst[K - 1]["s"] - lst[K]["s"])
        beam = lst[:K]
        if not beam:
          break
      for x, z in zip(beam, beam[1:]):
        margin = min(margin, x["s"] - z["s"])
      out.append(([(e["h"], e["s"], e["a"], e["c"], e["l"]) for e in beam], margin))
  return out


def lm_terms(tokens, labels, lm, alpha, beta, eos=EOS):
  """Independent of fused_ref: the language-model sum of a finished hypothesis read off its STRING, or None when the
  dictionary forbids it.  Returns (l, number of scored in-vocabulary words).  The string is split at spaces; inside a
  piece a transparent token (UNK) splits it again and only the run after the last one is the piece's word; every run
  must be a prefix of a vocabulary word; the last piece is scored only when the hypothesis ends with EOS."""
  words = sorted(w for w in lm.vocab if w not in SPECIAL and all(ch in labels and len(ch) == 1 for ch in w))
  prefixes = {w[:j] for w in words for j in range(len(w) + 1)}
  ended = bool(tokens) and tokens[-1] == eos
  body = tokens[:-1] if ended else tokens
  text = "".join(labels[v + 1] if len(labels[v + 1]) == 1 else "\0" for v in body)
  pieces = text.split(" ")
  l, done, hits = 0.0, [], 0
  for k, piece in enumerate(pieces):
    runs = piece.split("\0")
    if any(r not in prefixes for r in runs):
      return None
    word = runs[-1]
    if word and (k + 1 < len(pieces) or ended):
      known = word in words
      l += alpha * lm.lm_score(done, word if known else OOV_WORD) + beta
      hits += known and all(w != OOV_WORD for w in done[-(lm.order - 1):] if lm.order > 1)
      done.append(word if known else OOV_WORD)
  return l, hits


# ---- the readable trap -----------------------------------------------------------------------------------------------
TRAP_LABELS = ["_"] + SPECIALS + [" ", "a", "b"]    # V = 7: ' ' = 4, 'a' = 5, 'b' = 6
TRAP_ARPA = """\\data\\
ngram 1=4
ngram 2=1

\\1-grams:
-99\t<s>\t-0.3
-1.0\t</s>
-1.0\t<unk>
-0.3\tab\t-0.2

\\2-grams:
-0.1\t<s> ab

\\end\\
"""


def lm_trap():
  """A decoder that alone prefers the non-word 'b'; the only word of the model is 'ab'.  RNN, no attention, Hd = 4,
  char_dim = 7: the state is a code of the input token only (one-hot embedding, W_hh = 0; as greedy_trap), and
  output_proj reads per code
    after BOS: a .55  b .40  EOS .02  UNK .02  ' ' .01;     after a: a .45  b .30  EOS .20  UNK .03  ' ' .02;
    after b or anything else: EOS .90  a .03  b .03  UNK .02  ' ' .02.
  Alone (K = 2, Lmax = 3) the best transcript is b EOS (.36, against a b EOS at .15).  With the model 'b' is no
  vocabulary prefix at the root and 'a' must go on to 'ab': the best is a b EOS."""
  c2i = char2idx(TRAP_LABELS)
  dec = O.OracleCharDecodingStep(4, "RNN", 1, 7, 7, c2i, attention_type="none")
  a, b, sp = c2i["a"], c2i["b"], c2i[" "]
  code = {BOS: 0, a: 1, b: 2, UNK: 3, sp: 3, EOS: 3}
  rows = {0: {a: .55, b: .40, EOS: .02, UNK: .02, sp: .01}, 1: {a: .45, b: .30, EOS: .20, UNK: .03, sp: .02},
          2: {EOS: .90, a: .03, b: .03, UNK: .02, sp: .02}, 3: {EOS: .90, a: .03, b: .03, UNK: .02, sp: .02}}
  with torch.no_grad():
    for p in dec.parameters():
      p.zero_()
    dec.embedding.weight.copy_(torch.eye(7))
    dec.embedding.weight[PAD].zero_()
    for tok, j in code.items():
      dec.rnn.weight_ih_l0[j, tok] = 4.0
    for j, row in rows.items():
      for tok, p in row.items():
        dec.output_proj.weight[tok, j] = math.log(p)
  B, T = 2, 3
  return dec, torch.zeros(B, T, 4), torch.tensor([T, 2]), torch.zeros(1, B, 4)


TRAP_ALONE = [6, EOS]        # 'b'
TRAP_FUSED = [5, 6, EOS]     # 'ab'


def write_trap_arpa(tmp):
  path = os.path.join(str(tmp), "trap.arpa")
  with open(path, "w") as f:
    f.write(TRAP_ARPA)
  return path


# ---- the GPU cases ---------------------------------------------------------------------------------------------------
HD, T, B, LMAX = 64, 20, 12, 20
# (rnn, attention, lambda, ctc_log_probs passed to the device)
CONFIGS = [("GRU", "dot", 0.0, False), ("LSTM", "none", 0.3, True), ("LSTM", "1_layer_nn", 1.0, True),
           ("GRU", "concat", 0.3, True), ("RNN", "general", 0.0, True)]
WEIGHTS = [(0.5, 0.25), (1.0, -0.5), (0.25, 1.0)]   # (alpha, beta), dyadic


def _cases():
  out = []
  for i, (rnn, attn, lam, with_y) in enumerate(CONFIGS):
    for j, K in enumerate((1, 5, 10)):
      alpha, beta = WEIGHTS[(i + j) % 3]
      # the pre-beam ranks by the decoder alone, and the joint cases' decoder is nearly flat: a narrow beam takes a
      # wide pre-beam, or the frames' letters and the EOS are rarely among its candidates; the rest use the default
      P = {1: 30, 5: 20, 10: None}[K] if lam > 0 else None
      out.append(dict(id="%s-%s-%g-K%d" % (rnn, attn, lam, K), rnn=rnn, attn=attn, lam=lam, with_y=with_y, K=K,
                      order=2 + (i + j) % 2, kind="az", labels=tuple(LABELS), seed=300 + 3 * i + j, P=P,
                      alpha=alpha, beta=beta))
  # 64 < V <= 255: a lane of the scan owns two tokens, and the vocabulary uses characters of the second one
  out.append(dict(id="wide-V80", rnn="GRU", attn="dot", lam=0.3, with_y=True, K=5, order=3, kind="wide",
                  labels=tuple(LABELS_WIDE), seed=330, P=20, alpha=0.5, beta=0.25))
  return out


CASES = _cases()
CASE_BY_ID = {c["id"]: c for c in CASES}


def homophene_frames(labels, words, lens, Tmax, seed):
  """CTC log-probs (B, Tmax, C), float32 values in float64, that spell a sentence of vocabulary words per utterance
  as a lip reader sees it: every letter's frame gives .40 to the letter and .50 to a fixed look-alike (the next
  letter of the sentence's alphabet), so the frames alone prefer the wrong letter everywhere and only the words tell
  them apart.  Label i sits at frame 2 i (a blank frame between, so repeats are spelled); ' ' and the final EOS get
  .90, blank frames .90 on the blank; the rest of each frame is spread unevenly (seeded) over the other classes."""
  rng = np.random.default_rng(seed)
  C = len(labels)
  letters = sorted({ch for w in words for ch in w})
  twin = {ch: letters[(i + 1) % len(letters)] for i, ch in enumerate(letters)}
  y = np.empty((len(lens), Tmax, C))
  for b, Tb in enumerate(int(t) for t in lens):
    room = Tb // 2 - 1            # labels besides the EOS
    text = ""
    for _ in range(50):
      w = words[int(rng.integers(len(words)))]
      if len(text) + len(w) + (1 if text else 0) <= room:
        text += (" " if text else "") + w
    frame = np.full((Tmax, C), 0.0)
    for t in range(Tmax):
      i, odd = divmod(t, 2)
      if odd or i > len(text) or t >= Tb:
        peaks = {0: .90}
      elif i == len(text):
        peaks = {labels.index("<EOS>"): .90}
      elif text[i] == " ":
        peaks = {labels.index(" "): .90}
      else:
        peaks = {labels.index(text[i]): .40, labels.index(twin[text[i]]): .50}
      rest = np.exp(rng.standard_normal(C))      # uneven, or every unlikely class would tie exactly
      for k in peaks:
        rest[k] = 0.0
      frame[t] = (1.0 - sum(peaks.values())) * rest / rest.sum()
      for k, p in peaks.items():
        frame[t, k] = p
    y[b] = np.log(frame)
  return y.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs(case_id):
  """(oracle decoder, enc, lens, prev, y) of a case; y is always made (the plain reference needs it)."""
  c = CASE_BY_ID[case_id]
  labels = list(c["labels"])
  V = len(labels) - 1
  # With the CTC term the frames lead and the decoder is nearly flat (scale 1), and it ends sooner (a hypothesis longer
  # than its frames is a structural zero); without it the decoder alone proposes, so it is peaked and runs long.
  joint = c["lam"] > 0
  odec, enc, _, prev = small_case(c["rnn"], c["attn"], V=V, Hd=HD, T=T, B=B, seed=c["seed"],
                                  scale=1.0 if joint else 8.0, eos_bias=0.0 if joint else -1.0)
  with torch.no_grad():
    # text-like output: UNK is rare (a decoder that is free with UNK drops every run unscored and never meets the
    # model) and, where the frames do not supply them, spaces are common: hypotheses spell words the model scores
    odec.output_proj.bias[UNK] -= 12.0 if joint else 6.0
    if not joint:
      odec.output_proj.bias[labels.index(" ") - 1] += 2.0
  g = torch.Generator().manual_seed(c["seed"])
  lens = torch.randint(T // 3, T + 1, (B,), generator=g)
  lens[0] = T
  lm, _, _ = ref_model(arpa(c["kind"], c["order"]), c["labels"])
  words = sorted(w for w in lm.vocab if w not in SPECIAL and all(ch in labels for ch in w))
  return odec, enc, lens, prev, homophene_frames(labels, words, lens, T, c["seed"])


@functools.lru_cache(maxsize=None)
def reference(case_id):
  """fused_ref of a case, computed once per process and shared."""
  c = CASE_BY_ID[case_id]
  odec, enc, lens, prev, y = inputs(case_id)
  lm, dic, _ = ref_model(arpa(c["kind"], c["order"]), c["labels"])
  return fused_ref(odec, enc, lens, prev, y if c["lam"] > 0 else None, c["K"], LMAX, c["lam"], c["P"], lm, dic,
                   c["alpha"], c["beta"])


def hip_decoder(odec, labels, dev):
  """A CharDecodingStep holding the oracle's weights, over the vocabulary of `labels`."""
  from lipreading_amd.attention_decoder import CharDecodingStep
  from lipreading_amd.encoder import VideoEncoder
  enc = VideoEncoder(204, odec.hidden_size, rnn_type=odec.rnn_type, num_layers=odec.num_layers, bidirectional=False)
  ah = odec.attn_proj_layer1.out_features if odec.attention_type == "concat" else -1
  dec = CharDecodingStep(enc, char_dim=odec.char_dim, vocab_size=odec.vocab_size, char2idx=char2idx(list(labels)),
                         attention_type=odec.attention_type, attn_hidden_size=ah)
  r = dec.load_state_dict({k: v.float() for k, v in odec.state_dict().items()})
  assert not (r.missing_keys or r.unexpected_keys)
  return dec.to(dev).eval()
