// lr_ctc_beam.hip — CTC prefix beam search, with or without an ARPA n-gram word language model, for gfx950.
//
// Replaces src/models/lipreader/decoder.py:90-143 (BeamCTCDecoder), which hands the search to the external
// `ctcdecode` C++ library (CTCBeamDecoder with lm_path=None) after a probs.cpu() copy.  ctcdecode is not part of this
// build, so the specification is this build's own:
//
//   Input    probs element (b,t,c) at probs[b*stride_b + t*stride_t + c], fp32.  log_input = 0: the values are
//            probabilities (the reference's contract); 1: log-probabilities (what VideoEncoder returns).
//            sizes[B] int32 or NULL (= T), clamped to [0, T].  Frames t >= sizes[b] are never read.
//   Pruning  per frame (ctcdecode's cutoff_top_n / cutoff_prob): sort the classes by probability, descending, ties to
//            the lower index (as torch.max and lr_ctc_greedy_decode); keep the first cutoff_top_n; if cutoff_prob < 1,
//            keep only the shortest prefix of that list whose cumulative probability (float64) is >= cutoff_prob,
//            with at least one class.
//   State    per hypothesis (log p_blank, log p_nonblank); score = logaddexp of the two.  The empty prefix starts
//            with (0, -inf).  At frame t, for each hypothesis p with last character l and each kept class c:
//              c == blank  p.p_blank'    += score(p) * p(c)
//              c == l      p.p_nonblank' += p_nonblank(p) * p(c)    and   (p+c).p_nonblank' += p_blank(p) * p(c)
//              otherwise   (p+c).p_nonblank' += score(p) * p(c)
//            An extension p+c that equals a hypothesis already in the beam merges into it.  A candidate of
//            probability zero (score -inf) is not a hypothesis and is never kept.
//   Select   the beam_width best candidates by score; ties go to the lower (parent rank, class), the parent's own
//            continuation ranking before its extensions.  ctcdecode's `min_cutoff` early-out (skip classes whose
//            log p(c) falls below the worst kept score) is NOT applied: a stated deviation from ctcdecode.
//   Offsets  a hypothesis that already existed keeps its offsets; one first created at frame t takes its parent's
//            offsets plus t.  With beam_width = 1 and cutoff_top_n = 1 the ids and offsets are exactly
//            lr_ctc_greedy_decode's.
//   Output   out_ids[B][W][T], out_offsets[B][W][T] int32, padded with -1; out_lens[B][W] (0 for beam slots that
//            hold no hypothesis); out_scores[B][W] = -log P(prefix) fp32, ascending (+inf in empty slots).  This is
//            ctcdecode's score convention as the reference reads it; no ctcdecode is available to compare against,
//            so the convention is checked only against exhaustive enumeration (tests/test_gpu_beam.py).
//
// Limits: beam_width <= 128, cutoff_top_n <= 64 (values above C act as C), C <= 256, 1 + T*beam_width < 2^31;
// anything else is LR_ERR_UNSUPPORTED.
//
// Layout: two launches.
//   1. beam_prune_kernel — one wave per (b,t) frame across the whole chip: cutoff_top_n rounds of a 64-lane argmax
//      over (value, index) keys pick the kept classes in order, a float64 wave scan applies cutoff_prob, and the
//      compact (class, log p) list goes to the workspace.  The sequential loop never touches the C axis.
//   2. beam_loop_kernel — one workgroup per utterance, one pass per frame.  Hypotheses are trie node ids; the node
//      table (parent, class, frame) lives in the workspace, at most beam_width new nodes per frame (node 1+t*W+r is
//      the one created at frame t for rank r).  The beam's (node, parent node, class, depth, masses) stay in LDS, so
//      the table is only written during the loop and read at the end.  An extension p+c equals beam entry q iff
//      prefix(parent(q)) == prefix(p) && class(q) == c.  Node ids alone do not decide that: a prefix that leaves the
//      beam and comes back is a new node while its children that stayed keep the old one as parent.  So every beam
//      entry carries a 64-bit hash of its prefix, each q looks its parent's prefix hash up in an LDS table of the
//      beam's hashes, and a hit is confirmed exactly — same parent node, or both node chains walked back to a common
//      node with equal classes on the way (the rare case).  q then takes over that extension's mass.  The top-W of the W*(n+1) candidates is a radix select on 48-bit
//      (score, tie-break) keys — 8-bit digits, LDS histograms, stopping at the first digit that closes the count —
//      followed by a rank count among the W survivors.  At the end each beam walks its node chain backwards.
//
// With a word language model (lr_ctc_beam_lm_decode; the reference passes ctcdecode a KenLM model through lm_path,
// alpha and beta).  Everything above holds; the following is added.
//   Classes  class_roles[C] names each class's role.  The label that is exactly ' ' is the space class; it separates
//            words.  Every other one-character label except the blank is a word character.  All other classes
//            (the blank, multi-character labels such as <EOS>) are transparent: they stay in the output but never
//            extend or complete a word.  A prefix's words are its maximal runs of word characters.  A word is
//            completed by the space that follows it; a transparent class drops the run it follows, which is then
//            neither scored nor part of any later context, and the next word character starts a new word.
//   LM term  lm(w | ctx) = ln(10) * log10 P(w | ctx) by standard ARPA backoff.  ctx is the last order-1 completed
//            words before w, padded on the left with <s>.  If (ctx, w) is listed, its probability; otherwise
//            backoff(ctx) + P(w | ctx[1:]), an absent backoff counting as 0.  If w or any word of ctx is not an ARPA
//            unigram the term is OOV = -1000 (no ln 10 factor; ctcdecode's Scorer::get_log_cond_prob).  </s> is
//            never scored.
//   Apply    each application adds alpha * lm + beta to the extension's log mass: an extension p+space (from
//            score(p), and from p_blank(p) when p already ends in a space) applies it to the word p ends in, if
//            that word is non-empty.  A leading space, a repeated space or a space right after a transparent class
//            adds nothing.
//   Dict     a word-character extension exists only if the current word stays a prefix of a vocabulary word (a
//            trie of the vocabulary spelled in class ids, as ctcdecode's dictionary for a word LM); otherwise the
//            candidate is not a hypothesis.  The vocabulary is the ARPA unigrams except <s>, </s> and <unk>; words
//            with a character that has no class cannot be reached and are left out.  There is no switch to turn it
//            off.
//   End      after the last frame each hypothesis whose last word is non-empty gets alpha * lm + beta for that word
//            (a vocabulary prefix that is not a word is OOV); then the beam is re-sorted by the final score, ties
//            keeping the earlier rank.  out_scores = -(log mass + that term), ascending.
//   Merging  the LM state (trie node, context word ids) is a function of the prefix, so merging by prefix holds.
//   Deviations from ctcdecode: no character-based LM mode; no min_cutoff; empty words are not scored; ARPA only
//            (the host reads the text, lipreading_amd/lm.py; KenLM's binary formats are not read).
//   Limits   order <= 6 (KenLM's default maximum) and vocabulary < 2^24 (the packer's LR_ERR_UNSUPPORTED);
//            non-finite alpha or beta is LR_ERR_INVALID_ARG.
//   Layout   one packed read-only blob per model (lm_pack, below), uploaded once.  Lookups are open-addressing
//            hash tables on exact 64-bit keys: (entry id of the n-gram's first k-1 words, last word id) and
//            (trie node, class); a word or an n-gram is never identified by a hash of its string.  The loop keeps
//            each hypothesis's trie node, its node's word id, its last order-1 completed word ids and the cached
//            term alpha * lm + beta of its current word in LDS: phase 2 adds the cached term to the space
//            extension and probes the trie for each word-character extension; phase 5 probes the trie again for
//            the survivors and scores their new current word; the end term is the cached one.
//
// With hotwords (lr_ctc_beam_bias_decode, lr_ctc_beam_lm_bias_decode; contextual biasing as pyctcdecode's, the
// specification is this build's own).  Everything above holds; the following is added.
//   Phrases  q_k: class ids, length m_k >= 1, finite weight w_k > 0.  anchor = the class of ' ', or -1.  A start
//            position i of a prefix y is admissible if anchor < 0, or i == 0, or y[i-1] == anchor: with an anchor a
//            phrase matches only at the start of a word.  The blank never appears in y; every other class may appear
//            in a phrase and is compared by index.
//   Scores   occ_k(y) = the number of admissible i with y[i:i+m_k] == q_k (overlaps count).  partial(y) = the largest
//            w_k * j / m_k over k and 1 <= j < m_k such that y ends with q_k[:j] and that suffix starts at an
//            admissible position (0 if there is none).  bonus_end(y) = sum_k w_k * occ_k(y);
//            bonus_run(y) = bonus_end(y) + partial(y).
//   Search   the masses (p_blank, p_nonblank) evolve exactly as without hotwords (with a language model they carry
//            its terms).  At every frame a candidate's selection key is score + bonus_run(its prefix), the tie-break
//            unchanged: a parent's own continuation keeps the parent's bonus, an extension takes that of p+c.  The
//            bonus is a function of the prefix, so merging by prefix holds.
//   End      after the last frame the partial credit is dropped: final score = log mass (+ the LM's end term)
//            + bonus_end; the beam is re-sorted by it, ties keeping the earlier rank.  out_scores = -(final score),
//            ascending.  Offsets, ids and lens as above.
//   LM       the dictionary is unchanged: a hotword whose words are not ARPA unigrams stays unreachable.
//   Layout   the host (lr_ctc_beam_bias_pack) builds an Aho-Corasick automaton over the phrases (with an anchor: over
//            anchor + q_k, the search starting in the state that follows one anchor; the anchor is not counted in
//            j / m_k) and writes one read-only blob: next[node][C] int32 with the fail links resolved, out[node] =
//            the sum of w_k of every phrase ending at the node (through the fail chain), part[node] = the best
//            partial credit along the fail chain (phrases that end exactly there excluded).  Per hypothesis the loop
//            keeps one node id and one banked fp32 sum (bonus_end) in LDS.  An extension's bonus is
//            (bank + out[nn]) + part[nn] with nn = next[node][c], in fp32 and in that order: one 4-byte load and two
//            more.  The key's bonus is added to sm.score in phase 2; phases 3 and 5 recompute the few masses they
//            need (a merged extension's, a surviving extension's) with phase 2's own expression, so the masses stay
//            bit-identical to the search without hotwords.
//   Limits   at most 4096 automaton nodes, 1024 phrases, C <= 256 (the packer's LR_ERR_UNSUPPORTED); an empty phrase
//            or a weight that is not finite and positive is LR_ERR_INVALID_ARG.
//
// Sessions (lr_ctc_beam_stream_*): the four searches above, fed chunk by chunk.  Everything above holds, frame by
// frame; t is the frame's index in the session, so offsets and the trie's node ids count the session's frames.
//   Advance  consumes frames [0, clamp(sizes[b], 0, chunk_T)) of slot b's chunk from the slot's beam as the last
//            advance left it: the pruning launch over the chunk, then the loop kernel's STREAM instantiation.
//   Read     what the one-shot entry would put out if the stream ended now: the End terms of the variant are the
//            read's (they do not feed back into the loop) and it changes no byte of the state.  stable = the length
//            of the longest common prefix, as id strings, of all live hypotheses: every later hypothesis is a live
//            one or extends one, so those ids are final.
//   Equality fed the same frames in any chunks, a session holds the one-shot entry's bits: the state stored between
//            two launches is exactly what the loop carries from one frame to the next (the beam's arrays in beam
//            order, the live count, the trie), and fp32 values go through memory unchanged.
//   Limits   the search's, with max_frames in T's place.  No trie compaction: a session ends at max_frames.
#include <string.h>

#include <type_traits>
#include <vector>

#include "lr_common.h"
#include "lr_lm_dev.h"

namespace {

constexpr int kBeamMaxW = 128;
constexpr int kBeamMaxN = 64;
constexpr int kBeamMaxC = 256;
constexpr int kMaxCand = kBeamMaxW * (kBeamMaxN + 1);
constexpr int kHash = 512;            // >= 4 * kBeamMaxW: open addressing at load <= 1/4
constexpr int kLoopThreads = 512;
constexpr int kPruneWaves = 4;

__device__ __forceinline__ uint32_t ord_f32(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct BeamWs {
  int32_t* kcls;   // [B][T][n] kept classes, most probable first
  float* klp;      // [B][T][n] their log-probabilities
  int32_t* kcnt;   // [B][T]    how many were kept
  int32_t* npar;   // [B][NN]   trie: parent node
  int32_t* ncls;   // [B][NN]   trie: class
  int32_t* nfrm;   // [B][NN]   trie: frame the node was created at
};

__host__ __device__ inline int64_t beam_nodes(int T, int W) { return 1 + (int64_t)T * W; }

inline size_t beam_ws_bytes(int B, int T, int n, int W) {
  const size_t frames = (size_t)B * T;
  size_t s = lr_align_up(frames * n * 4, 256) * 2 + lr_align_up(frames * 4, 256);
  s += 3 * lr_align_up((size_t)B * beam_nodes(T, W) * 4, 256);
  return s;
}

inline BeamWs beam_ws_carve(void* ws, int B, int T, int n, int W) {
  char* p = static_cast<char*>(ws);
  const size_t frames = (size_t)B * T;
  BeamWs w;
  w.kcls = reinterpret_cast<int32_t*>(p); p += lr_align_up(frames * n * 4, 256);
  w.klp = reinterpret_cast<float*>(p);    p += lr_align_up(frames * n * 4, 256);
  w.kcnt = reinterpret_cast<int32_t*>(p); p += lr_align_up(frames * 4, 256);
  const size_t nodes = lr_align_up((size_t)B * beam_nodes(T, W) * 4, 256);
  w.npar = reinterpret_cast<int32_t*>(p); p += nodes;
  w.ncls = reinterpret_cast<int32_t*>(p); p += nodes;
  w.nfrm = reinterpret_cast<int32_t*>(p);
  return w;
}

// ---------------------------------------------------------------------------------------
// 1. per-frame top-n + cutoff: one wave per frame, lanes along the class axis (C <= 256: 4 per lane)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPruneWaves * LR_WAVE) void beam_prune_kernel(
    const float* __restrict__ probs, int64_t stride_b, int64_t stride_t, const int32_t* __restrict__ sizes,
    int log_input, float cutoff_prob, int32_t* __restrict__ kcls, float* __restrict__ klp,
    int32_t* __restrict__ kcnt, int B, int T, int C, int n) {
  const int lane = threadIdx.x & (LR_WAVE - 1);
  const int64_t f = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
  if (f >= (int64_t)B * T) return;
  const int b = (int)(f / T), t = (int)(f - (int64_t)b * T);
  int len = sizes ? sizes[b] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  if (t >= len) return;
  const float* pr = probs + (int64_t)b * stride_b + (int64_t)t * stride_t;
  // key = (order-preserving value bits, ~class): the largest key is the most probable class, lowest index on ties.
  // 0 marks "absent or taken"; a real key is never 0 (its low word ~c is > 0 for c < 2^32-1).
  uint64_t key[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = lane + r * LR_WAVE;
    key[r] = c < C ? ((uint64_t)ord_f32(pr[c]) << 32) | (uint64_t)(0xffffffffu - (uint32_t)c) : 0ull;
  }
  const int nn = n < C ? n : C;
  uint64_t mine = 0;   // lane k ends up with the k-th kept key
  for (int k = 0; k < nn; ++k) {
    uint64_t w = key[0] > key[1] ? key[0] : key[1];
    const uint64_t w2 = key[2] > key[3] ? key[2] : key[3];
    w = w > w2 ? w : w2;
#pragma unroll
    for (int off = LR_WAVE / 2; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor(w, off);
      w = o > w ? o : w;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (key[r] == w) key[r] = 0ull;
    if (lane == k) mine = w;
  }
  const bool have = lane < nn;
  const int c = (int)(0xffffffffu - (uint32_t)mine);
  const float v = unord_f32((uint32_t)(mine >> 32));
  int cnt = nn;
  if (cutoff_prob < 1.f) {
    double cum = have ? (log_input ? exp((double)v) : (double)v) : 0.0;
#pragma unroll
    for (int off = 1; off < LR_WAVE; off <<= 1) {
      const double o = __shfl_up(cum, off);
      if (lane >= off) cum += o;
    }
    const uint64_t hit = __ballot(have && cum >= (double)cutoff_prob);
    if (hit) cnt = __ffsll((unsigned long long)hit);   // first hit's lane + 1
  }
  if (lane < cnt) {
    kcls[f * n + lane] = c;
    klp[f * n + lane] = log_input ? v : logf(v);
  }
  if (lane == 0) kcnt[f] = cnt;
}

struct LmArgs {
  const uint8_t* blob;     // nullptr: no language model
  const int32_t* roles;    // [C] kRole*
  float alpha, beta;
};

// the loop kernel's last argument: the plain and LM instantiations take LmArgs as it is, the bias ones the blob too
struct BiasLmArgs : LmArgs {
  const uint8_t* bias;   // the packed hotword automaton
};
template <bool BIAS>
using LoopArgs = std::conditional_t<BIAS, BiasLmArgs, LmArgs>;

// the packed hotword automaton (lr_ctc_beam_bias_pack): header, next[nodes][stride] int32, out[nodes], part[nodes] fp32
constexpr uint32_t kBiasMagic = 0x5342524cu;   // "LRBS"
constexpr int kBiasVersion = 1;
constexpr int kBiasMaxNodes = 4096;
constexpr int kBiasMaxPhrases = 1024;
struct BiasHeader {
  uint32_t magic;
  int32_t version, nodes, stride, start, phrases, anchor, pad_;
  int64_t next_off, out_off, part_off, bytes;
};
static_assert(sizeof(BiasHeader) == 64, "BiasHeader is part of the blob's layout");

struct BiasView {
  const int32_t* next;
  const float* out;
  const float* part;
  int stride, start;
};
__device__ __forceinline__ BiasView bias_view(const uint8_t* blob) {
  const BiasHeader* h = reinterpret_cast<const BiasHeader*>(blob);
  return BiasView{reinterpret_cast<const int32_t*>(blob + h->next_off), reinterpret_cast<const float*>(blob + h->out_off),
                  reinterpret_cast<const float*>(blob + h->part_off), h->stride, h->start};
}
// a class the blob was not packed for is in no phrase and is not the anchor: it leads to the root
__device__ __forceinline__ int bias_next(const BiasView& v, int node, int c) {
  return c < v.stride ? v.next[node * v.stride + c] : 0;
}

// ---------------------------------------------------------------------------------------
// 2. the frame loop: one workgroup per utterance
// ---------------------------------------------------------------------------------------
// LM state of the beam (the LM instantiation only): trie node, the word id that node spells, the cached term
// alpha * lm + beta of that word (0 at the root) and the last m completed word ids
template <bool LM>
struct BeamLmSmem {
  int tnode[2][kBeamMaxW], tword[2][kBeamMaxW];
  float tterm[2][kBeamMaxW];
  int ctx[2][kBeamMaxW][kLmMaxCtx];
  int role[kBeamMaxC];
  float fin[kBeamMaxW];
  int perm[kBeamMaxW];
};
template <>
struct BeamLmSmem<false> {};

// hotword state of the beam (the bias instantiations only): automaton node, the banked bonus_end, this frame's
// bonus_run of the own continuation; without a language model also the end's re-sort (the LM block has its own)
template <bool BIAS, bool LM>
struct BeamBiasSmem {};
template <>
struct BeamBiasSmem<true, true> {
  int bnode[2][kBeamMaxW];
  float bbank[2][kBeamMaxW];
  float sbon[kBeamMaxW];
};
template <>
struct BeamBiasSmem<true, false> {
  int bnode[2][kBeamMaxW];
  float bbank[2][kBeamMaxW];
  float sbon[kBeamMaxW];
  float fin[kBeamMaxW];
  int perm[kBeamMaxW];
};

struct BeamSmem {
  float score[kMaxCand];          // candidate s = i*(n+1) + j: j = 0 parent i's own continuation, j = 1+k extension by
                                  // kept class k; -inf = not a hypothesis
  int hist[2][256];               // radix-select histograms (alternating, so clearing one never races the other)
  int hslot[kHash];               // prefix hash -> beam slot (open addressing; the key is hpre[cur][slot])
  uint64_t hpre[2][kBeamMaxW], hpar[2][kBeamMaxW];   // hash of the prefix and of its parent prefix
  int node[2][kBeamMaxW], par[2][kBeamMaxW], cls[2][kBeamMaxW], depth[2][kBeamMaxW];
  float pb[2][kBeamMaxW], pnb[2][kBeamMaxW];
  float spb[kBeamMaxW], spnb[kBeamMaxW];   // this frame's own-continuation masses
  int kc[kBeamMaxN];
  float kl[kBeamMaxN];
  int c2k[kBeamMaxC];             // class -> kept rank this frame, -1 if pruned
  uint64_t selkey[kBeamMaxW];
  int selslot[kBeamMaxW];
  int ctl[8];                     // [0] digit [1] need [2] count in digit [3] total [4] selected
};

// prefix hash of p+c from that of p (splitmix64's finaliser over the parent hash and the class)
__device__ __forceinline__ uint64_t prefix_hash(uint64_t h, int c) {
  uint64_t x = h ^ ((uint64_t)(c + 1) * 0x9e3779b97f4a7c15ull);
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint32_t hash_slot(uint64_t key) { return (uint32_t)(key >> (64 - 9)); }   // kHash = 2^9

// node-table reads that bypass the CU's L1: the entries were written by other threads of this workgroup in earlier
// frames (ordered by the frame's barriers)
__device__ __forceinline__ int node_ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// nodes a and b of equal depth spell the same prefix
__device__ bool same_prefix(int a, int b, const int32_t* gpar, const int32_t* gcls) {
  while (a != b) {
    if (node_ld(gcls + a) != node_ld(gcls + b)) return false;
    a = node_ld(gpar + a);
    b = node_ld(gpar + b);
  }
  return true;
}

// 48-bit selection key: score bits above the tie-break (parent rank, then own continuation before extensions in
// class order); larger is better.  tb <= 127*257 + 256 < 2^16.
__device__ __forceinline__ uint64_t cand_key(float sc, int s, int n1, const int* kc) {
  const int i = s / n1, j = s - i * n1;
  const int tb = i * (kBeamMaxC + 1) + (j == 0 ? 0 : 1 + kc[j - 1]);
  return ((uint64_t)ord_f32(sc) << 16) | (uint64_t)(0xffffu - (uint32_t)tb);
}

// the mass of parent i's extension by kept class k, as phase 2 computes it: the bias instantiations keep the key in
// sm.score and recompute the masses they need
template <bool LM>
__device__ __forceinline__ float ext_mass(const BeamSmem& sm, const BeamLmSmem<LM>& lsm, int cur, int i, int k) {
  const int c = sm.kc[k];
  const float pbi = sm.pb[cur][i], pnbi = sm.pnb[cur][i];
  float sc = (c == sm.cls[cur][i] ? pbi : lr_lse2(pbi, pnbi)) + sm.kl[k];
  if constexpr (LM) {
    if (lsm.role[c] == kRoleSpace) sc += lsm.tterm[cur][i];
  }
  return sc;
}

// A session (lr_ctc_beam_stream_*): one caller-owned device buffer that holds, for B independent slots, what the loop
// keeps in LDS between two frames, so that the search can stop after any frame and go on in a later launch.
//   header   [B] StreamHdr: the configuration of the last reset, the frames consumed, the live hypotheses, status bits
//   beam     [B][W] per array, in beam order: node, par, cls, depth, pb, pnb, hpre, hpar; with a language model tnode,
//            tword, tterm, ctx [B][W][kLmMaxCtx]; with hotwords bnode, bbank
//   trie     npar, ncls, nfrm [B][1 + max_frames * W]: node 1 + t*W + r is created at the session's frame t
// Every section starts at a multiple of 256 bytes.  The header's place does not depend on the configuration, so a call
// whose arguments disagree with it finds it all the same.
constexpr int32_t kStreamMagic = 0x5342524d;   // "MRBS"
constexpr int kStreamThreads = 128;            // reset and read: one thread per beam entry
struct StreamHdr {
  int32_t magic, B, W, max_frames, variant, frames, nb, status;
};
static_assert(sizeof(StreamHdr) == 32, "StreamHdr is part of the state's layout");
struct StreamState {
  StreamHdr* hdr;
  int32_t *node, *par, *cls, *depth;
  float *pb, *pnb;
  uint64_t *hpre, *hpar;
  int32_t *tnode, *tword;
  float* tterm;
  int32_t* ctx;
  int32_t* bnode;
  float* bbank;
  int32_t *npar, *ncls, *nfrm;
};
// what the one-shot instantiations take in the session's place
struct NoStream {
  int unused_;
};
// one advance: the state's sections and the max_frames the caller states
struct StreamLaunch : StreamState {
  int max_frames;
};
template <bool STREAM>
using StreamArg = std::conditional_t<STREAM, StreamLaunch, NoStream>;

__host__ __device__ inline int stream_variant(bool lm, bool bias) { return (lm ? 1 : 0) | (bias ? 2 : 0); }

// the state's sections for (B, max_frames, W, variant) over `base`; returns the state's size in bytes
__host__ __device__ inline size_t stream_carve(void* base, int B, int max_frames, int W, int variant, StreamState* s) {
  char* p = static_cast<char*>(base);
  size_t o = 0;
  const size_t slots = (size_t)B * W;
  auto take = [&](size_t bytes) {
    char* at = p ? p + o : nullptr;
    o += (bytes + 255) & ~(size_t)255;
    return at;
  };
  s->hdr = reinterpret_cast<StreamHdr*>(take((size_t)B * sizeof(StreamHdr)));
  s->node = reinterpret_cast<int32_t*>(take(slots * 4));
  s->par = reinterpret_cast<int32_t*>(take(slots * 4));
  s->cls = reinterpret_cast<int32_t*>(take(slots * 4));
  s->depth = reinterpret_cast<int32_t*>(take(slots * 4));
  s->pb = reinterpret_cast<float*>(take(slots * 4));
  s->pnb = reinterpret_cast<float*>(take(slots * 4));
  s->hpre = reinterpret_cast<uint64_t*>(take(slots * 8));
  s->hpar = reinterpret_cast<uint64_t*>(take(slots * 8));
  s->tnode = s->tword = s->ctx = s->bnode = nullptr;
  s->tterm = s->bbank = nullptr;
  if (variant & 1) {
    s->tnode = reinterpret_cast<int32_t*>(take(slots * 4));
    s->tword = reinterpret_cast<int32_t*>(take(slots * 4));
    s->tterm = reinterpret_cast<float*>(take(slots * 4));
    s->ctx = reinterpret_cast<int32_t*>(take(slots * 4 * kLmMaxCtx));
  }
  if (variant & 2) {
    s->bnode = reinterpret_cast<int32_t*>(take(slots * 4));
    s->bbank = reinterpret_cast<float*>(take(slots * 4));
  }
  const size_t nodes = (size_t)B * (size_t)beam_nodes(max_frames, W) * 4;
  s->npar = reinterpret_cast<int32_t*>(take(nodes));
  s->ncls = reinterpret_cast<int32_t*>(take(nodes));
  s->nfrm = reinterpret_cast<int32_t*>(take(nodes));
  return o;
}

// LM = false is the search without a language model; LM = true adds the terms and the dictionary of the header.
// BIAS = true adds the hotwords' bonus to the selection key.  LM + BIAS re-sorts through the LM block's fin / perm, so
// its 2.5 KB of hotword state fit beside the LM's 62 KB under the 64 KB of static LDS.
// STREAM = true is one advance of a session: T is the chunk's length, the beam comes from `ss` into the [0] halves
// and goes back from the [cur] ones, the frames count on from the slot's, and nothing is put out (beam_read_kernel).
template <bool LM, bool BIAS, bool STREAM = false>
__global__ __launch_bounds__(kLoopThreads) void beam_loop_kernel(
    const int32_t* __restrict__ kcls, const float* __restrict__ klp, const int32_t* __restrict__ kcnt,
    const int32_t* __restrict__ sizes, int32_t* __restrict__ npar, int32_t* __restrict__ ncls,
    int32_t* __restrict__ nfrm, int32_t* __restrict__ out_ids, int32_t* __restrict__ out_off,
    int32_t* __restrict__ out_lens, float* __restrict__ out_scores, int T, int W, int n, int blank, int C,
    LoopArgs<BIAS> lma, StreamArg<STREAM> ss) {
  __shared__ BeamSmem sm;
  __shared__ BeamLmSmem<LM> lsm;
  __shared__ BeamBiasSmem<BIAS, LM> bsm;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int nt = blockDim.x;
  const int n1 = n + 1;
  int len = sizes ? sizes[b] : T;
  len = len < 0 ? 0 : (len > T ? T : len);
  int t0 = 0, nb = 1;   // the first frame's index in the utterance; the live hypotheses
  int64_t nbase = (int64_t)b * beam_nodes(T, W);
  if constexpr (STREAM) {
    // T is the chunk's length; the slot's header decides where its frames count from and how many may follow
    const StreamHdr h = ss.hdr[b];
    if (h.magic != kStreamMagic || h.B != (int)gridDim.x || h.W != W || h.max_frames != ss.max_frames ||
        h.variant != stream_variant(LM, BIAS) || h.frames < 0 || h.frames > h.max_frames || h.nb < 0 || h.nb > W) {
      if (tid == 0) ss.hdr[b].status = h.status | LR_BEAM_STREAM_MISMATCH;
      return;
    }
    t0 = h.frames;
    nb = h.nb;
    if (len > h.max_frames - t0) {
      len = h.max_frames - t0;
      if (tid == 0) ss.hdr[b].status = h.status | LR_BEAM_STREAM_OVERFLOW;
    }
    if (len <= 0) return;   // the slot keeps every other bit
    nbase = (int64_t)b * beam_nodes(h.max_frames, W);
  }
  int32_t* gpar = npar + nbase;
  int32_t* gcls = ncls + nbase;
  int32_t* gfrm = nfrm + nbase;

  for (int c = tid; c < kBeamMaxC; c += nt) sm.c2k[c] = -1;
  if (tid == 0) {
    sm.node[0][0] = 0; sm.par[0][0] = -1; sm.cls[0][0] = -1; sm.depth[0][0] = 0;
    sm.pb[0][0] = 0.f; sm.pnb[0][0] = LR_NEG_INF;
    sm.hpre[0][0] = 0; sm.hpar[0][0] = 0;
  }
  LmView L{};
  if constexpr (LM) {
    L = lm_view(lma.blob);
    const int bos = reinterpret_cast<const LmHeader*>(lma.blob)->bos;
    for (int c = tid; c < kBeamMaxC; c += nt) lsm.role[c] = c < C ? lma.roles[c] : kRoleTransparent;
    if (tid == 0) {
      lsm.tnode[0][0] = 0; lsm.tword[0][0] = -1; lsm.tterm[0][0] = 0.f;
      for (int q = 0; q < kLmMaxCtx; ++q) lsm.ctx[0][0][q] = bos;
    }
  }
  BiasView bv{};
  if constexpr (BIAS) {
    bv = bias_view(lma.bias);
    if (tid == 0) { bsm.bnode[0][0] = bv.start; bsm.bbank[0][0] = 0.f; }
  }
  if constexpr (STREAM) {
    if (tid < nb) {
      const int64_t g = (int64_t)b * W + tid;
      sm.node[0][tid] = ss.node[g]; sm.par[0][tid] = ss.par[g]; sm.cls[0][tid] = ss.cls[g];
      sm.depth[0][tid] = ss.depth[g]; sm.pb[0][tid] = ss.pb[g]; sm.pnb[0][tid] = ss.pnb[g];
      sm.hpre[0][tid] = ss.hpre[g]; sm.hpar[0][tid] = ss.hpar[g];
      if constexpr (LM) {
        lsm.tnode[0][tid] = ss.tnode[g]; lsm.tword[0][tid] = ss.tword[g]; lsm.tterm[0][tid] = ss.tterm[g];
        for (int q = 0; q < kLmMaxCtx; ++q) lsm.ctx[0][tid][q] = ss.ctx[g * kLmMaxCtx + q];
      }
      if constexpr (BIAS) { bsm.bnode[0][tid] = ss.bnode[g]; bsm.bbank[0][tid] = ss.bbank[g]; }
    }
  }
  int cur = 0;
  // the kept list of the next frame is loaded one frame ahead
  int pf_cnt = 0, pf_c = 0;
  float pf_l = 0.f;
  if (len > 0) {
    const int64_t f = (int64_t)b * T;
    pf_cnt = kcnt[f];
    if (tid < pf_cnt) { pf_c = kcls[f * n + tid]; pf_l = klp[f * n + tid]; }
  }
  __syncthreads();

  for (int tt = 0; tt < len; ++tt) {
    const int t = t0 + tt;   // the frame's index in the utterance: the trie's node ids and the offsets count in it
    const int cnt = pf_cnt;
    // -- phase 1: this frame's kept classes, fresh hash and histograms
    for (int h = tid; h < kHash; h += nt) sm.hslot[h] = -1;
    if (tid < cnt) { sm.kc[tid] = pf_c; sm.kl[tid] = pf_l; sm.c2k[pf_c] = tid; }
    if (tid < 256) { sm.hist[0][tid] = 0; sm.hist[1][tid] = 0; }
    if (tid == 0) sm.ctl[4] = 0;
    if (tt + 1 < len) {
      const int64_t f = (int64_t)b * T + tt + 1;
      pf_cnt = kcnt[f];
      if (tid < pf_cnt) { pf_c = kcls[f * n + tid]; pf_l = klp[f * n + tid]; }
    }
    __syncthreads();

    // -- phase 2: prefix hash -> slot table; every candidate's mass
    if (tid < nb) {
      uint32_t h = hash_slot(sm.hpre[cur][tid]);
      while (atomicCAS(&sm.hslot[h], -1, tid) != -1) h = (h + 1) & (kHash - 1);
    }
    const int M = nb * n1;
    const int kblank = sm.c2k[blank];
    for (int s = tid; s < M; s += nt) {
      const int i = s / n1, j = s - i * n1;
      const float pbi = sm.pb[cur][i], pnbi = sm.pnb[cur][i];
      const int last = sm.cls[cur][i];
      if (j == 0) {
        const float nb_ = kblank >= 0 ? lr_lse2(pbi, pnbi) + sm.kl[kblank] : LR_NEG_INF;
        const int kl_ = last >= 0 ? sm.c2k[last] : -1;
        const float nnb = kl_ >= 0 ? pnbi + sm.kl[kl_] : LR_NEG_INF;
        sm.spb[i] = nb_;
        sm.spnb[i] = nnb;
        sm.score[s] = lr_lse2(nb_, nnb);
        if constexpr (BIAS) {
          const float bo = bsm.bbank[cur][i] + bv.part[bsm.bnode[cur][i]];
          bsm.sbon[i] = bo;
          sm.score[s] += bo;
        }
      } else {
        const int k = j - 1;
        float sc = LR_NEG_INF;
        if (k < cnt) {
          const int c = sm.kc[k];
          if (c != blank) sc = (c == last ? pbi : lr_lse2(pbi, pnbi)) + sm.kl[k];
          if constexpr (LM) {
            if (sc > LR_NEG_INF) {
              const int role = lsm.role[c];
              if (role == kRoleSpace) sc += lsm.tterm[cur][i];   // 0 when the current word is empty
              else if (role == kRoleWord && lm_trie_find(L, lsm.tnode[cur][i], c).x < 0) sc = LR_NEG_INF;
            }
          }
          if constexpr (BIAS) {
            if (sc > LR_NEG_INF) {
              const int nn = bias_next(bv, bsm.bnode[cur][i], c);
              sc += (bsm.bbank[cur][i] + bv.out[nn]) + bv.part[nn];
            }
          }
        }
        sm.score[s] = sc;
      }
    }
    __syncthreads();

    // -- phase 3: an extension that is already in the beam merges into that hypothesis
    if (tid < nb && sm.depth[cur][tid] > 0) {
      const int k = sm.c2k[sm.cls[cur][tid]];
      int i = -1;
      if (k >= 0) {
        const uint64_t key = sm.hpar[cur][tid];
        const int pdepth = sm.depth[cur][tid] - 1, pnode = sm.par[cur][tid];
        for (uint32_t h = hash_slot(key);; h = (h + 1) & (kHash - 1)) {
          const int c = sm.hslot[h];
          if (c < 0) break;
          if (sm.hpre[cur][c] == key && sm.depth[cur][c] == pdepth &&
              (sm.node[cur][c] == pnode || same_prefix(sm.node[cur][c], pnode, gpar, gcls))) {
            i = c;
            break;
          }
        }
        if (i >= 0) {
          const int e = i * n1 + 1 + k;
          float m = sm.score[e];
          if constexpr (BIAS) {
            if (m > LR_NEG_INF) m = ext_mass<LM>(sm, lsm, cur, i, k);
          }
          sm.score[e] = LR_NEG_INF;
          const float pn = lr_lse2(sm.spnb[tid], m);
          sm.spnb[tid] = pn;
          sm.score[tid * n1] = lr_lse2(sm.spb[tid], pn);
          if constexpr (BIAS) sm.score[tid * n1] += bsm.sbon[tid];
        }
      }
    }
    __syncthreads();

    // -- phase 4: radix select of the W largest keys among the valid candidates
    bool take_all = false;
    uint64_t thr = 0;
    int need = W;
    for (int pass = 0, shift = 40; pass < 6; ++pass, shift -= 8) {
      int* hist = sm.hist[pass & 1];
      for (int s = tid; s < M; s += nt) {
        const float sc = sm.score[s];
        if (!(sc > LR_NEG_INF)) continue;
        const uint64_t key = cand_key(sc, s, n1, sm.kc);
        if (pass == 0 || (key >> (shift + 8)) == (thr >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1);
      }
      __syncthreads();
      if (tid < LR_WAVE) {
        const int lane = tid;
        int c4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) c4[r] = hist[255 - 4 * lane - r];   // digits in descending order
        const int loc = c4[0] + c4[1] + c4[2] + c4[3];
        int inc = loc;
#pragma unroll
        for (int off = 1; off < LR_WAVE; off <<= 1) {
          const int o = __shfl_up(inc, off);
          if (lane >= off) inc += o;
        }
        const int ex = inc - loc;
        if (ex < need && need <= inc) {
          int cum = ex;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (need <= cum + c4[r]) {
              sm.ctl[0] = 255 - 4 * lane - r; sm.ctl[1] = need - cum; sm.ctl[2] = c4[r];
              break;
            }
            cum += c4[r];
          }
        }
        if (lane == LR_WAVE - 1) sm.ctl[3] = inc;
      }
      __syncthreads();
      if (pass == 0 && sm.ctl[3] <= W) { take_all = true; break; }
      thr |= (uint64_t)sm.ctl[0] << shift;
      need = sm.ctl[1];
      const bool closed = sm.ctl[2] == need;
      // this histogram is read; the next pass uses the other one, cleared in phase 1 or two passes ago
      if (tid < 256) hist[tid] = 0;
      if (closed) break;   // every key >= thr is in, exactly W of them
      // (ctl is rewritten only by the next pass's scan, behind its histogram barrier)
    }

    // -- phase 5: compact the survivors, rank them, build the next beam
    for (int s = tid; s < M; s += nt) {
      const float sc = sm.score[s];
      if (!(sc > LR_NEG_INF)) continue;
      const uint64_t key = cand_key(sc, s, n1, sm.kc);
      if (take_all || key >= thr) {
        const int pos = atomicAdd(&sm.ctl[4], 1);
        if (pos < W) { sm.selkey[pos] = key; sm.selslot[pos] = s; }
      }
    }
    __syncthreads();
    int nsel = sm.ctl[4];
    nsel = nsel < W ? nsel : W;
    const int nxt = cur ^ 1;
    if (tid < nsel) {
      const uint64_t key = sm.selkey[tid];
      int r = 0;
      for (int q = 0; q < nsel; ++q) r += sm.selkey[q] > key;
      const int s = sm.selslot[tid];
      const int i = s / n1, j = s - i * n1;
      if (j == 0) {
        sm.node[nxt][r] = sm.node[cur][i]; sm.par[nxt][r] = sm.par[cur][i];
        sm.cls[nxt][r] = sm.cls[cur][i];   sm.depth[nxt][r] = sm.depth[cur][i];
        sm.pb[nxt][r] = sm.spb[i];         sm.pnb[nxt][r] = sm.spnb[i];
        sm.hpre[nxt][r] = sm.hpre[cur][i]; sm.hpar[nxt][r] = sm.hpar[cur][i];
        if constexpr (LM) {
          lsm.tnode[nxt][r] = lsm.tnode[cur][i]; lsm.tword[nxt][r] = lsm.tword[cur][i];
          lsm.tterm[nxt][r] = lsm.tterm[cur][i];
          for (int q = 0; q < kLmMaxCtx; ++q) lsm.ctx[nxt][r][q] = lsm.ctx[cur][i][q];
        }
        if constexpr (BIAS) { bsm.bnode[nxt][r] = bsm.bnode[cur][i]; bsm.bbank[nxt][r] = bsm.bbank[cur][i]; }
      } else {
        const int c = sm.kc[j - 1];
        const int id = 1 + t * W + r;
        const int p = sm.node[cur][i];
        __hip_atomic_store(gpar + id, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(gcls + id, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gfrm[id] = t;
        sm.node[nxt][r] = id; sm.par[nxt][r] = p; sm.cls[nxt][r] = c; sm.depth[nxt][r] = sm.depth[cur][i] + 1;
        sm.pb[nxt][r] = LR_NEG_INF;        sm.pnb[nxt][r] = sm.score[s];
        sm.hpre[nxt][r] = prefix_hash(sm.hpre[cur][i], c); sm.hpar[nxt][r] = sm.hpre[cur][i];
        if constexpr (BIAS) {
          const int nn = bias_next(bv, bsm.bnode[cur][i], c);
          sm.pnb[nxt][r] = ext_mass<LM>(sm, lsm, cur, i, j - 1);   // sm.score[s] is the key
          bsm.bnode[nxt][r] = nn; bsm.bbank[nxt][r] = bsm.bbank[cur][i] + bv.out[nn];
        }
        if constexpr (LM) {
          const int role = lsm.role[c], node = lsm.tnode[cur][i];
          int* ctx = lsm.ctx[nxt][r];
          const int* pctx = lsm.ctx[cur][i];
          if (role == kRoleWord) {
            // the word stays in the dictionary (phase 2 dropped the others); score the new current word once
            const int2 ch = lm_trie_find(L, node, c);
            for (int q = 0; q < kLmMaxCtx; ++q) ctx[q] = pctx[q];
            lsm.tnode[nxt][r] = ch.x; lsm.tword[nxt][r] = ch.y;
            lsm.tterm[nxt][r] = lma.alpha * lm_score(L, ctx, ch.y) + lma.beta;
          } else {
            // a space completes a non-empty word: it joins the context; a transparent class drops the run
            const bool push = role == kRoleSpace && node != 0;
            for (int q = 0; q < L.m; ++q) ctx[q] = push ? (q + 1 < L.m ? pctx[q + 1] : lsm.tword[cur][i]) : pctx[q];
            lsm.tnode[nxt][r] = 0; lsm.tword[nxt][r] = -1; lsm.tterm[nxt][r] = 0.f;
          }
        }
      }
    }
    if (tid < cnt) sm.c2k[sm.kc[tid]] = -1;
    __syncthreads();
    cur = nxt;
    nb = nsel;
  }

  // -- a session stops here: the beam goes back to the state as it stands, the end terms are beam_read_kernel's
  if constexpr (STREAM) {
    if (tid < nb) {
      const int64_t g = (int64_t)b * W + tid;
      ss.node[g] = sm.node[cur][tid]; ss.par[g] = sm.par[cur][tid]; ss.cls[g] = sm.cls[cur][tid];
      ss.depth[g] = sm.depth[cur][tid]; ss.pb[g] = sm.pb[cur][tid]; ss.pnb[g] = sm.pnb[cur][tid];
      ss.hpre[g] = sm.hpre[cur][tid]; ss.hpar[g] = sm.hpar[cur][tid];
      if constexpr (LM) {
        ss.tnode[g] = lsm.tnode[cur][tid]; ss.tword[g] = lsm.tword[cur][tid]; ss.tterm[g] = lsm.tterm[cur][tid];
        // the model's own context length only: the words beyond it are never read and may hold anything
        for (int q = 0; q < L.m; ++q) ss.ctx[g * kLmMaxCtx + q] = lsm.ctx[cur][tid][q];
      }
      if constexpr (BIAS) { ss.bnode[g] = bsm.bnode[cur][tid]; ss.bbank[g] = bsm.bbank[cur][tid]; }
    }
    if (tid == 0) { ss.hdr[b].frames = t0 + len; ss.hdr[b].nb = nb; }
    return;
  }

  // -- end of utterance (LM): the last word's term, then a stable re-sort by the final score
  if constexpr (LM) {
    if (tid < nb) lsm.fin[tid] = lr_lse2(sm.pb[cur][tid], sm.pnb[cur][tid]) + lsm.tterm[cur][tid];
    if constexpr (BIAS) {
      if (tid < nb) lsm.fin[tid] += bsm.bbank[cur][tid];
    }
    __syncthreads();
    if (tid < nb) {
      const float f = lsm.fin[tid];
      int r = 0;
      for (int q = 0; q < nb; ++q) r += lsm.fin[q] > f || (lsm.fin[q] == f && q < tid);
      lsm.perm[r] = tid;
    }
  }

  // -- end of utterance (hotwords without an LM): bonus_end, then the same stable re-sort
  if constexpr (BIAS && !LM) {
    if (tid < nb) bsm.fin[tid] = lr_lse2(sm.pb[cur][tid], sm.pnb[cur][tid]) + bsm.bbank[cur][tid];
    __syncthreads();
    if (tid < nb) {
      const float f = bsm.fin[tid];
      int r = 0;
      for (int q = 0; q < nb; ++q) r += bsm.fin[q] > f || (bsm.fin[q] == f && q < tid);
      bsm.perm[r] = tid;
    }
  }

  // -- output: every beam walks its node chain back to the root
  __threadfence();
  __syncthreads();
  const int64_t obase = (int64_t)b * W * T;
  // output rank r holds beam entry src(r)
  auto src = [&](int r) {
    if constexpr (LM) return lsm.perm[r];
    else if constexpr (BIAS) return bsm.perm[r];
    else return r;
  };
  for (int64_t e = tid; e < (int64_t)W * T; e += nt) {
    const int r = (int)(e / T), d = (int)(e - (int64_t)r * T);
    const int dep = r < nb ? sm.depth[cur][src(r)] : 0;
    if (d >= dep) { out_ids[obase + e] = -1; out_off[obase + e] = -1; }
  }
  if (tid < W) {
    out_lens[(int64_t)b * W + tid] = tid < nb ? sm.depth[cur][src(tid)] : 0;
    if constexpr (LM)
      out_scores[(int64_t)b * W + tid] = tid < nb ? -lsm.fin[src(tid)] : __builtin_inff();
    else if constexpr (BIAS)
      out_scores[(int64_t)b * W + tid] = tid < nb ? -bsm.fin[src(tid)] : __builtin_inff();
    else
      out_scores[(int64_t)b * W + tid] =
          tid < nb ? -lr_lse2(sm.pb[cur][tid], sm.pnb[cur][tid]) : __builtin_inff();
  }
  if (tid < nb) {
    int id = sm.node[cur][src(tid)];
    int32_t* ids = out_ids + obase + (int64_t)tid * T;
    int32_t* off = out_off + obase + (int64_t)tid * T;
    for (int d = sm.depth[cur][src(tid)] - 1; d >= 0; --d) {
      ids[d] = gcls[id];
      off[d] = gfrm[id];
      id = gpar[id];
    }
  }
}

// ---------------------------------------------------------------------------------------
// 3. sessions: reset and read (the advance is beam_loop_kernel<.., .., true>)
// ---------------------------------------------------------------------------------------
__host__ __device__ inline bool stream_shape_ok(int B, int max_frames, int W) {
  return B > 0 && max_frames > 0 && W > 0 && W <= kBeamMaxW && beam_nodes(max_frames, W) < INT32_MAX;
}

// Masked slots (all of them for mask == nullptr) go back to the empty prefix.  Under a mask the slot must already
// carry this configuration: the sections' places depend on it, and the other slots keep theirs.
__global__ __launch_bounds__(kStreamThreads) void beam_stream_reset_kernel(
    StreamLaunch ss, const int32_t* __restrict__ mask, int W, int variant, const uint8_t* __restrict__ lm,
    const uint8_t* __restrict__ bias) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (mask) {
    if (mask[b] == 0) return;
    const StreamHdr h = ss.hdr[b];
    if (h.magic != kStreamMagic || h.B != (int)gridDim.x || h.W != W || h.max_frames != ss.max_frames ||
        h.variant != variant) {
      if (tid == 0) ss.hdr[b].status = h.status | LR_BEAM_STREAM_MISMATCH;
      return;
    }
  }
  const int bos = (variant & 1) ? reinterpret_cast<const LmHeader*>(lm)->bos : 0;
  const int start = (variant & 2) ? reinterpret_cast<const BiasHeader*>(bias)->start : 0;
  for (int i = tid; i < W; i += blockDim.x) {
    const int64_t g = (int64_t)b * W + i;
    const bool root = i == 0;
    ss.node[g] = 0; ss.par[g] = root ? -1 : 0; ss.cls[g] = root ? -1 : 0; ss.depth[g] = 0;
    ss.pb[g] = 0.f; ss.pnb[g] = root ? LR_NEG_INF : 0.f;
    ss.hpre[g] = 0; ss.hpar[g] = 0;
    if (variant & 1) {
      ss.tnode[g] = 0; ss.tword[g] = root ? -1 : 0; ss.tterm[g] = 0.f;
      for (int q = 0; q < kLmMaxCtx; ++q) ss.ctx[g * kLmMaxCtx + q] = root ? bos : 0;
    }
    if (variant & 2) { ss.bnode[g] = root ? start : 0; ss.bbank[g] = 0.f; }
  }
  if (tid == 0) ss.hdr[b] = StreamHdr{kStreamMagic, (int)gridDim.x, W, ss.max_frames, variant, 0, 1, 0};
}

// What the one-shot search would put out if the slot's stream ended now: the variant's end terms, the stable re-sort,
// the chain walks; and the common prefix of all live hypotheses.  Reads the state only.  The layout comes from the
// slot's own header, checked against the buffer's size before anything else is read.
__global__ __launch_bounds__(kStreamThreads) void beam_read_kernel(
    const uint8_t* __restrict__ state, size_t state_bytes, int variant, int n_out, int out_width,
    int32_t* __restrict__ out_ids, int32_t* __restrict__ out_off, int32_t* __restrict__ out_lens,
    float* __restrict__ out_scores, int32_t* __restrict__ out_stable, int32_t* __restrict__ out_frames,
    int32_t* __restrict__ out_status) {
  __shared__ float fin[kBeamMaxW];
  __shared__ int perm[kBeamMaxW], node[kBeamMaxW], depth[kBeamMaxW];
  __shared__ int lcp;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const StreamHdr h = reinterpret_cast<const StreamHdr*>(state)[b];
  StreamState ss{};
  bool ok = h.magic == kStreamMagic && h.B == (int)gridDim.x && stream_shape_ok(h.B, h.max_frames, h.W) &&
            h.variant == variant && h.frames >= 0 && h.frames <= h.max_frames && h.nb >= 0 && h.nb <= h.W;
  ok = ok && stream_carve(const_cast<uint8_t*>(state), h.B, h.max_frames, h.W, h.variant, &ss) <= state_bytes;
  const int nb = ok ? h.nb : 0;
  const int W = ok ? h.W : 1;
  const int32_t* gpar = nullptr;
  const int32_t* gcls = nullptr;
  const int32_t* gfrm = nullptr;
  if (ok) {
    const int64_t nbase = (int64_t)b * beam_nodes(h.max_frames, W);
    gpar = ss.npar + nbase; gcls = ss.ncls + nbase; gfrm = ss.nfrm + nbase;
  }
  if (tid < nb) {
    const int64_t g = (int64_t)b * W + tid;
    node[tid] = ss.node[g];
    depth[tid] = ss.depth[g];
    // the one-shot end's own expressions, term by term
    float f = lr_lse2(ss.pb[g], ss.pnb[g]);
    if (variant & 1) f = f + ss.tterm[g];
    if (variant & 2) f = f + ss.bbank[g];
    fin[tid] = f;
  }
  __syncthreads();
  if (tid < nb) {
    int r = tid;   // without end terms the beam is in output order already
    if (variant != 0) {
      const float f = fin[tid];
      r = 0;
      for (int q = 0; q < nb; ++q) r += fin[q] > f || (fin[q] == f && q < tid);
    }
    perm[r] = tid;
  }
  if (tid == 0) lcp = nb > 0 ? depth[0] : 0;
  __syncthreads();

  const int64_t obase = (int64_t)b * n_out * out_width;
  for (int64_t e = tid; e < (int64_t)n_out * out_width; e += nt) {
    const int r = (int)(e / out_width), d = (int)(e - (int64_t)r * out_width);
    const int dep = r < nb ? depth[perm[r]] : 0;
    if (d >= dep) { out_ids[obase + e] = -1; out_off[obase + e] = -1; }
  }
  for (int r = tid; r < n_out; r += nt) {
    out_lens[(int64_t)b * n_out + r] = r < nb ? depth[perm[r]] : 0;   // the true length, whatever out_width
    out_scores[(int64_t)b * n_out + r] = r < nb ? -fin[perm[r]] : __builtin_inff();
  }
  if (tid < nb && tid < n_out) {
    int id = node[perm[tid]];
    int32_t* ids = out_ids + obase + (int64_t)tid * out_width;
    int32_t* off = out_off + obase + (int64_t)tid * out_width;
    for (int d = depth[perm[tid]] - 1; d >= 0; --d) {
      if (d < out_width) { ids[d] = gcls[id]; off[d] = gfrm[id]; }
      id = gpar[id];
    }
  }
  // the longest common prefix of all live hypotheses: each one against beam entry 0, both chains at equal depth;
  // the lowest position at which the classes differ bounds it
  if (tid < nb) {
    int a = node[tid], c = node[0], d = depth[tid], d0 = depth[0];
    for (; d > d0; --d) a = gpar[a];
    for (; d0 > d; --d0) c = gpar[c];
    int l = d;
    for (; d > 0 && a != c; --d) {
      if (gcls[a] != gcls[c]) l = d - 1;
      a = gpar[a];
      c = gpar[c];
    }
    atomicMin(&lcp, l);
  }
  __syncthreads();
  if (tid == 0) {
    out_stable[b] = lcp;
    out_frames[b] = ok ? h.frames : 0;
    out_status[b] = ok ? h.status : ((h.magic == kStreamMagic ? h.status : 0) | LR_BEAM_STREAM_MISMATCH);
  }
}

bool beam_supported(int T, int C, int W, int n) {
  return W <= kBeamMaxW && n <= kBeamMaxN && C <= kBeamMaxC && beam_nodes(T, W) < INT32_MAX;
}

size_t stream_ws_bytes(int B, int T, int n) {
  const size_t frames = (size_t)B * T;
  return lr_align_up(frames * n * 4, 256) * 2 + lr_align_up(frames * 4, 256);
}

template <bool LM, bool BIAS>
int stream_advance(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes, int log_input,
                   float cutoff_prob, int blank, const LoopArgs<BIAS>& lma, const StreamLaunch& ss, void* workspace,
                   int B, int T, int C, int W, int n, lr_stream_t stream) {
  const BeamWs w = beam_ws_carve(workspace, B, T, n, W);   // the node tables are the state's, not these
  const int64_t frames = (int64_t)B * T;
  LR_LAUNCH(beam_prune_kernel, dim3((unsigned)((frames + kPruneWaves - 1) / kPruneWaves)),
            dim3(kPruneWaves * LR_WAVE), 0, stream, probs, stride_b, stride_t, sizes, log_input, cutoff_prob,
            w.kcls, w.klp, w.kcnt, B, T, C, n);
  const int st = lr_launch_status();
  if (st != LR_OK) return st;
  LR_LAUNCH((beam_loop_kernel<LM, BIAS, true>), dim3(B), dim3(kLoopThreads), 0, stream, w.kcls, w.klp, w.kcnt, sizes,
            ss.npar, ss.ncls, ss.nfrm, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, T, W,
            n, blank, C, lma, ss);
  return lr_launch_status();
}

uint64_t pow2_at_least(uint64_t x) {
  uint64_t p = 16;
  while (p < x) p <<= 1;
  return p;
}

struct LmSizes {
  int64_t higher;    // n-grams of order >= 2
  uint64_t nslots, tslots;
  size_t uni_off, ngram_off, trie_off, bytes;
};

// 0 for orders and vocabularies the blob does not hold (LR_ERR_UNSUPPORTED), -1 for bad arguments
int lm_sizes(int order, const int64_t* counts, int64_t dict_chars, LmSizes* z) {
  if (order < 1 || !counts || dict_chars < 0) return -1;
  if (order > kLmMaxOrder) return 0;
  if (counts[0] < 1) return -1;
  if (counts[0] >= kLmMaxVocab) return 0;
  z->higher = 0;
  for (int k = 1; k < order; ++k) {
    if (counts[k] < 0) return -1;
    z->higher += counts[k];
  }
  if (z->higher > ((int64_t)1 << 36) || dict_chars >= ((int64_t)1 << 30)) return 0;
  z->nslots = pow2_at_least(2 * (uint64_t)z->higher);
  z->tslots = pow2_at_least(2 * (uint64_t)dict_chars);
  z->uni_off = kLmHeaderBytes;
  z->ngram_off = lr_align_up(z->uni_off + (size_t)counts[0] * sizeof(float2), 16);
  z->trie_off = z->ngram_off + z->nslots * sizeof(LmNgram);
  z->bytes = z->trie_off + z->tslots * sizeof(LmTrie);
  return 1;
}

// host-side open addressing over the blob's tables (the device reads them with lm_ngram_find / lm_trie_find)
template <class Slot>
Slot* host_probe(Slot* tab, uint64_t mask, uint64_t key) {
  for (uint64_t s = lm_mix(key) & mask;; s = (s + 1) & mask)
    if (tab[s].key == key || tab[s].key == kLmEmpty) return tab + s;
}

// the hotword automaton on the host: Aho-Corasick over the (anchor-prefixed) phrases, as a dense table
struct BiasAuto {
  int nodes = 0, start = 0;
  std::vector<int32_t> next;        // [nodes][C]: the trie's edges while it is built, the resolved table afterwards
  std::vector<double> out, part;    // [nodes]
};

// 1: built; 0: more phrases, nodes or classes than the blob holds (LR_ERR_UNSUPPORTED); -1: bad arguments.
// weights == nullptr counts the nodes only.
int bias_build(int n_phrases, const int64_t* off, const int32_t* cls, const float* weights, int anchor, int C,
               BiasAuto* a) {
  if (n_phrases < 1 || !off || !cls || C < 1 || off[0] != 0) return -1;
  if (C > kBeamMaxC) return 0;
  if (anchor < -1 || anchor >= C) return -1;
  for (int k = 0; k < n_phrases; ++k) {
    if (off[k + 1] <= off[k]) return -1;   // an empty phrase
    for (int64_t j = off[k]; j < off[k + 1]; ++j)
      if (cls[j] < 0 || cls[j] >= C) return -1;
    if (weights && !(isfinite(weights[k]) && weights[k] > 0.f)) return -1;
  }
  if (n_phrases > kBiasMaxPhrases) return 0;
  std::vector<int32_t>& next = a->next;
  std::vector<double> own(1, 0.0), val(1, 0.0);   // weights ending at the node; its best partial credit
  next.assign(C, -1);
  int nodes = 1;
  auto child = [&](int node, int c) {
    if (next[(size_t)node * C + c] < 0) {
      next[(size_t)node * C + c] = nodes++;
      next.resize((size_t)nodes * C, -1);
      own.push_back(0.0);
      val.push_back(0.0);
    }
    return next[(size_t)node * C + c];
  };
  a->start = anchor >= 0 ? child(0, anchor) : 0;
  for (int k = 0; k < n_phrases; ++k) {
    const int64_t m = off[k + 1] - off[k];
    const double w = weights ? (double)weights[k] : 0.0;
    int node = a->start;
    for (int64_t j = 1; j <= m; ++j) {
      node = child(node, cls[off[k] + j - 1]);
      if (nodes > kBiasMaxNodes) return 0;
      if (j < m) val[node] = fmax(val[node], w * (double)j / (double)m);
      else own[node] += w;
    }
  }
  a->nodes = nodes;
  if (!weights) return 1;
  // breadth first: a node's fail target is shallower, so its row, out and part are final when the node is reached
  std::vector<int> fail(nodes, 0), queue;
  queue.reserve(nodes);
  a->out.assign(nodes, 0.0);
  a->part.assign(nodes, 0.0);
  for (int c = 0; c < C; ++c) {
    const int u = next[c];
    if (u < 0) next[c] = 0;
    else queue.push_back(u);
  }
  for (size_t h = 0; h < queue.size(); ++h) {
    const int u = queue[h], f = fail[u];
    a->out[u] = own[u] + a->out[f];
    a->part[u] = fmax(val[u], a->part[f]);
    for (int c = 0; c < C; ++c) {
      int32_t& e = next[(size_t)u * C + c];
      const int via = next[(size_t)f * C + c];
      if (e < 0) e = via;
      else { fail[e] = via; queue.push_back(e); }
    }
  }
  return 1;
}

size_t bias_bytes(int nodes, int C) {
  return lr_align_up(sizeof(BiasHeader) + (size_t)nodes * C * 4 + (size_t)nodes * 8, 16);
}

// the two hotword entry points: lr_ctc_beam_decode / lr_ctc_beam_lm_decode with the bias instantiation of the loop
template <bool LM>
int beam_bias_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes, int log_input,
                     int cutoff_top_n, float cutoff_prob, int beam_width, int blank, const LmArgs& lma,
                     const void* bias, int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens, float* out_scores,
                     void* workspace, size_t workspace_bytes, int B, int T, int C, lr_stream_t stream) {
  LR_CHECK_ARG(probs && out_ids && out_offsets && out_lens && out_scores && workspace && bias);
  LR_CHECK_ARG(B > 0 && T > 0 && C > 0 && beam_width > 0 && cutoff_top_n > 0);
  LR_CHECK_ARG(blank >= 0 && blank < C && !(cutoff_prob != cutoff_prob));
  if (!beam_supported(T, C, beam_width, cutoff_top_n)) return LR_ERR_UNSUPPORTED;
  const int W = beam_width, n = cutoff_top_n;
  if (workspace_bytes < beam_ws_bytes(B, T, n, W)) return LR_ERR_WORKSPACE;
  const BeamWs w = beam_ws_carve(workspace, B, T, n, W);
  const int64_t frames = (int64_t)B * T;
  LR_LAUNCH(beam_prune_kernel, dim3((unsigned)((frames + kPruneWaves - 1) / kPruneWaves)),
            dim3(kPruneWaves * LR_WAVE), 0, stream, probs, stride_b, stride_t, sizes, log_input, cutoff_prob,
            w.kcls, w.klp, w.kcnt, B, T, C, n);
  int st = lr_launch_status();
  if (st != LR_OK) return st;
  LR_LAUNCH((beam_loop_kernel<LM, true>), dim3(B), dim3(kLoopThreads), 0, stream, w.kcls, w.klp, w.kcnt, sizes,
            w.npar, w.ncls, w.nfrm, out_ids, out_offsets, out_lens, out_scores, T, W, n, blank, C,
            BiasLmArgs{lma, static_cast<const uint8_t*>(bias)}, NoStream{});
  return lr_launch_status();
}

}  // namespace

extern "C" size_t lr_ctc_beam_workspace_bytes(int B, int T, int C, int beam_width, int cutoff_top_n) {
  if (B <= 0 || T <= 0 || C <= 0 || beam_width <= 0 || cutoff_top_n <= 0) return 0;
  if (!beam_supported(T, C, beam_width, cutoff_top_n)) return 0;
  return beam_ws_bytes(B, T, cutoff_top_n, beam_width);
}

extern "C" int lr_ctc_beam_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                  int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                                  int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens, float* out_scores,
                                  void* workspace, size_t workspace_bytes, int B, int T, int C, lr_stream_t stream) {
  LR_CHECK_ARG(probs && out_ids && out_offsets && out_lens && out_scores && workspace);
  LR_CHECK_ARG(B > 0 && T > 0 && C > 0 && beam_width > 0 && cutoff_top_n > 0);
  LR_CHECK_ARG(blank >= 0 && blank < C && !(cutoff_prob != cutoff_prob));
  if (!beam_supported(T, C, beam_width, cutoff_top_n)) return LR_ERR_UNSUPPORTED;
  const int W = beam_width, n = cutoff_top_n;
  if (workspace_bytes < beam_ws_bytes(B, T, n, W)) return LR_ERR_WORKSPACE;
  const BeamWs w = beam_ws_carve(workspace, B, T, n, W);
  const int64_t frames = (int64_t)B * T;
  LR_LAUNCH(beam_prune_kernel, dim3((unsigned)((frames + kPruneWaves - 1) / kPruneWaves)),
            dim3(kPruneWaves * LR_WAVE), 0, stream, probs, stride_b, stride_t, sizes, log_input, cutoff_prob,
            w.kcls, w.klp, w.kcnt, B, T, C, n);
  int st = lr_launch_status();
  if (st != LR_OK) return st;
  LR_LAUNCH((beam_loop_kernel<false, false>), dim3(B), dim3(kLoopThreads), 0, stream, w.kcls, w.klp, w.kcnt, sizes,
            w.npar, w.ncls, w.nfrm, out_ids, out_offsets, out_lens, out_scores, T, W, n, blank, C, LmArgs{}, NoStream{});
  return lr_launch_status();
}

extern "C" size_t lr_ctc_beam_lm_pack_bytes(int order, const int64_t* counts, int64_t dict_chars) {
  LmSizes z;
  return lm_sizes(order, counts, dict_chars, &z) == 1 ? z.bytes : 0;
}

extern "C" int lr_ctc_beam_lm_pack(void* out, size_t out_bytes, int order, const int64_t* counts,
                                   const int32_t* words, const double* log10_prob, const double* log10_backoff,
                                   int bos, int64_t dict_n, const int32_t* dict_word, const int64_t* dict_off,
                                   const int32_t* dict_cls, int n_classes) {
  LR_CHECK_ARG(out && words && log10_prob && log10_backoff && dict_n >= 0 && dict_off);
  LR_CHECK_ARG(dict_n == 0 || (dict_word && dict_cls));
  LR_CHECK_ARG(n_classes > 0 && n_classes <= kBeamMaxC);
  LmSizes z;
  const int ok = lm_sizes(order, counts, dict_off[dict_n], &z);
  if (ok == 0) return LR_ERR_UNSUPPORTED;
  if (ok < 0) return LR_ERR_INVALID_ARG;
  if (out_bytes < z.bytes) return LR_ERR_WORKSPACE;
  const int64_t V = counts[0];
  LR_CHECK_ARG(bos >= -1 && bos < V);
  const double ln10 = 2.302585092994045684;
  uint8_t* blob = static_cast<uint8_t*>(out);
  memset(blob, 0, z.ngram_off);
  memset(blob + z.ngram_off, 0xff, z.bytes - z.ngram_off);   // every key kLmEmpty
  LmHeader* h = reinterpret_cast<LmHeader*>(blob);
  h->magic = kLmMagic; h->version = kLmVersion; h->order = order; h->vocab = (int32_t)V; h->bos = bos; h->pad_ = 0;
  h->ngram_slots = (int64_t)z.nslots; h->trie_slots = (int64_t)z.tslots;
  h->uni_off = (int64_t)z.uni_off; h->ngram_off = (int64_t)z.ngram_off; h->trie_off = (int64_t)z.trie_off;
  h->bytes = (int64_t)z.bytes;
  float2* uni = reinterpret_cast<float2*>(blob + z.uni_off);
  LmNgram* ng = reinterpret_cast<LmNgram*>(blob + z.ngram_off);
  LmTrie* tr = reinterpret_cast<LmTrie*>(blob + z.trie_off);
  // n-grams, lower orders first so that every prefix already has its entry id
  int64_t row = 0;
  const int32_t* w = words;
  for (int k = 1; k <= order; ++k) {
    for (int64_t i = 0; i < counts[k - 1]; ++i, ++row, w += k) {
      for (int q = 0; q < k; ++q) LR_CHECK_ARG(w[q] >= 0 && w[q] < V);
      const float lp = (float)(log10_prob[row] * ln10), lbow = (float)(log10_backoff[row] * ln10);
      if (k == 1) {
        LR_CHECK_ARG(w[0] == i);   // unigram i is word id i
        uni[i] = make_float2(lp, lbow);
        continue;
      }
      int64_t e = 1 + w[0];
      for (int q = 1; q + 1 < k; ++q) {
        const LmNgram* g = host_probe(ng, z.nslots - 1, lm_ngram_key(e, w[q]));
        LR_CHECK_ARG(g->key != kLmEmpty);   // the (k-1)-gram prefix is not listed
        e = V + 1 + (g - ng);
      }
      const uint64_t key = lm_ngram_key(e, w[k - 1]);
      LmNgram* g = host_probe(ng, z.nslots - 1, key);
      LR_CHECK_ARG(g->key == kLmEmpty);     // a duplicate n-gram
      g->key = key; g->lp = lp; g->lbow = lbow;
    }
  }
  // the vocabulary trie over class ids
  int32_t nodes = 1;
  for (int64_t d = 0; d < dict_n; ++d) {
    const int64_t a = dict_off[d], b = dict_off[d + 1];
    LR_CHECK_ARG(a < b && dict_word[d] >= 0 && dict_word[d] < V);
    int32_t node = 0;
    LmTrie* e = nullptr;
    for (int64_t j = a; j < b; ++j) {
      LR_CHECK_ARG(dict_cls[j] >= 0 && dict_cls[j] < n_classes);
      const uint64_t key = lm_trie_key(node, dict_cls[j]);
      e = host_probe(tr, z.tslots - 1, key);
      if (e->key == kLmEmpty) { e->key = key; e->child = nodes++; e->word = -1; }
      node = e->child;
    }
    LR_CHECK_ARG(e->word < 0);   // two words with one spelling
    e->word = dict_word[d];
  }
  return LR_OK;
}

extern "C" int lr_ctc_beam_lm_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                     int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                                     const void* lm, const int32_t* class_roles, float alpha, float beta,
                                     int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens, float* out_scores,
                                     void* workspace, size_t workspace_bytes, int B, int T, int C, lr_stream_t stream) {
  LR_CHECK_ARG(probs && out_ids && out_offsets && out_lens && out_scores && workspace && lm && class_roles);
  LR_CHECK_ARG(B > 0 && T > 0 && C > 0 && beam_width > 0 && cutoff_top_n > 0);
  LR_CHECK_ARG(blank >= 0 && blank < C && !(cutoff_prob != cutoff_prob));
  LR_CHECK_ARG(isfinite(alpha) && isfinite(beta));
  if (!beam_supported(T, C, beam_width, cutoff_top_n)) return LR_ERR_UNSUPPORTED;
  const int W = beam_width, n = cutoff_top_n;
  if (workspace_bytes < beam_ws_bytes(B, T, n, W)) return LR_ERR_WORKSPACE;
  const BeamWs w = beam_ws_carve(workspace, B, T, n, W);
  const int64_t frames = (int64_t)B * T;
  LR_LAUNCH(beam_prune_kernel, dim3((unsigned)((frames + kPruneWaves - 1) / kPruneWaves)),
            dim3(kPruneWaves * LR_WAVE), 0, stream, probs, stride_b, stride_t, sizes, log_input, cutoff_prob,
            w.kcls, w.klp, w.kcnt, B, T, C, n);
  int st = lr_launch_status();
  if (st != LR_OK) return st;
  const LmArgs lma{static_cast<const uint8_t*>(lm), class_roles, alpha, beta};
  LR_LAUNCH((beam_loop_kernel<true, false>), dim3(B), dim3(kLoopThreads), 0, stream, w.kcls, w.klp, w.kcnt, sizes,
            w.npar, w.ncls, w.nfrm, out_ids, out_offsets, out_lens, out_scores, T, W, n, blank, C, lma, NoStream{});
  return lr_launch_status();
}

extern "C" size_t lr_ctc_beam_bias_pack_bytes(int n_phrases, const int64_t* phrase_off, const int32_t* phrase_cls,
                                              int anchor, int n_classes) {
  BiasAuto a;
  return bias_build(n_phrases, phrase_off, phrase_cls, nullptr, anchor, n_classes, &a) == 1
             ? bias_bytes(a.nodes, n_classes) : 0;
}

extern "C" int lr_ctc_beam_bias_pack(void* out, size_t out_bytes, int n_phrases, const int64_t* phrase_off,
                                     const int32_t* phrase_cls, const float* weights, int anchor, int n_classes) {
  LR_CHECK_ARG(out && weights);
  BiasAuto a;
  const int ok = bias_build(n_phrases, phrase_off, phrase_cls, weights, anchor, n_classes, &a);
  if (ok == 0) return LR_ERR_UNSUPPORTED;
  if (ok < 0) return LR_ERR_INVALID_ARG;
  const int C = n_classes;
  const size_t bytes = bias_bytes(a.nodes, C);
  if (out_bytes < bytes) return LR_ERR_WORKSPACE;
  uint8_t* blob = static_cast<uint8_t*>(out);
  memset(blob, 0, bytes);
  BiasHeader* h = reinterpret_cast<BiasHeader*>(blob);
  h->magic = kBiasMagic; h->version = kBiasVersion; h->nodes = a.nodes; h->stride = C; h->start = a.start;
  h->phrases = n_phrases; h->anchor = anchor; h->pad_ = 0;
  h->next_off = (int64_t)sizeof(BiasHeader);
  h->out_off = h->next_off + (int64_t)a.nodes * C * 4;
  h->part_off = h->out_off + (int64_t)a.nodes * 4;
  h->bytes = (int64_t)bytes;
  memcpy(blob + h->next_off, a.next.data(), (size_t)a.nodes * C * 4);
  float* fo = reinterpret_cast<float*>(blob + h->out_off);
  float* fp = reinterpret_cast<float*>(blob + h->part_off);
  for (int u = 0; u < a.nodes; ++u) { fo[u] = (float)a.out[u]; fp[u] = (float)a.part[u]; }
  return LR_OK;
}

extern "C" int lr_ctc_beam_bias_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                       int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                                       const void* bias, int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens,
                                       float* out_scores, void* workspace, size_t workspace_bytes, int B, int T, int C,
                                       lr_stream_t stream) {
  return beam_bias_decode<false>(probs, stride_b, stride_t, sizes, log_input, cutoff_top_n, cutoff_prob, beam_width,
                                 blank, LmArgs{}, bias, out_ids, out_offsets, out_lens, out_scores, workspace,
                                 workspace_bytes, B, T, C, stream);
}

extern "C" int lr_ctc_beam_lm_bias_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                          int log_input, int cutoff_top_n, float cutoff_prob, int beam_width,
                                          int blank, const void* lm, const int32_t* class_roles, float alpha,
                                          float beta, const void* bias, int32_t* out_ids, int32_t* out_offsets,
                                          int32_t* out_lens, float* out_scores, void* workspace,
                                          size_t workspace_bytes, int B, int T, int C, lr_stream_t stream) {
  LR_CHECK_ARG(lm && class_roles && isfinite(alpha) && isfinite(beta));
  const LmArgs lma{static_cast<const uint8_t*>(lm), class_roles, alpha, beta};
  return beam_bias_decode<true>(probs, stride_b, stride_t, sizes, log_input, cutoff_top_n, cutoff_prob, beam_width,
                                blank, lma, bias, out_ids, out_offsets, out_lens, out_scores, workspace,
                                workspace_bytes, B, T, C, stream);
}

// ---- sessions: the same searches fed chunk by chunk ----

extern "C" size_t lr_ctc_beam_stream_state_bytes(int B, int max_frames, int beam_width, int with_lm, int with_bias) {
  if (!stream_shape_ok(B, max_frames, beam_width)) return 0;
  StreamState s;
  return stream_carve(nullptr, B, max_frames, beam_width, stream_variant(with_lm != 0, with_bias != 0), &s);
}

extern "C" size_t lr_ctc_beam_stream_workspace_bytes(int B, int chunk_T, int C, int beam_width, int cutoff_top_n) {
  if (B <= 0 || chunk_T <= 0 || C <= 0 || beam_width <= 0 || cutoff_top_n <= 0) return 0;
  if (beam_width > kBeamMaxW || cutoff_top_n > kBeamMaxN || C > kBeamMaxC) return 0;
  if ((int64_t)B * chunk_T >= INT32_MAX) return 0;
  return stream_ws_bytes(B, chunk_T, cutoff_top_n);
}

extern "C" int lr_ctc_beam_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int B, int max_frames,
                                        int beam_width, int with_lm, int with_bias, const void* lm, const void* bias,
                                        lr_stream_t stream) {
  LR_CHECK_ARG(state && B > 0 && max_frames > 0 && beam_width > 0);
  LR_CHECK_ARG((with_lm != 0) == (lm != nullptr) && (with_bias != 0) == (bias != nullptr));
  if (!stream_shape_ok(B, max_frames, beam_width)) return LR_ERR_UNSUPPORTED;
  const int variant = stream_variant(with_lm != 0, with_bias != 0);
  StreamLaunch ss{};
  if (state_bytes < stream_carve(state, B, max_frames, beam_width, variant, &ss)) return LR_ERR_WORKSPACE;
  ss.max_frames = max_frames;
  LR_LAUNCH(beam_stream_reset_kernel, dim3(B), dim3(kStreamThreads), 0, stream, ss, mask, beam_width, variant,
            static_cast<const uint8_t*>(lm), static_cast<const uint8_t*>(bias));
  return lr_launch_status();
}

extern "C" int lr_ctc_beam_stream_advance(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                          int log_input, int cutoff_top_n, float cutoff_prob, int beam_width,
                                          int blank, const void* lm, const int32_t* class_roles, float alpha,
                                          float beta, const void* bias, void* state, size_t state_bytes,
                                          int max_frames, void* workspace, size_t workspace_bytes, int B, int chunk_T,
                                          int C, lr_stream_t stream) {
  LR_CHECK_ARG(probs && state && workspace);
  LR_CHECK_ARG(B > 0 && chunk_T > 0 && C > 0 && beam_width > 0 && cutoff_top_n > 0 && max_frames > 0);
  LR_CHECK_ARG(blank >= 0 && blank < C && !(cutoff_prob != cutoff_prob));
  LR_CHECK_ARG(!lm || (class_roles && isfinite(alpha) && isfinite(beta)));
  const int W = beam_width, n = cutoff_top_n;
  if (!stream_shape_ok(B, max_frames, W) || n > kBeamMaxN || C > kBeamMaxC || (int64_t)B * chunk_T >= INT32_MAX)
    return LR_ERR_UNSUPPORTED;
  const int variant = stream_variant(lm != nullptr, bias != nullptr);
  StreamLaunch ss{};
  if (state_bytes < stream_carve(state, B, max_frames, W, variant, &ss)) return LR_ERR_WORKSPACE;
  ss.max_frames = max_frames;
  if (workspace_bytes < stream_ws_bytes(B, chunk_T, n)) return LR_ERR_WORKSPACE;
  const LmArgs lma{static_cast<const uint8_t*>(lm), class_roles, alpha, beta};
  const BiasLmArgs bla{lma, static_cast<const uint8_t*>(bias)};
  switch (variant) {
    case 0:
      return stream_advance<false, false>(probs, stride_b, stride_t, sizes, log_input, cutoff_prob, blank, lma, ss,
                                          workspace, B, chunk_T, C, W, n, stream);
    case 1:
      return stream_advance<true, false>(probs, stride_b, stride_t, sizes, log_input, cutoff_prob, blank, lma, ss,
                                         workspace, B, chunk_T, C, W, n, stream);
    case 2:
      return stream_advance<false, true>(probs, stride_b, stride_t, sizes, log_input, cutoff_prob, blank, bla, ss,
                                         workspace, B, chunk_T, C, W, n, stream);
    default:
      return stream_advance<true, true>(probs, stride_b, stride_t, sizes, log_input, cutoff_prob, blank, bla, ss,
                                        workspace, B, chunk_T, C, W, n, stream);
  }
}

extern "C" int lr_ctc_beam_stream_read(const void* state, size_t state_bytes, const void* lm, float alpha, float beta,
                                       const void* bias, int n_out, int out_width, int32_t* out_ids,
                                       int32_t* out_offsets, int32_t* out_lens, float* out_scores, int32_t* out_stable,
                                       int32_t* out_frames, int32_t* out_status, int B, lr_stream_t stream) {
  LR_CHECK_ARG(state && out_ids && out_offsets && out_lens && out_scores && out_stable && out_frames && out_status);
  LR_CHECK_ARG(B > 0 && n_out > 0 && out_width > 0);
  LR_CHECK_ARG(!lm || (isfinite(alpha) && isfinite(beta)));
  if (n_out > kBeamMaxW) return LR_ERR_UNSUPPORTED;
  if (state_bytes < lr_align_up((size_t)B * sizeof(StreamHdr), 256)) return LR_ERR_WORKSPACE;
  LR_LAUNCH(beam_read_kernel, dim3(B), dim3(kStreamThreads), 0, stream, static_cast<const uint8_t*>(state),
            state_bytes, stream_variant(lm != nullptr, bias != nullptr), n_out, out_width, out_ids, out_offsets,
            out_lens, out_scores, out_stable, out_frames, out_status);
  return lr_launch_status();
}
