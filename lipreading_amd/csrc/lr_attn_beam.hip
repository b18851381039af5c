// lr_attn_beam.hip — deterministic beam search through the attention decoder on gfx950.
//
// Reference capability replaced here (paths under the reference root):
//   src/models/lipreader/analysis.py:12-66  inference(): a beam search through CharDecodingStep that stops
//       at EOS, one utterance at a time on the host, one decoding_step call per candidate;
//   src/scripts/train.py:323-331            its use ("student-forcing outputs with beam search", beam_width
//       10, max_label_len 100).
//
// Specification (per utterance b, beam width K, cap Lmax = max_label_len):
//   * A hypothesis is (history, state, score).  The start beam holds one: empty history, the encoder's final
//     state for b (every decoder layer's h, plus c for the LSTM), score 0.
//   * A hypothesis is finished when its last token is EOS, or when len(history) == Lmax + 1 (the reference's
//     len(history) > max_label_len).
//   * One round works through the beam in order, building a list:
//       - an unfinished hypothesis runs one CharDecodingStep step on its last token (BOS if the history is
//         empty) from its state, attending over b's encoder states masked by enc_lens[b].  That gives lp (the
//         masked log-softmax, V entries) and a new state.  Its candidates are the min(K, V - 2) tokens with the
//         largest lp, PAD and BOS excluded, listed by lp descending with ties to the lower id; each has score
//         score + lp[v] and the new state;
//       - a finished hypothesis contributes itself, unchanged, at its place in the list.
//     The new beam is the first K entries of the list after a STABLE sort by score, descending.
//     (Scores are carried in float64 on the device: a float32 running sum of ~100 log-probabilities loses ~1e-4.)
//   * The search stops when every hypothesis of the beam is finished: at most Lmax + 1 rounds.
//   * The result is the beam in order, best first: each entry's tokens (the final EOS included when it has
//     one), their count and its score — a plain sum of log-probabilities, no length normalisation.  Slots past
//     the beam's size (only when fewer than K complete hypotheses exist) have length 0 and score -inf.
// Departures from the reference:
//   1. The reference draws each hypothesis's beam_width candidates with multinomial(replacement=False); here
//      they are the top K, which makes the result reproducible and testable.
//   2. PAD and BOS are never candidates (the reference gives them weight ~1e-45 after masked_log_softmax).
//
// Structure.  Every beam row stays resident: R = B*K rows (row = b*K + k), dead or finished rows masked, so
// every shape is static.  One round is
//   * the step pieces of lr_decoder.hip at one step (lr_decoder_dev.h): the EW-table gather by each row's
//     input token; per layer lr_rnn_step_fwd run as step 0 from the rows' current state (packed into the
//     step kernel's slot by lr_rnn_pack_state), with the upper layers' W_ih GEMM; the attention as
//     lr_sgemm_batched_impl over batch = B with M = K (the beams stand where the steps stand in training), so
//     enc and the step-independent halves (GE, cE / se, PE) stay per utterance and are never copied K times;
//     the concat GEMMs; the output head without the multinomial draw;
//   * beam_select_kernel, one workgroup per utterance: the per-beam top-K over V, then the stable sort of the
//     <= K*K list by rank counting in LDS; it writes each new slot's parent, token, score, length and finished
//     flag, its history row (double-buffered, and the caller's out_ids row), the next round's input token,
//     and counts the utterance into the finished counter once all its hypotheses are finished;
//   * beam_reorder_kernel: every layer's h (and c) gathered by parent for the next round.
// The search never waits for the host.  Both new kernels of an utterance whose hypotheses are all finished
// return at once (a round of such an utterance changes nothing, by the rule), so the host may launch rounds
// past the end: it reads the finished counter (4 bytes) every `poll_every` rounds and stops launching when all
// B utterances are finished.  The results do not depend on poll_every.
//
// Limits (LR_ERR_UNSUPPORTED, workspace query 0): 1 <= K <= 32, 1 <= Lmax <= 65535, 3 <= V <= 1024,
// B * K <= 65535, the head's and the concat attention's LDS as in lr_decoder_forward; every RNN mode, every
// attention type, 1 .. LR_DEC_MAX_LAYERS layers.
//
// ---- Joint CTC/attention search (lr_decoder_joint_beam_search; Watanabe et al. 2017) ----
// Inputs beyond the above, per utterance b: CTC log-probs y[b, t, c] for t < T_b = enc_lens[b], C = V + 1 classes,
// class 0 blank and decoder token v = class v + 1 (decoder.ctc_labels, the encoder head's layout); a weight lambda
// in [0, 1]; a pre-beam size P, min(K, V - 2) <= P <= min(64, V - 2) (default min(V - 2, ceil(1.5 K)) on the host).
//   * A hypothesis is (history g, state, attention score a, CTC score c); a is the sum of the decoder's lp as above,
//     c = log psi(g), and the joint score is s = (1 - lambda) a + lambda c (s = a exactly at lambda = 0, where c is
//     never computed; s = c at lambda = 1).
//   * CTC terms (log domain, float64).  BOS is not part of g.  Empty prefix: gamma^n_t = 0 (log -inf),
//     gamma^b_t = prod_{tau <= t} y_tau^blank, psi = 1.  Extension h = g + v, class k = v + 1:
//       phi_t = gamma^b_t(g) + (gamma^n_t(g) if last(g) != k else 0),  phi_{-1} = [g empty];
//       gamma^n_t(h) = (gamma^n_{t-1}(h) + phi_{t-1}) y_t^k,  gamma^n_{-1}(h) = 0;
//       gamma^b_t(h) = (gamma^b_{t-1}(h) + gamma^n_{t-1}(h)) y_t^blank,  gamma^b_{-1}(h) = 0;
//       psi(h) = sum_{t < T_b} phi_{t-1} y_t^k, the probability that the labelling starts with h.
//     The CTC head was trained with EOS as its last label, so EOS is an ordinary class; an EOS candidate completes
//     the hypothesis and its c is the full-sequence log(gamma^n_{T_b-1}(h) + gamma^b_{T_b-1}(h)), not log psi(h).
//   * Start: one hypothesis, empty history, the encoder's final state, a = c = s = 0.
//   * One round builds the list as above, except: an unfinished hypothesis's candidates are its P best tokens by lp
//     (PAD, BOS excluded, ties to the lower id), each with a' = a + lp[v], its c' and s'; when lambda > 0 a
//     candidate with c' = -inf (a structural zero: the prefix needs more frames than T_b) is not listed.  A finished
//     hypothesis lists itself unchanged (a capped one keeps its prefix score).  The new beam is the first K of a
//     STABLE sort by s.  An utterance whose list is empty is finished with an empty beam (length 0, score -inf).
//   * The output is as above, with s as the score.  At lambda = 0 it is lr_decoder_beam_search's, bit for bit: a
//     candidate ranked >= K within its own row cannot reach the top K.
// Structure.  The round's step pieces are the same launches; the selection becomes joint_score_kernel (one wave per
// row: the top P scan, then one lane per candidate running the recursion serially over t < T_b, the parent's
// arrays read at the same address by every lane) and beam_select_kernel<true> (the per-utterance stable sort of
// <= K*P entries; it also copies each surviving extension's arrays from the candidate buffer into its row).
// Each row's (gamma^n_t, gamma^b_t) live in the workspace, [R][T] double2, single-buffered: the score kernel reads
// them and writes candidates to cand [R][T][P] double2 (R*P*T*16 bytes, 5.8 MB at B = 32, K = 10, P = 15, T = 75);
// the select kernel reads only cand.  The CTC log-probs are read in place through (stride_b, stride_t).
// Extra limits: C = V + 1, blank = 0, lambda in [0, 1] (else LR_ERR_INVALID_ARG); the P range above and
// T <= 65535 (LR_ERR_UNSUPPORTED).  Precondition: 1 <= enc_lens[b] <= T (the kernels clamp it to stay in bounds).
//
// ---- Word language model fusion (lr_decoder_lm_beam_search) ----
// Everything in the joint specification holds; the following is added.  Inputs beyond the joint search's: the packed
// model of lr_ctc_beam_lm_pack (lr_lm_dev.h), class_roles[C] as in lr_ctc_beam_lm_decode (0 transparent, 1 word
// character, 2 space; a token's role is role[v + 1]: a blob packed for decoder.ctc_labels serves both searches), and
// alpha, beta as in BeamCTCDecoder.
//   * State.  A hypothesis also carries its language-model sum l in float64 (0 at the start), the trie node of its
//     current word (root at the start), that node's word id, the last order - 1 completed word ids (<s>-padded) and the
//     cached term alpha * lm(word | ctx) + beta of its current word: float64, from lm_score's fp32 value; 0 at the
//     root; a node that is only a prefix (word id -1) gives OOV = -1000.
//   * Dictionary.  For an unfinished hypothesis a word-character token whose class is not a child of the current trie
//     node is not a candidate: it is excluded before the top-P scan, as PAD and BOS are, so a row still lists its P
//     best remaining tokens, or all of them when fewer than P remain.
//   * Terms.  A space candidate adds the cached term when the current word is non-empty; the word id (-1 stays -1)
//     shifts into the context and the node returns to the root.  A leading or repeated space adds nothing.  An EOS
//     candidate also adds the cached term of a non-empty current word (the CTC search's End rule).  Any other
//     transparent token (UNK) drops the current run unscored and leaves the context unchanged.  A hypothesis finished
//     by the length cap keeps l as it is: its unfinished word is not scored.
//   * Score.  s = (1 - lambda) a + lambda c + l (s = c + l at lambda = 1; s = a + l at lambda = 0, where no CTC term
//     is computed and ctc_lp may be NULL).  Sorting, structural zeros, the finished rule and the outputs are unchanged.
//   * At lambda = 0 the result is no longer the plain search's: the terms reorder candidates across rows, so P matters.
// Structure.  joint_score_kernel<true> loads the row's node once, probes the trie for each word-character token a lane
// owns (the exclusion of the scan) and forms each candidate's l' from the cached term: no lookup.
// beam_select_kernel<true, true> loads the K parents' language-model state into LDS before it writes any row (rows
// are updated in place), then gives each survivor its new state: a word character costs one trie probe and one
// lm_score, a space shifts the context; a carried-over row keeps its state.  No global synchronisation: the hash
// probes end at the first empty slot of tables packed at load <= 1/2 (pass only blobs the packer produced).
// Extra limits: V + 1 <= 256 (the trie key holds the class in 8 bits; LR_ERR_UNSUPPORTED, workspace query 0);
// non-finite alpha or beta, or a NULL blob or roles pointer: LR_ERR_INVALID_ARG.
#include <type_traits>

#include "lr_common.h"
#include "lr_decoder_dev.h"
#include "lr_lm_dev.h"

namespace {

constexpr int BEAM_MAX_K = 32;
constexpr int BEAM_MAX_V = 1024;
constexpr int BEAM_MAX_LMAX = 65535;
constexpr int BEAM_JOINT_MAX_T = 65535;
constexpr int MAXL = LR_DEC_MAX_LAYERS;
constexpr int SEL_THREADS = 256;
constexpr int VPL = BEAM_MAX_V / 64;   // vocabulary entries per lane in the top-K scan

// per-utterance words of the search: history buffer in use, all-finished flag, rounds run
enum { U_CUR = 0, U_DONE = 1, U_ROUNDS = 2, U_WORDS = 4 };

inline int gates_of(int mode) { return mode == LR_RNN_GRU ? 3 : (mode == LR_RNN_LSTM ? 4 : 1); }

struct Sizes {
  int B, K, LH, T, Hd, Cd, V, A, G, type, NL;   // LH = Lmax + 1: history capacity
  int P;                                         // joint search: pre-beam size (0: the attention-only search)
  int LM;                                        // 1: with a word language model (its state is allocated)
};

// ---- workspace layout, in 4-byte words ------------------------------------------------------------------------
struct Ws {
  size_t EW, biasf[MAXL], wp[MAXL], hp[MAXL], gates[MAXL], extra[MAXL], y[MAXL], hcur[MAXL], ccur[MAXL];
  size_t ones, ids_used, logits, wts, ctx, pre, aux1, aux2, ph, lp;
  size_t score, len, fin, live, next_in, parent, hist, ustate, ctr, gemm, total;
  size_t hp_slot, gemm_bytes;
  size_t sa, sc, ent_tok, ent_s, ent_a, ent_c, gam, cand;   // joint search only (empty when P == 0)
  size_t lm_l, lm_node, lm_word, lm_term, lm_ctx, ent_l;    // language model only (empty when LM == 0)
};

Ws ws_layout(const Sizes& z) {
  Ws w;
  const size_t R = (size_t)z.B * z.K, GH = (size_t)z.G * z.Hd, BT = (size_t)z.B * z.T;
  const bool attn = z.type != ATT_NONE;
  size_t o = 0;
  auto take = [&](size_t n) { size_t at = o; o += (n + 63) / 64 * 64; return at; };
  w.EW = take((size_t)z.V * GH);
  w.hp_slot = lr_rnn_packed_state_floats((int)R, z.Hd);
  for (int k = 0; k < MAXL; ++k)
    w.biasf[k] = w.wp[k] = w.hp[k] = w.gates[k] = w.extra[k] = w.y[k] = w.hcur[k] = w.ccur[k] = 0;
  for (int k = 0; k < z.NL; ++k) {
    w.biasf[k] = take(GH);
    w.wp[k] = take(lr_rnn_packed_w_floats(z.G, z.Hd));
    w.hp[k] = take(2 * w.hp_slot);
    w.gates[k] = take(R * GH);
    w.extra[k] = take(R * z.Hd);
    w.y[k] = take(R * z.Hd);
    w.hcur[k] = take(R * z.Hd);
    w.ccur[k] = take(z.G == 4 ? R * z.Hd : 0);
  }
  w.ones = take(R);
  w.ids_used = take(R);
  w.logits = take(attn ? R * z.T : 0);
  w.wts = take(attn ? R * z.T : 0);
  w.ctx = take(attn ? R * z.Hd : 0);
  w.pre = take(attn ? R * z.Hd : 0);
  w.aux1 = take(z.type == ATT_GENERAL ? BT * z.Hd : (z.type == ATT_CONCAT ? BT * z.A : 0));   // GE | PE
  w.aux2 = take((z.type == ATT_GENERAL || z.type == ATT_1LNN) ? BT : 0);                       // cE | se
  w.ph = take(z.type == ATT_CONCAT ? R * z.A : 0);
  w.lp = take(R * z.V);
  w.score = take(2 * R);   // double
  w.len = take(R);
  w.fin = take(R);
  w.live = take(R);
  w.next_in = take(R);
  w.parent = take(R);
  w.hist = take(2 * R * z.LH);
  w.ustate = take((size_t)z.B * U_WORDS);
  w.ctr = take(2);   // {utterances finished, rounds run}
  const int a = z.A > 0 ? z.A : 1;
  const int dims[][3] = {{z.V, (int)GH, z.Cd}, {(int)BT, z.Hd, z.Hd}, {(int)BT, a, z.Hd}, {(int)R, z.Hd, z.Hd},
                         {(int)R, a, z.Hd}, {(int)R, (int)GH, z.Hd}};
  w.gemm_bytes = 0;
  for (const auto& d : dims) {
    const size_t g = lr_sgemm_workspace_bytes(d[0], d[1], d[2]);
    if (g > w.gemm_bytes) w.gemm_bytes = g;
  }
  w.gemm = take((w.gemm_bytes + 3) / 4);
  const size_t RP = R * z.P, RT = z.P ? R * z.T : 0;
  w.sa = take(z.P ? 2 * R : 0);        // double: attention score a
  w.sc = take(z.P ? 2 * R : 0);        // double: CTC score c
  w.ent_tok = take(RP);                // the round's list, entry (row, candidate)
  w.ent_s = take(2 * RP);
  w.ent_a = take(2 * RP);
  w.ent_c = take(2 * RP);
  w.gam = take(4 * RT);                // double2 (gamma^n, gamma^b) [R][T]: each row's CTC arrays
  w.cand = take(4 * RT * z.P);         // double2 [R][T][P]: each candidate's arrays, this round
  const size_t RL = z.LM ? R : 0;
  w.lm_l = take(2 * RL);               // double: language-model sum l
  w.lm_node = take(RL);                // trie node of the current word, and the word id it spells
  w.lm_word = take(RL);
  w.lm_term = take(2 * RL);            // double: cached term of the current word
  w.lm_ctx = take(RL * kLmMaxCtx);     // the last order - 1 completed word ids
  w.ent_l = take(z.LM ? 2 * RP : 0);   // double [R][P]: each entry's l'
  w.total = o;
  return w;
}

// rows of the output head per workgroup (lr_decoder_forward's rule); 0 when even one row does not fit
int head_rows(int Hd, int V) {
  int rows = OUT_ROWS;
  while (rows > 1 && (size_t)rows * (Hd + V) * sizeof(float) > 60 * 1024) rows >>= 1;
  return (size_t)rows * (Hd + V) * sizeof(float) > 60 * 1024 ? 0 : rows;
}

bool sizes_ok(int mode, int type, int NL, int B, int K, int Lmax, int T, int Hd, int Cd, int V, int A) {
  return (mode == LR_RNN_GRU || mode == LR_RNN_LSTM || mode == LR_RNN_TANH) && type >= ATT_NONE &&
         type <= ATT_CONCAT && NL >= 1 && NL <= MAXL && B > 0 && K >= 1 && K <= BEAM_MAX_K &&
         (int64_t)B * K <= 65535 && Lmax >= 1 && Lmax <= BEAM_MAX_LMAX && T > 0 && Hd > 0 && Hd % 4 == 0 &&
         Cd > 0 && V >= 3 && V <= BEAM_MAX_V && (type != ATT_CONCAT || (A > 0 && (size_t)2 * A * 4 <= 60 * 1024)) &&
         head_rows(Hd, V) > 0;
}

// the joint search's own limits: C = V + 1 classes, min(K, V - 2) <= P <= min(64, V - 2), T <= 65535
bool joint_ok(int K, int T, int V, int C, int P) {
  const int hi = V - 2 < 64 ? V - 2 : 64, lo = K < V - 2 ? K : V - 2;
  return C == V + 1 && P >= lo && P <= hi && T <= BEAM_JOINT_MAX_T;
}

// the fusion's own limit: the trie key holds the class v + 1 in 8 bits
bool lm_ok(int V) { return V + 1 <= 256; }

// dst[b*K + k][:] = src[b][:] for every k (the start state of every row of utterance b)
__global__ void beam_bcast_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int Hd) {
  const int r = blockIdx.x, b = r / K;
  const float4* s = reinterpret_cast<const float4*>(src + (int64_t)b * Hd);
  float4* d = reinterpret_cast<float4*>(dst + (int64_t)r * Hd);
  for (int c = threadIdx.x; c < Hd / 4; c += blockDim.x) d[c] = s[c];
}

// the start beam: row b*K holds (empty history, score 0); rows b*K + 1 .. are empty slots
__global__ void beam_init_kernel(double* score, int32_t* len, int32_t* fin, int32_t* live, int32_t* next_in,
                                 int32_t* parent, int32_t* ones, int32_t* ustate, int32_t* ctr, int R, int K, int bos) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) ctr[0] = ctr[1] = 0;
  if (r >= R) return;
  const int k = r % K;
  score[r] = 0.0;
  len[r] = 0;
  fin[r] = 0;
  live[r] = k == 0;
  next_in[r] = bos;
  parent[r] = r;
  ones[r] = 1;
  if (k == 0) {
    int32_t* u = ustate + (int64_t)(r / K) * U_WORDS;
    u[U_CUR] = 0;
    u[U_DONE] = 0;
    u[U_ROUNDS] = 0;
  }
}

template <typename S>
__device__ __forceinline__ bool ranks_before(S sa, int ia, S sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

struct ExcludeNone {
  __device__ __forceinline__ bool operator()(int) const { return false; }
};

// One wave's scan of one row's lp [V]: the n tokens with the largest lp, PAD, BOS and every v with excluded(v)
// left out, by lp descending with ties to the lower id.  emit(c, v, lp) runs on every lane for c = 0 .. n-1 (all lanes
// hold the same values); it stops early when fewer than n tokens remain.
template <typename F, typename X = ExcludeNone>
__device__ __forceinline__ void wave_topn(const float* __restrict__ row, int lane, int V, int pad, int bos, int n,
                                          F&& emit, X&& excluded = X()) {
  float val[VPL];
  unsigned avail = 0;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int v = lane + 64 * i;
    bool ok = v < V && v != pad && v != bos;
    if constexpr (!std::is_same<typename std::decay<X>::type, ExcludeNone>::value) ok = ok && !excluded(v);
    val[i] = ok ? row[v] : LR_NEG_INF;
    if (ok) avail |= 1u << i;
  }
  for (int c = 0; c < n; ++c) {
    float bv = LR_NEG_INF;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
      if (((avail >> i) & 1u) && ranks_before(val[i], lane + 64 * i, bv, bi)) { bv = val[i]; bi = lane + 64 * i; }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float ov = __shfl_xor(bv, d, 64);
      const int oi = __shfl_xor(bi, d, 64);
      if (ranks_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) break;   // (uniform) fewer than n tokens left: only with an exclusion (n <= V - 2)
    if ((bi & 63) == lane) avail &= ~(1u << (bi >> 6));
    emit(c, bi, bv);
  }
}

// The joint search's extra state (lr_decoder_joint_beam_search); unused by beam_select_kernel<false>.
struct JointState {
  const int32_t* ent_tok;   // [R][P] the round's list: token; -1 a finished hypothesis carried over; -2 no entry
  const double* ent_s;      // [R][P] joint score s', attention score a', CTC score c'
  const double* ent_a;
  const double* ent_c;
  double* sa;               // [R] each row's a and c (its s lives in `score`)
  double* sc;
  double2* gam;             // [R][T] each row's (gamma^n_t, gamma^b_t), log domain
  const double2* cand;      // [R][T][P] each candidate's arrays, written by joint_score_kernel
  const int32_t* enc_lens;
  int T, P, ctc;            // ctc: lambda > 0 (the CTC terms are computed and carried)
};

// The language model's state (lr_decoder_lm_beam_search); unused by the instantiations without one.
struct LmState {
  const uint8_t* blob;      // the packed model (lr_lm_dev.h)
  const int32_t* roles;     // [C] kRole*; token v has role roles[v + 1]
  float alpha, beta;
  int C;
  double* l;                // [R] each row's language-model sum
  int32_t* node;            // [R] trie node of the current word (0: the root, no current word)
  int32_t* word;            // [R] the word id that node spells (-1: only a prefix)
  double* term;             // [R] alpha * lm(word | ctx) + beta of the current word, 0 at the root
  int32_t* ctx;             // [R][kLmMaxCtx] the last order - 1 completed word ids, oldest first
  double* ent_l;            // [R][P] the round's list: l'
};

__device__ __forceinline__ int token_role(const LmState& lm, int v) {
  return v + 1 < lm.C ? lm.roles[v + 1] : kRoleTransparent;
}

__device__ __forceinline__ int utt_frames(const int32_t* enc_lens, int b, int T) {
  const int t = enc_lens[b];
  return t < 1 ? 1 : (t > T ? T : t);   // a precondition (1 <= enc_lens[b] <= T); clamped to stay in bounds
}

// One workgroup per utterance: the rule's round after the step pieces left each row's lp [R][V].
// Entry e = k*Kc + c of the round's list is candidate c of row k (c = 0 only for a finished row, which
// contributes itself); e is also the entry's place in the list, so the stable sort is a sort by (score desc, e).
// JOINT: the list was built by joint_score_kernel (Kc = P, score = the joint score s); the new rows also take
// their entry's a and c and, when the CTC terms are carried, their candidate's CTC arrays.
// LM (with JOINT): the new rows also take their entry's l and their language-model state, computed here from the
// parent's (held in LDS: a parent's row may be overwritten by an earlier slot).
template <bool JOINT, bool LM = false>
__global__ __launch_bounds__(SEL_THREADS) void beam_select_kernel(
    const float* __restrict__ lp, double* __restrict__ score, int32_t* __restrict__ len, int32_t* __restrict__ fin,
    int32_t* __restrict__ live, int32_t* __restrict__ next_in, int32_t* __restrict__ parent,
    int32_t* __restrict__ hist, int32_t* __restrict__ ustate, int32_t* __restrict__ ctr, int32_t* __restrict__ out_ids,
    int32_t* __restrict__ out_lens, float* __restrict__ out_scores, int K, int Kc, int V, int LH, int bos, int eos,
    int pad, JointState js, LmState lm) {
  static_assert(JOINT || !LM, "the language model rides on the joint search's list");
  constexpr int NEMAX = JOINT ? BEAM_MAX_K * 64 : BEAM_MAX_K * BEAM_MAX_K;
  __shared__ double e_score[NEMAX];
  __shared__ int e_tok[NEMAX];   // token; -1 = a finished hypothesis carried over; -2 = no entry
  __shared__ double o_score[BEAM_MAX_K];
  __shared__ int o_len[BEAM_MAX_K], o_state[BEAM_MAX_K];   // o_state: 0 empty slot, 1 unfinished, 2 finished
  __shared__ int sel[BEAM_MAX_K];
  __shared__ int n_sel, all_fin;
  __shared__ int p_node[LM ? BEAM_MAX_K : 1], p_word[LM ? BEAM_MAX_K : 1], p_ctx[LM ? BEAM_MAX_K : 1][kLmMaxCtx];
  __shared__ double p_term[LM ? BEAM_MAX_K : 1];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* u = ustate + (int64_t)b * U_WORDS;
  if (u[U_DONE]) return;   // (uniform) every hypothesis finished: a round changes nothing
  const int r0 = b * K;
  const int NE = K * Kc;
  if constexpr (JOINT) {
    if (tid < K) {
      o_len[tid] = len[r0 + tid];
      sel[tid] = -1;
      if constexpr (LM) {
        p_node[tid] = lm.node[r0 + tid];
        p_word[tid] = lm.word[r0 + tid];
        p_term[tid] = lm.term[r0 + tid];
        for (int q = 0; q < kLmMaxCtx; ++q) p_ctx[tid][q] = lm.ctx[(int64_t)(r0 + tid) * kLmMaxCtx + q];
      }
    }
    if (tid == 0) n_sel = 0;
    for (int e = tid; e < NE; e += SEL_THREADS) {
      e_tok[e] = js.ent_tok[(int64_t)r0 * Kc + e];
      e_score[e] = js.ent_s[(int64_t)r0 * Kc + e];
    }
    __syncthreads();
  } else {
    if (tid < K) {
      o_score[tid] = score[r0 + tid];
      o_len[tid] = len[r0 + tid];
      o_state[tid] = live[r0 + tid] ? (fin[r0 + tid] ? 2 : 1) : 0;
      sel[tid] = -1;
    }
    if (tid == 0) n_sel = 0;
    for (int e = tid; e < NE; e += SEL_THREADS) e_tok[e] = -2;
    __syncthreads();

    // candidates: one wave per row, Kc rounds of a wave argmax over the row's unused entries
    for (int k = wave; k < K; k += SEL_THREADS / 64) {
      const int st = o_state[k];
      if (st == 0) continue;
      if (st == 2) {
        if (lane == 0) { e_tok[k * Kc] = -1; e_score[k * Kc] = o_score[k]; }
        continue;
      }
      wave_topn(lp + (int64_t)(r0 + k) * V, lane, V, pad, bos, Kc, [&](int c, int v, float l) {
        if (lane == 0) { e_tok[k * Kc + c] = v; e_score[k * Kc + c] = o_score[k] + (double)l; }
      });
    }
    __syncthreads();
  }

  // stable sort, first K: an entry's rank is the count of entries before it in (score desc, place asc)
  for (int e = tid; e < NE; e += SEL_THREADS) {
    if (e_tok[e] == -2) continue;
    const double s = e_score[e];
    int rank = 0;
    for (int f = 0; f < NE && rank < K; ++f)
      if (e_tok[f] != -2 && ranks_before(e_score[f], f, s, e)) ++rank;
    if (rank < K) { sel[rank] = e; atomicAdd(&n_sel, 1); }
  }
  __syncthreads();

  // the new beam: slot s takes entry sel[s]
  const int nsel = n_sel;
  const int cur = u[U_CUR];
  const int32_t* hin = hist + ((int64_t)cur * gridDim.x + b) * K * LH;
  int32_t* hout = hist + ((int64_t)(cur ^ 1) * gridDim.x + b) * K * LH;
  int32_t* oid = out_ids + (int64_t)b * K * LH;
  for (int idx = tid; idx < K * LH; idx += SEL_THREADS) {
    const int s = idx / LH, t = idx - s * LH;
    int v = pad;
    if (s < nsel) {
      const int e = sel[s], k = e / Kc, tok = e_tok[e];
      const int l0 = o_len[k];
      if (t < l0) v = hin[k * LH + t];
      else if (t == l0 && tok >= 0) v = tok;
    }
    hout[idx] = v;
    oid[idx] = v;
  }
  if constexpr (JOINT) {
    // a new row that extends its parent takes the candidate's CTC arrays (a carried-over row never extends)
    if (js.ctc) {
      const int Tb = utt_frames(js.enc_lens, b, js.T);
      for (int idx = tid; idx < nsel * Tb; idx += SEL_THREADS) {
        const int s = idx / Tb, t = idx - s * Tb;
        const int e = sel[s], k = e / Kc, c = e - k * Kc;
        if (e_tok[e] >= 0)
          js.gam[(int64_t)(r0 + s) * js.T + t] = js.cand[((int64_t)(r0 + k) * js.T + t) * Kc + c];
      }
    }
  }
  if (tid == 0) all_fin = 1;
  __syncthreads();
  if (tid < K) {
    const int s = tid, r = r0 + s;
    if (s < nsel) {
      const int e = sel[s], k = e / Kc, tok = e_tok[e];
      const int nl = o_len[k] + (tok >= 0 ? 1 : 0);
      const bool f = tok < 0 || tok == eos || nl == LH;
      score[r] = e_score[e];
      if constexpr (JOINT) {
        js.sa[r] = js.ent_a[(int64_t)r0 * Kc + e];
        js.sc[r] = js.ent_c[(int64_t)r0 * Kc + e];
      }
      if constexpr (LM) {
        lm.l[r] = lm.ent_l[(int64_t)r0 * Kc + e];
        const int role = tok < 0 ? -1 : token_role(lm, tok);
        int node = 0, word = -1;
        double term = 0.0;
        int ctx[kLmMaxCtx];
        for (int q = 0; q < kLmMaxCtx; ++q) ctx[q] = p_ctx[k][q];
        if (tok < 0) {
          // a finished hypothesis carried over keeps its state
          node = p_node[k]; word = p_word[k]; term = p_term[k];
        } else if (role == kRoleWord && tok != eos) {
          // the word stays in the dictionary (the score kernel excluded the others); score the new current word once
          const LmView L = lm_view(lm.blob);
          const int2 ch = lm_trie_find(L, p_node[k], tok + 1);
          node = ch.x; word = ch.y;
          term = (double)lm.alpha * (double)lm_score(L, ctx, ch.y) + (double)lm.beta;
        } else if (role == kRoleSpace && tok != eos && p_node[k] != 0) {
          // a space completes a non-empty word: it joins the context (a transparent token drops the run instead)
          const int m = reinterpret_cast<const LmHeader*>(lm.blob)->order - 1;
          for (int q = 0; q < m; ++q) ctx[q] = q + 1 < m ? p_ctx[k][q + 1] : p_word[k];
        }
        lm.node[r] = node;
        lm.word[r] = word;
        lm.term[r] = term;
        for (int q = 0; q < kLmMaxCtx; ++q) lm.ctx[(int64_t)r * kLmMaxCtx + q] = ctx[q];
      }
      len[r] = nl;
      fin[r] = f;
      live[r] = 1;
      next_in[r] = tok >= 0 ? tok : bos;
      parent[r] = r0 + k;
      out_lens[r] = nl;
      out_scores[r] = (float)e_score[e];
      if (!f) atomicAnd(&all_fin, 0);
    } else {
      score[r] = -__builtin_inf();
      len[r] = 0;
      fin[r] = 1;
      live[r] = 0;
      next_in[r] = bos;
      parent[r] = r;
      out_lens[r] = 0;
      out_scores[r] = LR_NEG_INF;
    }
  }
  __syncthreads();
  if (tid == 0) {
    u[U_CUR] = cur ^ 1;
    const int rounds = u[U_ROUNDS] + 1;
    u[U_ROUNDS] = rounds;
    atomicMax(&ctr[1], rounds);
    if (all_fin) {
      u[U_DONE] = 1;
      atomicAdd(&ctr[0], 1);
    }
  }
}

// log(e^x + e^y) in float64; -inf only when both are
__device__ __forceinline__ double log_add(double x, double y) {
  const double m = x > y ? x : y, d = x > y ? y : x;
  if (m == -__builtin_inf()) return m;
  return m + log1p(exp(d - m));
}

// The joint search's list for one row: one wave per row (grid R, 64 threads).  A finished row lists itself at
// its place (c = 0); an unfinished row lists its P best tokens by lp, lane c holding candidate c.  Each lane
// then runs the CTC prefix recursion of its candidate over the utterance's frames (serial in t; the parent's
// arrays gam[r][t] are the same address for every lane of the row), writes its arrays to cand[r][t][c] (lanes of
// one t side by side) and its entry (token, s', a', c').  With ctc == 0 (lambda = 0) s' = a' and nothing of the
// CTC terms is computed.  A candidate whose c' is -inf (a structural zero) is dropped when lambda > 0.
// LM: word-character tokens that leave the dictionary are excluded from the scan (a row may then list fewer than P:
// the lanes past them write "no entry"), and each entry takes l' = l plus the row's cached term for a space or EOS.
template <bool LM>
__global__ __launch_bounds__(64) void joint_score_kernel(
    const float* __restrict__ lp, const double* __restrict__ score, const int32_t* __restrict__ len,
    const int32_t* __restrict__ fin, const int32_t* __restrict__ live, const int32_t* __restrict__ next_in,
    const int32_t* __restrict__ ustate, const float* __restrict__ y, int64_t stride_b, int64_t stride_t,
    const double* __restrict__ sa, const double* __restrict__ sc, const double2* __restrict__ gam,
    int32_t* __restrict__ ent_tok, double* __restrict__ ent_s, double* __restrict__ ent_a, double* __restrict__ ent_c,
    double2* __restrict__ cand, const int32_t* __restrict__ enc_lens, double lambda, int ctc, int K, int P, int V,
    int T, int blank, int bos, int eos, int pad, LmState lm) {
  const int r = blockIdx.x, b = r / K, lane = threadIdx.x;
  if (ustate[(int64_t)b * U_WORDS + U_DONE]) return;   // (uniform)
  const int64_t e0 = (int64_t)r * P;
  if (!live[r] || fin[r]) {
    if (lane < P) {
      const bool carry = live[r] && lane == 0;
      ent_tok[e0 + lane] = carry ? -1 : -2;
      if (carry) {
        ent_s[e0] = score[r];
        ent_a[e0] = sa[r];
        ent_c[e0] = sc[r];
        if constexpr (LM) lm.ent_l[e0] = lm.l[r];
      }
    }
    return;
  }
  int tok = LM ? -2 : 0;   // LM: a lane the scan does not reach holds no entry
  float l = 0.f;
  if constexpr (LM) {
    const LmView L = lm_view(lm.blob);
    const int node = lm.node[r];
    wave_topn(lp + (int64_t)r * V, lane, V, pad, bos, P, [&](int c, int v, float x) {
      if (lane == c) { tok = v; l = x; }
    }, [&](int v) { return v != eos && token_role(lm, v) == kRoleWord && lm_trie_find(L, node, v + 1).x < 0; });
  } else {
    wave_topn(lp + (int64_t)r * V, lane, V, pad, bos, P, [&](int c, int v, float x) {
      if (lane == c) { tok = v; l = x; }
    });
  }
  if (lane >= P) return;
  if constexpr (LM) {
    if (tok < 0) {
      ent_tok[e0 + lane] = -2;
      return;
    }
  }
  const double a = sa[r] + (double)l;
  double c = 0.0, s = a;
  if (ctc) {
    const double NEG = -__builtin_inf();
    const int Tb = utt_frames(enc_lens, b, T);
    const int k = tok + 1;                                    // decoder token v is class v + 1
    const int n0 = len[r];
    const int lastk = n0 > 0 ? next_in[r] + 1 : -1;           // last(g)'s class; none for the empty prefix
    const double2* g = gam + (int64_t)r * T;
    const float* yb = y + (int64_t)b * stride_b;
    double2* out = cand + (int64_t)r * T * P + lane;
    double gn = NEG, gb = NEG, psi = NEG;
    double phi = n0 == 0 ? 0.0 : NEG;                         // phi_{t-1}, from phi_{-1} = [g empty]
#pragma unroll 4
    for (int t = 0; t < Tb; ++t) {
      const float* yt = yb + (int64_t)t * stride_t;
      const double yk = (double)yt[k], y0 = (double)yt[blank];
      const double2 gp = g[t];
      const double x = phi + yk;
      const double gn1 = log_add(gn, phi) + yk;
      const double gb1 = log_add(gb, gn) + y0;
      psi = log_add(psi, x);
      gn = gn1;
      gb = gb1;
      out[(int64_t)t * P] = make_double2(gn, gb);
      phi = k == lastk ? gp.y : log_add(gp.y, gp.x);         // phi_t of g for class k
    }
    c = tok == eos ? log_add(gn, gb) : psi;
    s = lambda == 1.0 ? c : (1.0 - lambda) * a + lambda * c;
  }
  if constexpr (LM) {
    // a space or EOS completes the current word: its cached term (0 at the root) joins l
    const double l1 = lm.l[r] + (tok == eos || token_role(lm, tok) == kRoleSpace ? lm.term[r] : 0.0);
    s += l1;
    lm.ent_l[e0 + lane] = l1;
  }
  ent_tok[e0 + lane] = ctc && c == -__builtin_inf() ? -2 : tok;
  ent_s[e0 + lane] = s;
  ent_a[e0 + lane] = a;
  ent_c[e0 + lane] = c;
}

// the start rows' CTC arrays: gamma^n(empty) = -inf, gamma^b_t(empty) = sum_{tau <= t} y_tau^blank; a = c = 0
__global__ void joint_init_kernel(const float* __restrict__ y, int64_t stride_b, int64_t stride_t,
                                  const int32_t* __restrict__ enc_lens, double* sa, double* sc, double2* gam, int B,
                                  int K, int T, int blank, int ctc) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B * K) return;
  sa[r] = 0.0;
  sc[r] = 0.0;
  if (!ctc || r % K) return;
  const int b = r / K, Tb = utt_frames(enc_lens, b, T);
  double acc = 0.0;
  for (int t = 0; t < Tb; ++t) {
    acc += (double)y[(int64_t)b * stride_b + (int64_t)t * stride_t + blank];
    gam[(int64_t)r * T + t] = make_double2(-__builtin_inf(), acc);
  }
}

// the start rows' language-model state: l = 0, the trie's root, the context all <s>
__global__ void lm_init_kernel(LmState lm, int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int bos = reinterpret_cast<const LmHeader*>(lm.blob)->bos;
  lm.l[r] = 0.0;
  lm.node[r] = 0;
  lm.word[r] = -1;
  lm.term[r] = 0.0;
  for (int q = 0; q < kLmMaxCtx; ++q) lm.ctx[(int64_t)r * kLmMaxCtx + q] = bos;
}

struct StatePtrs {
  const float* y[MAXL];    // each layer's new h [R][Hd] (the step's output)
  const float* yc[MAXL];   // each layer's new c (LSTM) or NULL
  float* h[MAXL];          // each layer's state for the next round
  float* c[MAXL];
};

// next round's state of row r = the new state of its parent.  grid (R, NL)
__global__ void beam_reorder_kernel(StatePtrs q, const int32_t* __restrict__ parent,
                                    const int32_t* __restrict__ ustate, int K, int Hd) {
  const int r = blockIdx.x, k = blockIdx.y;
  if (ustate[(int64_t)(r / K) * U_WORDS + U_DONE]) return;
  const int64_t src = (int64_t)parent[r] * Hd, dst = (int64_t)r * Hd;
  for (int c = threadIdx.x; c < Hd / 4; c += blockDim.x) {
    reinterpret_cast<float4*>(q.h[k] + dst)[c] = reinterpret_cast<const float4*>(q.y[k] + src)[c];
    if (q.c[k]) reinterpret_cast<float4*>(q.c[k] + dst)[c] = reinterpret_cast<const float4*>(q.yc[k] + src)[c];
  }
}

#define LR_TRY(expr)                \
  do {                              \
    const int st__ = (expr);        \
    if (st__ != LR_OK) return st__; \
  } while (0)

}  // namespace

extern "C" size_t lr_decoder_beam_workspace_bytes(int mode, int attn_type, int num_layers, int B, int K, int Lmax,
                                                  int T, int Hd, int Cd, int V, int A) {
  if (!sizes_ok(mode, attn_type, num_layers, B, K, Lmax, T, Hd, Cd, V, A)) return 0;
  const Sizes z = {B, K, Lmax + 1, T, Hd, Cd, V, A, gates_of(mode), attn_type, num_layers, 0};
  return ws_layout(z).total * 4;
}

extern "C" size_t lr_decoder_joint_beam_workspace_bytes(int mode, int attn_type, int num_layers, int B, int K,
                                                        int Lmax, int T, int Hd, int Cd, int V, int A, int C,
                                                        int pre_beam) {
  if (!sizes_ok(mode, attn_type, num_layers, B, K, Lmax, T, Hd, Cd, V, A) || !joint_ok(K, T, V, C, pre_beam))
    return 0;
  const Sizes z = {B, K, Lmax + 1, T, Hd, Cd, V, A, gates_of(mode), attn_type, num_layers, pre_beam};
  return ws_layout(z).total * 4;
}

extern "C" size_t lr_decoder_lm_beam_workspace_bytes(int mode, int attn_type, int num_layers, int B, int K, int Lmax,
                                                     int T, int Hd, int Cd, int V, int A, int C, int pre_beam) {
  if (!sizes_ok(mode, attn_type, num_layers, B, K, Lmax, T, Hd, Cd, V, A) || !joint_ok(K, T, V, C, pre_beam) ||
      !lm_ok(V))
    return 0;
  const Sizes z = {B, K, Lmax + 1, T, Hd, Cd, V, A, gates_of(mode), attn_type, num_layers, pre_beam, 1};
  return ws_layout(z).total * 4;
}

namespace {

// The joint search's inputs beyond lr_decoder_beam_search's (NULL: the attention-only search).
struct JointArgs {
  const float* y;
  int64_t stride_b, stride_t;
  int C, blank, P;
  double lambda;
};

// The language model's inputs beyond the joint search's (NULL: no language model).
struct LmInputs {
  const uint8_t* blob;
  const int32_t* roles;
  float alpha, beta;
};

int beam_search_impl(int mode, int attn_type, const lr_decoder_params* p, const lr_decoder_upper* up,
                     const float* enc, const int32_t* enc_lens, const float* h0, const float* c0, int bos, int eos,
                     int pad, int beam_width, int max_label_len, int poll_every, int32_t* out_ids, int32_t* out_lens,
                     float* out_scores, int32_t* rounds_host, void* workspace, size_t workspace_bytes, int B, int T,
                     int Hd, int Cd, int V, int A, hipStream_t stream, const JointArgs* jt,
                     const LmInputs* lmi = nullptr) {
  const int NL = up ? up->num_layers : 1;
  const int K = beam_width, Lmax = max_label_len;
  if (!sizes_ok(mode, attn_type, NL, B, K, Lmax, T, Hd, Cd, V, A)) {
    // a well-formed request the kernels do not cover is UNSUPPORTED; nonsense is INVALID_ARG
    const bool sane = B > 0 && T > 0 && Hd > 0 && Cd > 0 && V > 0 && K > 0 && Lmax > 0 && NL >= 1;
    return sane ? LR_ERR_UNSUPPORTED : LR_ERR_INVALID_ARG;
  }
  LR_CHECK_ARG(p && enc && enc_lens && h0 && out_ids && out_lens && out_scores && workspace && poll_every >= 1);
  LR_CHECK_ARG(p->emb && p->w_ih && p->w_hh && p->b_ih && p->b_hh && p->w_o && p->b_o && p->out_mask);
  LR_CHECK_ARG(attn_type == ATT_NONE || (p->w_c && p->b_c));
  LR_CHECK_ARG(mode != LR_RNN_LSTM || c0);
  LR_CHECK_ARG(!up || !up->drop_mask);   // inference: no inter-layer dropout
  for (int k = 1; k < NL; ++k) LR_CHECK_ARG(up->w_ih[k - 1] && up->w_hh[k - 1] && up->b_ih[k - 1] && up->b_hh[k - 1]);
  LR_CHECK_ARG(bos >= 0 && bos < V && eos >= 0 && eos < V && pad >= 0 && pad < V && bos != pad && eos != bos &&
               eos != pad);
  if (attn_type == ATT_GENERAL || attn_type == ATT_1LNN) LR_CHECK_ARG(p->attn_w1 && p->attn_b1);
  if (attn_type == ATT_CONCAT) LR_CHECK_ARG(p->attn_w1 && p->attn_b1 && p->attn_w2 && p->attn_b2);
  const Sizes z = {B, K, Lmax + 1, T, Hd, Cd, V, A, gates_of(mode), attn_type, NL, jt ? jt->P : 0, lmi ? 1 : 0};
  const Ws w = ws_layout(z);
  if (workspace_bytes < w.total * 4) return LR_ERR_WORKSPACE;
  float* base = (float*)workspace;
  auto I = [&](size_t off) { return (int32_t*)(base + off); };
  const int G = z.G, GH = G * Hd, R = B * K, LH = Lmax + 1, Kc = K < V - 2 ? K : V - 2;
  const bool attn = attn_type != ATT_NONE;
  const size_t state = (size_t)B * Hd;
  const float* w_hh[MAXL];
  const float* w_ihu[MAXL];
  const float* b_hhl[MAXL];
  const float* b_ihl[MAXL];
  for (int k = 0; k < NL; ++k) {
    w_hh[k] = k == 0 ? p->w_hh : up->w_hh[k - 1];
    w_ihu[k] = k == 0 ? nullptr : up->w_ih[k - 1];
    b_ihl[k] = k == 0 ? p->b_ih : up->b_ih[k - 1];
    b_hhl[k] = k == 0 ? p->b_hh : up->b_hh[k - 1];
  }
  void* gws = base + w.gemm;
  float* top = base + w.y[NL - 1];   // the top layer's new states: what the attention and the head read
  float* logits = base + w.logits;
  float* wts = base + w.wts;
  float* ctx = base + w.ctx;
  float* pre = base + w.pre;
  float* ph = base + w.ph;
  float* lp = base + w.lp;
  int32_t* ctr = I(w.ctr);
  const int out_rows = head_rows(Hd, V);
  const size_t out_lds = (size_t)out_rows * (Hd + V) * sizeof(float);

  // ---- prologue: weights in the step kernels' forms, the start beam, the step-independent attention halves ----
  for (int k = 0; k < NL; ++k) {
    LR_TRY(lr_rnn_fold_bias(b_ihl[k], b_hhl[k], base + w.biasf[k], G, Hd, stream));
    LR_TRY(lr_rnn_pack_w(w_hh[k], base + w.wp[k], G, Hd, 0, stream));
    lr_clear_error();
    if (hipMemsetAsync(base + w.hp[k], 0, 2 * w.hp_slot * sizeof(float), stream) != hipSuccess) return LR_ERR_LAUNCH;
    LR_LAUNCH(beam_bcast_kernel, dim3(R), dim3(256), 0, stream, h0 + k * state, base + w.hcur[k], K, Hd);
    LR_TRY(lr_launch_status());
    if (G == 4) {
      LR_LAUNCH(beam_bcast_kernel, dim3(R), dim3(256), 0, stream, c0 + k * state, base + w.ccur[k], K, Hd);
      LR_TRY(lr_launch_status());
    }
  }
  LR_LAUNCH(beam_init_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, (double*)(base + w.score), I(w.len), I(w.fin),
            I(w.live), I(w.next_in), I(w.parent), I(w.ones), I(w.ustate), ctr, R, K, bos);
  LR_TRY(lr_launch_status());
  JointState js = {};
  const int ctc = jt && jt->lambda > 0.0;
  if (jt) {
    js = {I(w.ent_tok), (const double*)(base + w.ent_s), (const double*)(base + w.ent_a),
          (const double*)(base + w.ent_c), (double*)(base + w.sa), (double*)(base + w.sc), (double2*)(base + w.gam),
          (const double2*)(base + w.cand), enc_lens, T, jt->P, ctc};
    LR_LAUNCH(joint_init_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, jt->y, jt->stride_b, jt->stride_t,
              enc_lens, js.sa, js.sc, js.gam, B, K, T, jt->blank, ctc);
    LR_TRY(lr_launch_status());
  }
  LmState lms = {};
  if (lmi) {
    lms = {lmi->blob, lmi->roles, lmi->alpha, lmi->beta, jt->C, (double*)(base + w.lm_l), I(w.lm_node), I(w.lm_word),
           (double*)(base + w.lm_term), I(w.lm_ctx), (double*)(base + w.ent_l)};
    LR_LAUNCH(lm_init_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, lms, R);
    LR_TRY(lr_launch_status());
  }
  LR_TRY(lr_sgemm_impl(0, 1, V, GH, Cd, 1.f, p->emb, Cd, p->w_ih, Cd, 0.f, base + w.EW, GH, base + w.biasf[0], 0, 0,
                       gws, w.gemm_bytes, stream));
  const int BT = B * T;
  const float* src = nullptr;     // dot: enc; general: GE = enc W_g        [B][T][Hd]
  const float* cterm = nullptr;   // general: cE = enc . b_g; 1_layer_nn: se = enc . w_e   [B][T]
  if (attn_type == ATT_DOT) {
    src = enc;
  } else if (attn_type == ATT_GENERAL) {
    LR_TRY(lr_sgemm_impl(0, 0, BT, Hd, Hd, 1.f, enc, Hd, p->attn_w1, Hd, 0.f, base + w.aux1, Hd, nullptr, 0, 0, gws,
                         w.gemm_bytes, stream));
    LR_TRY(lr_sgemm_impl(0, 1, BT, 1, Hd, 1.f, enc, Hd, p->attn_b1, Hd, 0.f, base + w.aux2, 1, nullptr, 0, 0, nullptr,
                         0, stream));
    src = base + w.aux1;
    cterm = base + w.aux2;
  } else if (attn_type == ATT_1LNN) {
    LR_TRY(lr_sgemm_impl(0, 1, BT, 1, Hd, 1.f, enc, Hd, p->attn_w1, 2 * Hd, 0.f, base + w.aux2, 1, nullptr, 0, 0,
                         nullptr, 0, stream));
    cterm = base + w.aux2;
  } else if (attn_type == ATT_CONCAT) {
    LR_TRY(lr_sgemm_impl(0, 1, BT, A, Hd, 1.f, enc, Hd, p->attn_w1, 2 * Hd, 0.f, base + w.aux1, A, p->attn_b1, 0, 0,
                         gws, w.gemm_bytes, stream));
  }
  StatePtrs sp;
  for (int k = 0; k < MAXL; ++k) {
    const bool on = k < NL;
    sp.y[k] = on ? base + w.y[k] : nullptr;
    sp.yc[k] = on && G == 4 ? base + w.extra[k] : nullptr;
    sp.h[k] = on ? base + w.hcur[k] : nullptr;
    sp.c[k] = on && G == 4 ? base + w.ccur[k] : nullptr;
  }

  // ---- one round ----
  auto round = [&]() -> int {
    LR_LAUNCH(dec_gather_kernel, dim3(1, R), dim3(256), 0, stream, (const float*)(base + w.EW),
              (const int32_t*)I(w.next_in), (const int32_t*)I(w.next_in), I(w.ids_used), base + w.gates[0], 1, GH, V,
              0, 1);
    LR_TRY(lr_launch_status());
    for (int k = 0; k < NL; ++k) {
      if (k > 0)
        LR_TRY(lr_sgemm_impl(0, 1, R, GH, Hd, 1.f, base + w.y[k - 1], Hd, w_ihu[k], Hd, 0.f, base + w.gates[k], GH,
                             base + w.biasf[k], 0, 0, gws, w.gemm_bytes, stream));
      // step 0 of a one-step sequence from the rows' current state: the kernel reads the state's packed copy
      // from parity slot 1 and h0 / c0 = the unpacked state
      LR_TRY(lr_rnn_pack_state(base + w.hcur[k], base + w.hp[k] + w.hp_slot, R, Hd, stream));
      LR_TRY(lr_rnn_step_fwd(G, base + w.gates[k], base + w.extra[k], base + w.y[k], base + w.hp[k], I(w.ones),
                             base + w.wp[k], b_hhl[k], base + w.hcur[k], G == 4 ? base + w.ccur[k] : nullptr, R, 1,
                             Hd, 0, stream));
    }
    if (attn) {
      if (attn_type == ATT_DOT || attn_type == ATT_GENERAL) {
        // logits[b] (K x T) = top[b] (K x Hd) . src[b]^T
        LR_TRY(lr_sgemm_batched_impl(0, 1, K, T, Hd, 1.f, top, Hd, (int64_t)K * Hd, src, Hd, (int64_t)T * Hd, 0.f,
                                     logits, T, (int64_t)K * T, nullptr, B, stream));
      } else if (attn_type == ATT_CONCAT) {
        LR_TRY(lr_sgemm_impl(0, 1, R, A, Hd, 1.f, top, Hd, p->attn_w1 + Hd, 2 * Hd, 0.f, ph, A, nullptr, 0, 0, gws,
                             w.gemm_bytes, stream));   // ph = W1h h
        LR_LAUNCH(dec_concat_logits_kernel, dim3(K, B), dim3(256), (size_t)2 * A * sizeof(float), stream,
                  (const float*)(base + w.aux1), (const float*)ph, p->attn_w2, p->attn_b2, logits, K, T, A, 0);
        LR_TRY(lr_launch_status());
      }
      LR_LAUNCH(dec_attn_softmax_kernel, dim3(K, B), dim3(64), 0, stream, attn_type, (const float*)top, enc_lens,
                cterm, attn_type == ATT_1LNN ? p->attn_w1 + Hd : (const float*)nullptr,
                attn_type == ATT_1LNN ? p->attn_b1 : (const float*)nullptr, logits, wts, K, T, Hd, 0);
      LR_TRY(lr_launch_status());
      // ctx[b] (K x Hd) = wts[b] (K x T) . enc[b] (T x Hd)
      LR_TRY(lr_sgemm_batched_impl(0, 0, K, Hd, T, 1.f, wts, T, (int64_t)K * T, enc, Hd, (int64_t)T * Hd, 0.f, ctx,
                                   Hd, (int64_t)K * Hd, nullptr, B, stream));
      LR_TRY(lr_sgemm_impl(0, 1, R, Hd, Hd, 1.f, ctx, Hd, p->w_c, 2 * Hd, 0.f, pre, Hd, p->b_c, 0, 0, gws,
                           w.gemm_bytes, stream));
      LR_TRY(lr_sgemm_impl(0, 1, R, Hd, Hd, 1.f, top, Hd, p->w_c + Hd, 2 * Hd, 1.f, pre, Hd, nullptr, 0, 0, gws,
                           w.gemm_bytes, stream));
    }
    LR_LAUNCH(dec_out_fwd_kernel<false>, dim3((R + out_rows - 1) / out_rows), dim3(256), out_lds, stream,
              attn ? pre : top, p->w_o, p->b_o, p->out_mask, lp, (int32_t*)nullptr, 1, Hd, V, 0, 1, R, out_rows,
              attn ? 1 : 0, (uint64_t)0);
    LR_TRY(lr_launch_status());
    if (!jt) {
      LR_LAUNCH(beam_select_kernel<false>, dim3(B), dim3(SEL_THREADS), 0, stream, (const float*)lp,
                (double*)(base + w.score), I(w.len), I(w.fin), I(w.live), I(w.next_in), I(w.parent), I(w.hist),
                I(w.ustate), ctr, out_ids, out_lens, out_scores, K, Kc, V, LH, bos, eos, pad, js, lms);
    } else if (!lmi) {
      LR_LAUNCH(joint_score_kernel<false>, dim3(R), dim3(64), 0, stream, (const float*)lp,
                (const double*)(base + w.score), (const int32_t*)I(w.len), (const int32_t*)I(w.fin),
                (const int32_t*)I(w.live), (const int32_t*)I(w.next_in), (const int32_t*)I(w.ustate), jt->y,
                jt->stride_b, jt->stride_t,
                (const double*)js.sa, (const double*)js.sc, (const double2*)js.gam, I(w.ent_tok),
                (double*)(base + w.ent_s), (double*)(base + w.ent_a), (double*)(base + w.ent_c),
                (double2*)(base + w.cand), enc_lens, jt->lambda, ctc, K, jt->P, V, T, jt->blank, bos, eos, pad, lms);
      LR_TRY(lr_launch_status());
      LR_LAUNCH(beam_select_kernel<true>, dim3(B), dim3(SEL_THREADS), 0, stream, (const float*)lp,
                (double*)(base + w.score), I(w.len), I(w.fin), I(w.live), I(w.next_in), I(w.parent), I(w.hist),
                I(w.ustate), ctr, out_ids, out_lens, out_scores, K, jt->P, V, LH, bos, eos, pad, js, lms);
    } else {
      LR_LAUNCH(joint_score_kernel<true>, dim3(R), dim3(64), 0, stream, (const float*)lp,
                (const double*)(base + w.score), (const int32_t*)I(w.len), (const int32_t*)I(w.fin),
                (const int32_t*)I(w.live), (const int32_t*)I(w.next_in), (const int32_t*)I(w.ustate), jt->y,
                jt->stride_b, jt->stride_t, (const double*)js.sa, (const double*)js.sc, (const double2*)js.gam,
                I(w.ent_tok), (double*)(base + w.ent_s), (double*)(base + w.ent_a), (double*)(base + w.ent_c),
                (double2*)(base + w.cand), enc_lens, jt->lambda, ctc, K, jt->P, V, T, jt->blank, bos, eos, pad, lms);
      LR_TRY(lr_launch_status());
      LR_LAUNCH((beam_select_kernel<true, true>), dim3(B), dim3(SEL_THREADS), 0, stream, (const float*)lp,
                (double*)(base + w.score), I(w.len), I(w.fin), I(w.live), I(w.next_in), I(w.parent), I(w.hist),
                I(w.ustate), ctr, out_ids, out_lens, out_scores, K, jt->P, V, LH, bos, eos, pad, js, lms);
    }
    LR_TRY(lr_launch_status());
    LR_LAUNCH(beam_reorder_kernel, dim3(R, NL), dim3(256), 0, stream, sp, (const int32_t*)I(w.parent),
              (const int32_t*)I(w.ustate), K, Hd);
    return lr_launch_status();
  };

  int32_t host[2] = {0, 0};
  for (int rd = 1; rd <= LH; ++rd) {
    LR_TRY(round());
    if (rd % poll_every == 0 && rd < LH) {
      lr_clear_error();
      if (hipMemcpyAsync(host, ctr, sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
          hipStreamSynchronize(stream) != hipSuccess)
        return LR_ERR_LAUNCH;
      if (host[0] >= B) break;
    }
  }
  if (rounds_host) {
    lr_clear_error();
    if (hipMemcpyAsync(host, ctr, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return LR_ERR_LAUNCH;
    *rounds_host = host[1];
  }
  return LR_OK;
}

}  // namespace

extern "C" int lr_decoder_beam_search(int mode, int attn_type, const lr_decoder_params* p, const lr_decoder_upper* up,
                                      const float* enc, const int32_t* enc_lens, const float* h0, const float* c0,
                                      int bos, int eos, int pad, int beam_width, int max_label_len, int poll_every,
                                      int32_t* out_ids, int32_t* out_lens, float* out_scores, int32_t* rounds_host,
                                      void* workspace, size_t workspace_bytes, int B, int T, int Hd, int Cd, int V,
                                      int A, lr_stream_t stream) {
  return beam_search_impl(mode, attn_type, p, up, enc, enc_lens, h0, c0, bos, eos, pad, beam_width, max_label_len,
                          poll_every, out_ids, out_lens, out_scores, rounds_host, workspace, workspace_bytes, B, T, Hd,
                          Cd, V, A, (hipStream_t)stream, nullptr);
}

extern "C" int lr_decoder_joint_beam_search(int mode, int attn_type, const lr_decoder_params* p,
                                            const lr_decoder_upper* up, const float* enc, const int32_t* enc_lens,
                                            const float* h0, const float* c0, const float* ctc_lp, int64_t stride_b,
                                            int64_t stride_t, int C, int blank, double ctc_weight, int pre_beam,
                                            int bos, int eos, int pad, int beam_width, int max_label_len,
                                            int poll_every, int32_t* out_ids, int32_t* out_lens, float* out_scores,
                                            int32_t* rounds_host, void* workspace, size_t workspace_bytes, int B,
                                            int T, int Hd, int Cd, int V, int A, lr_stream_t stream) {
  const int NL = up ? up->num_layers : 1;
  if (sizes_ok(mode, attn_type, NL, B, beam_width, max_label_len, T, Hd, Cd, V, A)) {
    LR_CHECK_ARG(C == V + 1 && blank == 0);
    LR_CHECK_ARG(ctc_weight >= 0.0 && ctc_weight <= 1.0);   // false for NaN
    if (!joint_ok(beam_width, T, V, C, pre_beam)) return LR_ERR_UNSUPPORTED;
    LR_CHECK_ARG(ctc_lp && stride_b >= 0 && stride_t >= 0);
  }
  const JointArgs jt = {ctc_lp, stride_b, stride_t, C, blank, pre_beam, ctc_weight};
  return beam_search_impl(mode, attn_type, p, up, enc, enc_lens, h0, c0, bos, eos, pad, beam_width, max_label_len,
                          poll_every, out_ids, out_lens, out_scores, rounds_host, workspace, workspace_bytes, B, T, Hd,
                          Cd, V, A, (hipStream_t)stream, &jt);
}

extern "C" int lr_decoder_lm_beam_search(int mode, int attn_type, const lr_decoder_params* p,
                                         const lr_decoder_upper* up, const float* enc, const int32_t* enc_lens,
                                         const float* h0, const float* c0, const float* ctc_lp, int64_t stride_b,
                                         int64_t stride_t, int C, int blank, double ctc_weight, int pre_beam,
                                         const void* lm, const int32_t* class_roles, float alpha, float beta, int bos,
                                         int eos, int pad, int beam_width, int max_label_len, int poll_every,
                                         int32_t* out_ids, int32_t* out_lens, float* out_scores, int32_t* rounds_host,
                                         void* workspace, size_t workspace_bytes, int B, int T, int Hd, int Cd, int V,
                                         int A, lr_stream_t stream) {
  const int NL = up ? up->num_layers : 1;
  if (sizes_ok(mode, attn_type, NL, B, beam_width, max_label_len, T, Hd, Cd, V, A)) {
    LR_CHECK_ARG(C == V + 1 && blank == 0);
    LR_CHECK_ARG(ctc_weight >= 0.0 && ctc_weight <= 1.0);   // false for NaN
    LR_CHECK_ARG(isfinite(alpha) && isfinite(beta));
    if (!joint_ok(beam_width, T, V, C, pre_beam) || !lm_ok(V)) return LR_ERR_UNSUPPORTED;
    LR_CHECK_ARG(lm && class_roles);
    LR_CHECK_ARG((ctc_lp || ctc_weight == 0.0) && stride_b >= 0 && stride_t >= 0);   // no CTC term at weight 0
  }
  const JointArgs jt = {ctc_lp, stride_b, stride_t, C, blank, pre_beam, ctc_weight};
  const LmInputs lmi = {static_cast<const uint8_t*>(lm), class_roles, alpha, beta};
  return beam_search_impl(mode, attn_type, p, up, enc, enc_lens, h0, c0, bos, eos, pad, beam_width, max_label_len,
                          poll_every, out_ids, out_lens, out_scores, rounds_host, workspace, workspace_bytes, B, T, Hd,
                          Cd, V, A, (hipStream_t)stream, &jt, &lmi);
}
