// lr_attn_rescore.hip — attention rescoring of CTC N-best lists on gfx950: the second pass of
// two-pass decoding.  The CTC prefix beam search runs first (live, chunk by chunk if wanted); when the utterance
// ends its N best hypotheses are scored ONCE by the attention decoder, teacher-forced, and reordered by a weighted
// sum of the two scores (WeNet's "attention rescoring").  The reference has nothing of this: its analysis.py holds
// only the one-pass search.
//
// The rule (per utterance b: N first-pass hypotheses, slot n holding len_n CTC classes and a first-pass score f_n):
//   * f_n is fp32 -log P, as the CTC searches return it (language-model and hotword terms included if the search had
//     them).  A slot is EMPTY when len_n == 0 and f_n is +inf, as the CTC searches leave it, or when f_n is NaN.
//   * Class k is decoder token k - 1 (the layout of decoder.ctc_labels).  Ids past len_n are never read; len_n is
//     clamped to [0, W] to stay in bounds.
//   * Scored sequence q_n: the tokens up to and including the first EOS; if there is no EOS, all tokens followed by
//     one EOS.  So 1 <= |q_n| <= W + 1.  Tokens after the first EOS are not looked at.  A non-empty slot with
//     len_n == 0 is the empty transcript: q_n = [EOS].
//   * A slot is SCORABLE when it is not empty and every token of q_n lies in [0, V) and is neither PAD nor BOS (the
//     blank class, token -1, makes it unscorable).
//   * a_n = sum_i lp_i[q_n[i]]: the decoder starts from the encoder's final state for b, is fed BOS and then
//     q_n[0], q_n[1], ..., and attends over b's encoder states masked by enc_lens[b].  The arithmetic is that of one
//     CharDecodingStep step, the same launches as lr_decoder_forward and the beam search; the fp32 terms are summed
//     in float64 in step order, as the beam search sums them.
//   * s_n = (1 - lambda) a_n - lambda f_n + gamma |q_n|, lambda = ctc_weight in [0, 1], gamma = length_bonus (any
//     finite value), in float64, returned as fp32.  A term whose weight is exactly 0 is left out (lambda = 0 never
//     reads f_n, lambda = 1 never reads a_n), so at lambda = 1, gamma = 0 the score is -f_n exactly.  A scorable
//     slot whose s is NaN (a non-finite model) is ranked with the unscorable ones.
//   * Order: the scorable slots by s descending with a STABLE sort (ties keep first-pass order), then the
//     unscorable non-empty slots in first-pass order, then the empty slots in first-pass order.
//   * Outputs, ranked best first: out_order[b][r] the input slot at rank r, out_scores[b][r] its s, out_attn[b][r]
//     its a (both -inf for unscorable and empty slots).
//   * Consequence: at lambda = 1, gamma = 0 with every slot scorable and f ascending (the CTC searches' order), the
//     order is the identity and out_scores == -f exactly.
//
// Structure.  Rows R = B*N (row = b*N + n), steps L = W + 1, every shape static; a row's steps past |q| are masked
// (the step kernel writes zero states there and the head skips them), an unscorable or empty row has 0 live steps.
//   * rescore_prep_kernel, one thread per row: reads the row's ids through the caller's strides, finds |q|, the
//     row's class (scorable / unscorable / empty), and writes the row's input tokens [L] (BOS, q_0, ...), its
//     targets [L] and its step count.
//   * The step pieces of lr_decoder.hip (lr_decoder_dev.h), each layer over all steps: the EW-table gather by token;
//     per layer lr_rnn_step_fwd from the packed start state (the encoder's final state of b, broadcast to b's N
//     rows: B*N*Hd floats per layer, the only N-fold copy), upper layers' W_ih as one GEMM over all (row, step).
//     The one-launch recurrence is not used.
//   * The attention products are batched over batch = B with M = N*L: all (hypothesis, step) rows of an utterance
//     stand where the steps stand in training, so enc and the step-independent halves (GE, cE / se, PE) stay per
//     utterance and are never copied N times.  The concat GEMMs run over all R*L rows.
//   * rescore_head_kernel (new), the fused scoring head: OUT_ROWS (row, step) pairs per workgroup, so W_o is read
//     once per group as in dec_out_fwd_kernel; tanh, output_proj, then one wave per pair: the masked log-sum-exp
//     (lr_wave_max / lr_wave_sum) and the single term logit[target] - lse -> term[row][step].  [R][L][V]
//     log-probabilities are never written; a group with no live pair returns at once.
//   * rescore_rank_kernel (new), one workgroup per utterance: thread n sums row n's live terms in float64 (one
//     owner per sum: no atomics), forms s, and the N entries are sorted stably by rank counting in LDS, as
//     beam_select_kernel does; it writes out_order, out_scores, out_attn.
// No host synchronisation inside the call.
//
// Limits (LR_ERR_UNSUPPORTED, workspace query 0): 1 <= N <= 128, 1 <= W <= 1024, 3 <= V <= 1024, B*N <= 65535,
// B*N*(W+1) <= 65535*64 (the GEMMs' grid), B*N*(W+1) and B*T below 2^31 / max(G*Hd, T, V, A) (their int row
// offsets), Hd % 4 == 0, the head's LDS (Hd + V) * 4 <= 60 KB and, with concat attention, A > 0 and 2*A*4 <= 60 KB
// (as in lr_decoder_forward); every RNN mode, every attention type, 1 .. LR_DEC_MAX_LAYERS layers.  A ctc_weight outside [0, 1], a non-finite weight or bonus, a NULL required pointer, a negative id
// stride or drop_mask != NULL is LR_ERR_INVALID_ARG.
#include "lr_common.h"
#include "lr_decoder_dev.h"

namespace {

constexpr int RS_MAX_N = 128;
constexpr int RS_MAX_W = 1024;
constexpr int RS_MAX_V = 1024;
constexpr int MAXL = LR_DEC_MAX_LAYERS;

enum { CLS_SCORABLE = 0, CLS_UNSCORABLE = 1, CLS_EMPTY = 2 };

inline int gates_of(int mode) { return mode == LR_RNN_GRU ? 3 : (mode == LR_RNN_LSTM ? 4 : 1); }

struct Sizes {
  int B, N, L, T, Hd, Cd, V, A, G, type, NL;   // L = W + 1 steps
};

// ---- workspace layout, in 4-byte words --------------------------------------------------------------------------
struct Ws {
  size_t EW, biasf[MAXL], wp[MAXL], hp[MAXL], gates[MAXL], extra[MAXL], y[MAXL], h0[MAXL], c0[MAXL];
  size_t tokens, targets, ids_used, steps, cls, qlen, term;
  size_t logits, wts, ctx, pre, aux1, aux2, ph, gemm, total;
  size_t hp_slot, gemm_bytes;
};

Ws ws_layout(const Sizes& z) {
  Ws w;
  const size_t R = (size_t)z.B * z.N, RL = R * z.L, GH = (size_t)z.G * z.Hd, BT = (size_t)z.B * z.T;
  const bool attn = z.type != ATT_NONE;
  size_t o = 0;
  auto take = [&](size_t n) { size_t at = o; o += (n + 63) / 64 * 64; return at; };
  w.EW = take((size_t)z.V * GH);
  w.hp_slot = lr_rnn_packed_state_floats((int)R, z.Hd);
  for (int k = 0; k < MAXL; ++k)
    w.biasf[k] = w.wp[k] = w.hp[k] = w.gates[k] = w.extra[k] = w.y[k] = w.h0[k] = w.c0[k] = 0;
  for (int k = 0; k < z.NL; ++k) {
    w.biasf[k] = take(GH);
    w.wp[k] = take(lr_rnn_packed_w_floats(z.G, z.Hd));
    w.hp[k] = take(2 * w.hp_slot);
    w.gates[k] = take(RL * GH);
    w.extra[k] = take(RL * z.Hd);
    w.y[k] = take(RL * z.Hd);
    w.h0[k] = take(R * z.Hd);
    w.c0[k] = take(z.G == 4 ? R * z.Hd : 0);
  }
  w.tokens = take(RL);
  w.targets = take(RL);
  w.ids_used = take(RL);
  w.steps = take(R);
  w.cls = take(R);
  w.qlen = take(R);
  w.term = take(RL);
  w.logits = take(attn ? RL * z.T : 0);
  w.wts = take(attn ? RL * z.T : 0);
  w.ctx = take(attn ? RL * z.Hd : 0);
  w.pre = take(attn ? RL * z.Hd : 0);
  w.aux1 = take(z.type == ATT_GENERAL ? BT * z.Hd : (z.type == ATT_CONCAT ? BT * z.A : 0));   // GE | PE
  w.aux2 = take((z.type == ATT_GENERAL || z.type == ATT_1LNN) ? BT : 0);                       // cE | se
  w.ph = take(z.type == ATT_CONCAT ? RL * z.A : 0);
  const int a = z.A > 0 ? z.A : 1;
  const int dims[][3] = {{z.V, (int)GH, z.Cd}, {(int)BT, z.Hd, z.Hd}, {(int)BT, a, z.Hd}, {(int)RL, z.Hd, z.Hd},
                         {(int)RL, a, z.Hd}, {(int)RL, (int)GH, z.Hd}};
  w.gemm_bytes = 0;
  for (const auto& d : dims) {
    const size_t g = lr_sgemm_workspace_bytes(d[0], d[1], d[2]);
    if (g > w.gemm_bytes) w.gemm_bytes = g;
  }
  w.gemm = take((w.gemm_bytes + 3) / 4);
  w.total = o;
  return w;
}

// rows of the scoring head per workgroup (lr_decoder_forward's rule); 0 when even one row does not fit
int head_rows(int Hd, int V) {
  int rows = OUT_ROWS;
  while (rows > 1 && (size_t)rows * (Hd + V) * sizeof(float) > 60 * 1024) rows >>= 1;
  return (size_t)rows * (Hd + V) * sizeof(float) > 60 * 1024 ? 0 : rows;
}

bool sizes_ok(int mode, int type, int NL, int B, int N, int W, int T, int Hd, int Cd, int V, int A) {
  if (!((mode == LR_RNN_GRU || mode == LR_RNN_LSTM || mode == LR_RNN_TANH) && type >= ATT_NONE &&
        type <= ATT_CONCAT && NL >= 1 && NL <= MAXL && B > 0 && N >= 1 && N <= RS_MAX_N && (int64_t)B * N <= 65535 &&
        W >= 1 && W <= RS_MAX_W && T > 0 && Hd > 0 && Hd % 4 == 0 && Cd > 0 && V >= 3 && V <= RS_MAX_V &&
        (type != ATT_CONCAT || (A > 0 && (size_t)2 * A * 4 <= 60 * 1024)) && head_rows(Hd, V) > 0))
    return false;
  // the GEMMs address rows with int offsets: rows * leading dimension stays below 2^31
  int64_t ld = (int64_t)gates_of(mode) * Hd;
  if (T > ld) ld = T;
  if (V > ld) ld = V;
  if (A > ld) ld = A;
  const int64_t rows = (int64_t)B * N * (W + 1), bt = (int64_t)B * T;
  // ... and tile 64 rows per workgroup along grid.y
  return rows <= (int64_t)65535 * 64 && rows * ld < ((int64_t)1 << 31) && bt * ld < ((int64_t)1 << 31);
}

// dst[b*N + n][:] = src[b][:] for every n (the start state of every row of utterance b)
__global__ void rescore_bcast_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int Hd) {
  const int r = blockIdx.x, b = r / N;
  const float4* s = reinterpret_cast<const float4*>(src + (int64_t)b * Hd);
  float4* d = reinterpret_cast<float4*>(dst + (int64_t)r * Hd);
  for (int c = threadIdx.x; c < Hd / 4; c += blockDim.x) d[c] = s[c];
}

// One thread per row: the rule's q_n, its class, and the row's teacher-forced inputs and targets.
__global__ __launch_bounds__(256) void rescore_prep_kernel(
    const int32_t* __restrict__ hyp_ids, int64_t stride_b, int64_t stride_n, const int32_t* __restrict__ hyp_lens,
    const float* __restrict__ first, int32_t* __restrict__ tokens, int32_t* __restrict__ targets,
    int32_t* __restrict__ steps, int32_t* __restrict__ cls, int32_t* __restrict__ qlen, int R, int N, int W, int V,
    int bos, int eos, int pad) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int L = W + 1, b = r / N, n = r - b * N;
  const int32_t* ids = hyp_ids + (int64_t)b * stride_b + (int64_t)n * stride_n;
  int32_t* tk = tokens + (int64_t)r * L;
  int32_t* tg = targets + (int64_t)r * L;
  int len = hyp_lens[r];
  len = len < 0 ? 0 : (len > W ? W : len);
  const float f = first[r];
  const bool empty = (f != f) || (len == 0 && f == __builtin_inff());
  bool ok = !empty;
  int q = 0;
  if (!empty) {
    bool ended = false;
    for (int i = 0; i < len && !ended; ++i) {
      const int v = ids[i] - 1;   // class k is token k - 1
      ok = ok && v >= 0 && v < V && v != pad && v != bos;
      tg[q++] = v;
      ended = v == eos;
    }
    if (!ended) tg[q++] = eos;
  }
  const int live = ok ? q : 0;
  // inputs: BOS, then the targets shifted by one; dead steps read PAD (their states are masked, their terms skipped)
  for (int i = 0; i < L; ++i) tk[i] = i == 0 ? bos : (i < live ? tg[i - 1] : pad);
  for (int i = live; i < L; ++i) tg[i] = pad;
  steps[r] = live;
  qlen[r] = empty ? 0 : q;
  cls[r] = empty ? CLS_EMPTY : (ok ? CLS_SCORABLE : CLS_UNSCORABLE);
}

// The fused scoring head.  `nrows` (<= OUT_ROWS) consecutive (row, step) pairs per workgroup, pair p = row*L + step:
// x = tanh(pre) (has_attn) or the RNN state, logits = W_o x + b_o + log(mask + 1e-45) exactly as dec_out_fwd_kernel
// forms them, then one wave per live pair: lse over the V logits and term[p] = logit[target] - lse.  A pair is live
// when step < steps[row]; a workgroup without one returns at once and a pair that is not live costs no product.
// Nothing else is written.
__global__ __launch_bounds__(256) void rescore_head_kernel(const float* __restrict__ nh, const float* __restrict__ w_o,
                                                           const float* __restrict__ b_o,
                                                           const float* __restrict__ mask,
                                                           const int32_t* __restrict__ targets,
                                                           const int32_t* __restrict__ steps,
                                                           float* __restrict__ term, int L, int Hd, int V, int total,
                                                           int nrows, int has_attn) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* x = reinterpret_cast<float*>(smem_raw);   // [nrows][Hd]
  float* lg = x + (size_t)nrows * Hd;              // [nrows][V]
  __shared__ int live[OUT_ROWS];
  __shared__ int any_live;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = blockIdx.x * nrows;
  if (tid == 0) any_live = 0;
  __syncthreads();
  if (tid < nrows) {
    const int p = p0 + tid;
    const int on = p < total && (p % L) < steps[p / L];
    live[tid] = on;
    if (on) any_live = 1;   // (every writer stores the same value)
  }
  __syncthreads();
  if (!any_live) return;   // (uniform)
  const int H4 = Hd >> 2;
  for (int idx = tid; idx < nrows * H4; idx += 256) {
    const int r = idx / H4, k4 = idx - r * H4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live[r]) {
      v = *(reinterpret_cast<const float4*>(nh + (int64_t)(p0 + r) * Hd) + k4);
      if (has_attn) { v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w); }
    }
    *reinterpret_cast<float4*>(&x[(size_t)r * Hd + 4 * k4]) = v;
  }
  __syncthreads();
  // 4 lanes per output class, each a quarter of the k range in 16-byte pieces (dec_out_fwd_kernel's product); the
  // pairs of the group that are not live are left out of it
  const int q4 = tid & 3;
  unsigned on = 0;
#pragma unroll
  for (int r = 0; r < OUT_ROWS; ++r)
    if (r < nrows && live[r]) on |= 1u << r;
  for (int vc = 0; vc < V; vc += 64) {
    const int v = vc + (tid >> 2);
    float acc[OUT_ROWS];
#pragma unroll
    for (int r = 0; r < OUT_ROWS; ++r) acc[r] = 0.f;
    if (v < V) {
      const float* wrow = w_o + (int64_t)v * Hd;
      for (int k = q4 * 4; k < Hd; k += 16) {
        const float4 w4 = *reinterpret_cast<const float4*>(wrow + k);
#pragma unroll
        for (int r = 0; r < OUT_ROWS; ++r) {
          if ((on >> r) & 1u) {
            const float4 x4 = *reinterpret_cast<const float4*>(&x[(size_t)r * Hd + k]);
            acc[r] += w4.x * x4.x + w4.y * x4.y + w4.z * x4.z + w4.w * x4.w;
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < OUT_ROWS; ++r) {
      acc[r] += __shfl_xor(acc[r], 1, 64);
      acc[r] += __shfl_xor(acc[r], 2, 64);
    }
    if (q4 == 0 && v < V) {
      const float add = b_o[v] + logf(mask[v] + 1e-45f);
#pragma unroll
      for (int r = 0; r < OUT_ROWS; ++r)
        if ((on >> r) & 1u) lg[(size_t)r * V + v] = acc[r] + add;
    }
  }
  __syncthreads();
  for (int r = wave; r < nrows; r += 4) {
    if (!live[r]) continue;   // wave-uniform
    const float* l = lg + (size_t)r * V;
    float m = LR_NEG_INF;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, l[v]);
    m = lr_wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(l[v] - m);
    s = lr_wave_sum(s);
    const float lse = m + logf(s);
    if (lane == 0) {
      int tg = targets[p0 + r];
      tg = tg < 0 ? 0 : (tg >= V ? V - 1 : tg);   // a live pair's target is in range by the rule; clamped all the same
      term[p0 + r] = l[tg] - lse;
    }
  }
}

template <typename S>
__device__ __forceinline__ bool ranks_before(S sa, int ia, S sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// One workgroup per utterance (RS_MAX_N threads, thread n owns slot n): a in float64 from the row's live terms in
// step order, s by the rule, then the stable sort by rank counting in LDS: scorable by (s desc, slot asc), then
// unscorable by slot, then empty by slot.  Every rank is taken exactly once.
__global__ __launch_bounds__(RS_MAX_N) void rescore_rank_kernel(const float* __restrict__ term,
                                                                const int32_t* __restrict__ steps,
                                                                const int32_t* __restrict__ cls,
                                                                const int32_t* __restrict__ qlen,
                                                                const float* __restrict__ first, double lambda,
                                                                double gamma, int32_t* __restrict__ out_order,
                                                                float* __restrict__ out_scores,
                                                                float* __restrict__ out_attn, int N, int L) {
  __shared__ double e_s[RS_MAX_N];
  __shared__ int e_cls[RS_MAX_N];
  const int b = blockIdx.x, n = threadIdx.x;
  const int r = b * N + n;
  double a = -__builtin_inf(), s = -__builtin_inf();
  int c = CLS_EMPTY;
  if (n < N) {
    c = cls[r];
    if (c == CLS_SCORABLE) {
      const float* t = term + (int64_t)r * L;
      const int q = steps[r];
      a = 0.0;
      for (int i = 0; i < q; ++i) a += (double)t[i];
      s = gamma * (double)qlen[r];
      if (lambda != 1.0) s += (1.0 - lambda) * a;
      if (lambda != 0.0) s -= lambda * (double)first[r];
      if (s != s) c = CLS_UNSCORABLE;
    }
    if (c != CLS_SCORABLE) a = s = -__builtin_inf();
    e_s[n] = s;
    e_cls[n] = c;
  }
  __syncthreads();
  if (n >= N) return;
  int rank = 0;
  for (int f = 0; f < N; ++f) {
    const int cf = e_cls[f];
    if (cf < c || (cf == c && (c == CLS_SCORABLE ? ranks_before(e_s[f], f, s, n) : f < n))) ++rank;
  }
  const int64_t o = (int64_t)b * N + rank;
  out_order[o] = n;
  out_scores[o] = (float)s;
  out_attn[o] = (float)a;
}

#define LR_TRY(expr)                \
  do {                              \
    const int st__ = (expr);        \
    if (st__ != LR_OK) return st__; \
  } while (0)

}  // namespace

extern "C" size_t lr_decoder_rescore_workspace_bytes(int mode, int attn_type, int num_layers, int B, int N, int W,
                                                     int T, int Hd, int Cd, int V, int A) {
  if (!sizes_ok(mode, attn_type, num_layers, B, N, W, T, Hd, Cd, V, A)) return 0;
  const Sizes z = {B, N, W + 1, T, Hd, Cd, V, A, gates_of(mode), attn_type, num_layers};
  return ws_layout(z).total * 4;
}

extern "C" int lr_decoder_rescore(int mode, int attn_type, const lr_decoder_params* p, const lr_decoder_upper* up,
                                  const float* enc, const int32_t* enc_lens, const float* h0, const float* c0,
                                  const int32_t* hyp_ids, int64_t hyp_stride_b, int64_t hyp_stride_n,
                                  const int32_t* hyp_lens, const float* first_scores, int bos, int eos, int pad,
                                  double ctc_weight, double length_bonus, int32_t* out_order, float* out_scores,
                                  float* out_attn, void* workspace, size_t workspace_bytes, int B, int N, int W, int T,
                                  int Hd, int Cd, int V, int A, lr_stream_t stream_) {
  const int NL = up ? up->num_layers : 1;
  if (!sizes_ok(mode, attn_type, NL, B, N, W, T, Hd, Cd, V, A)) {
    // a well-formed request the kernels do not cover is UNSUPPORTED; nonsense is INVALID_ARG
    const bool sane = B > 0 && T > 0 && Hd > 0 && Cd > 0 && V > 0 && N > 0 && W > 0 && NL >= 1;
    return sane ? LR_ERR_UNSUPPORTED : LR_ERR_INVALID_ARG;
  }
  LR_CHECK_ARG(ctc_weight >= 0.0 && ctc_weight <= 1.0);   // false for NaN
  LR_CHECK_ARG(length_bonus - length_bonus == 0.0);        // finite
  LR_CHECK_ARG(p && enc && enc_lens && h0 && hyp_ids && hyp_lens && first_scores && out_order && out_scores &&
               out_attn && workspace);
  LR_CHECK_ARG(hyp_stride_b >= 0 && hyp_stride_n >= 0);
  LR_CHECK_ARG(p->emb && p->w_ih && p->w_hh && p->b_ih && p->b_hh && p->w_o && p->b_o && p->out_mask);
  LR_CHECK_ARG(attn_type == ATT_NONE || (p->w_c && p->b_c));
  LR_CHECK_ARG(mode != LR_RNN_LSTM || c0);
  LR_CHECK_ARG(!up || !up->drop_mask);   // inference: no inter-layer dropout
  for (int k = 1; k < NL; ++k) LR_CHECK_ARG(up->w_ih[k - 1] && up->w_hh[k - 1] && up->b_ih[k - 1] && up->b_hh[k - 1]);
  LR_CHECK_ARG(bos >= 0 && bos < V && eos >= 0 && eos < V && pad >= 0 && pad < V && bos != pad && eos != bos &&
               eos != pad);
  if (attn_type == ATT_GENERAL || attn_type == ATT_1LNN) LR_CHECK_ARG(p->attn_w1 && p->attn_b1);
  if (attn_type == ATT_CONCAT) LR_CHECK_ARG(p->attn_w1 && p->attn_b1 && p->attn_w2 && p->attn_b2);
  const Sizes z = {B, N, W + 1, T, Hd, Cd, V, A, gates_of(mode), attn_type, NL};
  const Ws w = ws_layout(z);
  if (workspace_bytes < w.total * 4) return LR_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* base = (float*)workspace;
  auto I = [&](size_t off) { return (int32_t*)(base + off); };
  const int G = z.G, GH = G * Hd, R = B * N, L = W + 1, RL = R * L, NLs = N * L, BT = B * T;
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
  float* hs = base + w.y[NL - 1];   // the top layer's states [R][L][Hd]: what the attention and the head read
  float* logits = base + w.logits;
  float* wts = base + w.wts;
  float* ctx = base + w.ctx;
  float* pre = base + w.pre;
  float* ph = base + w.ph;
  const int32_t* steps = I(w.steps);
  const int out_rows = head_rows(Hd, V);
  const size_t out_lds = (size_t)out_rows * (Hd + V) * sizeof(float);

  // ---- the rows: q_n, class, inputs and targets ----
  LR_LAUNCH(rescore_prep_kernel, dim3((R + 255) / 256), dim3(256), 0, stream, hyp_ids, hyp_stride_b, hyp_stride_n,
            hyp_lens, first_scores, I(w.tokens), I(w.targets), I(w.steps), I(w.cls), I(w.qlen), R, N, W, V, bos, eos,
            pad);
  LR_TRY(lr_launch_status());

  // ---- weights in the step kernels' forms, the start state of every row, the step-independent attention halves ----
  for (int k = 0; k < NL; ++k) {
    LR_TRY(lr_rnn_fold_bias(b_ihl[k], b_hhl[k], base + w.biasf[k], G, Hd, stream));
    LR_TRY(lr_rnn_pack_w(w_hh[k], base + w.wp[k], G, Hd, 0, stream));
    lr_clear_error();
    if (hipMemsetAsync(base + w.hp[k], 0, 2 * w.hp_slot * sizeof(float), stream) != hipSuccess) return LR_ERR_LAUNCH;
    LR_LAUNCH(rescore_bcast_kernel, dim3(R), dim3(256), 0, stream, h0 + k * state, base + w.h0[k], N, Hd);
    LR_TRY(lr_launch_status());
    if (G == 4) {
      LR_LAUNCH(rescore_bcast_kernel, dim3(R), dim3(256), 0, stream, c0 + k * state, base + w.c0[k], N, Hd);
      LR_TRY(lr_launch_status());
    }
    // step 0 reads parity (0+1)&1 = 1
    LR_TRY(lr_rnn_pack_state(base + w.h0[k], base + w.hp[k] + w.hp_slot, R, Hd, stream));
  }
  LR_TRY(lr_sgemm_impl(0, 1, V, GH, Cd, 1.f, p->emb, Cd, p->w_ih, Cd, 0.f, base + w.EW, GH, base + w.biasf[0], 0, 0,
                       gws, w.gemm_bytes, stream));
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

  // ---- the recurrence, layer by layer over all steps (the tokens are all known) ----
  LR_LAUNCH(dec_gather_kernel, dim3(L, R), dim3(256), 0, stream, (const float*)(base + w.EW),
            (const int32_t*)I(w.tokens), (const int32_t*)I(w.tokens), I(w.ids_used), base + w.gates[0], L, GH, V, 0, 1);
  LR_TRY(lr_launch_status());
  for (int k = 0; k < NL; ++k) {
    if (k > 0)
      LR_TRY(lr_sgemm_impl(0, 1, RL, GH, Hd, 1.f, base + w.y[k - 1], Hd, w_ihu[k], Hd, 0.f, base + w.gates[k], GH,
                           base + w.biasf[k], 0, 0, gws, w.gemm_bytes, stream));
    for (int s = 0; s < L; ++s)
      LR_TRY(lr_rnn_step_fwd(G, base + w.gates[k], base + w.extra[k], base + w.y[k], base + w.hp[k], steps,
                             base + w.wp[k], b_hhl[k], base + w.h0[k], G == 4 ? base + w.c0[k] : nullptr, R, L, Hd, s,
                             stream));
  }

  // ---- attention and concat_layer over all (row, step) pairs: batch = B utterances, M = N*L pairs each ----
  if (attn) {
    if (attn_type == ATT_DOT || attn_type == ATT_GENERAL) {
      // logits[b] (N*L x T) = hs[b] (N*L x Hd) . src[b]^T
      LR_TRY(lr_sgemm_batched_impl(0, 1, NLs, T, Hd, 1.f, hs, Hd, (int64_t)NLs * Hd, src, Hd, (int64_t)T * Hd, 0.f,
                                   logits, T, (int64_t)NLs * T, nullptr, B, stream));
    } else if (attn_type == ATT_CONCAT) {
      LR_TRY(lr_sgemm_impl(0, 1, RL, A, Hd, 1.f, hs, Hd, p->attn_w1 + Hd, 2 * Hd, 0.f, ph, A, nullptr, 0, 0, gws,
                           w.gemm_bytes, stream));   // ph = W1h h
      LR_LAUNCH(dec_concat_logits_kernel, dim3(NLs, B), dim3(256), (size_t)2 * A * sizeof(float), stream,
                (const float*)(base + w.aux1), (const float*)ph, p->attn_w2, p->attn_b2, logits, NLs, T, A, 0);
      LR_TRY(lr_launch_status());
    }
    LR_LAUNCH(dec_attn_softmax_kernel, dim3(NLs, B), dim3(64), 0, stream, attn_type, (const float*)hs, enc_lens,
              cterm, attn_type == ATT_1LNN ? p->attn_w1 + Hd : (const float*)nullptr,
              attn_type == ATT_1LNN ? p->attn_b1 : (const float*)nullptr, logits, wts, NLs, T, Hd, 0);
    LR_TRY(lr_launch_status());
    // ctx[b] (N*L x Hd) = wts[b] (N*L x T) . enc[b] (T x Hd)
    LR_TRY(lr_sgemm_batched_impl(0, 0, NLs, Hd, T, 1.f, wts, T, (int64_t)NLs * T, enc, Hd, (int64_t)T * Hd, 0.f, ctx,
                                 Hd, (int64_t)NLs * Hd, nullptr, B, stream));
    LR_TRY(lr_sgemm_impl(0, 1, RL, Hd, Hd, 1.f, ctx, Hd, p->w_c, 2 * Hd, 0.f, pre, Hd, p->b_c, 0, 0, gws,
                         w.gemm_bytes, stream));
    LR_TRY(lr_sgemm_impl(0, 1, RL, Hd, Hd, 1.f, hs, Hd, p->w_c + Hd, 2 * Hd, 1.f, pre, Hd, nullptr, 0, 0, gws,
                         w.gemm_bytes, stream));
  }

  // ---- the scoring head and the ranking ----
  LR_LAUNCH(rescore_head_kernel, dim3((RL + out_rows - 1) / out_rows), dim3(256), out_lds, stream,
            (const float*)(attn ? pre : hs), p->w_o, p->b_o, p->out_mask, (const int32_t*)I(w.targets), steps,
            base + w.term, L, Hd, V, RL, out_rows, attn ? 1 : 0);
  LR_TRY(lr_launch_status());
  LR_LAUNCH(rescore_rank_kernel, dim3(B), dim3(RS_MAX_N), 0, stream, (const float*)(base + w.term), steps,
            (const int32_t*)I(w.cls), (const int32_t*)I(w.qlen), first_scores, ctc_weight, length_bonus, out_order,
            out_scores, out_attn, N, L);
  return lr_launch_status();
}
