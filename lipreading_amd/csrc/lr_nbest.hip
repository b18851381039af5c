// lr_nbest.hip — N-best minimum error rate training of the CTC head (BUILD-DEFINED: the reference has no such
// objective; the specification is in include/lipreading_hip.h, DESIGN.md §25, the yardstick tests/mwer_cases.py).
//
// Per utterance b, N hypothesis slots over ONE block of log-probabilities: the full-sum CTC lattice of every slot, a
// softmax across the slots' likelihoods, the expected risk, and one gradient that is the risk-weighted sum of the N
// occupancies.
//
//   lr_ctc_nbest_risk       nbest_lattice_kernel  one workgroup per (utterance, slot): B * N workgroups.  The first
//                                                 half of the workgroup walks alpha forwards, the second half walks
//                                                 beta backwards AT THE SAME TIME (the two recursions do not depend
//                                                 on each other), one thread per state, one LDS barrier per frame.
//                                                 Both tables go to the workspace.
//                           nbest_reduce_kernel   one workgroup: per utterance the softmax over its used slots in
//                                                 slot order, the expected risk, then the loss by a fixed tree.
//   lr_ctc_nbest_risk_grad  nbest_grad_kernel     one workgroup per (utterance, frame): no recursion is left, every
//                                                 frame's row is independent.  Per slot in slot order: one thread per
//                                                 state puts exp(alpha + beta - lp - ll) into LDS, then one thread
//                                                 per CLASS adds its states' terms in ascending state order.
//
// Arithmetic: the lattices, the softmax and the occupancy sums are fp64 in log space (libm's exp / log); inputs and
// outputs are fp32.  Every sum has a fixed order and there is no atomic, so two launches give the same bits.
#include "lr_common.h"

namespace {

constexpr int kMaxSlots = LR_NBEST_MAX_SLOTS;
constexpr int kMaxClasses = LR_NBEST_MAX_CLASSES;
constexpr int kMaxLen = LR_NBEST_MAX_HYP_LEN;
constexpr int kMaxStates = 2 * kMaxLen + 1;
constexpr int kHalfMax = 512;        // threads per recursion at the most: a thread then owns states s and s + 512
constexpr int kReduceThreads = 256;
constexpr int kGradThreads = 256;    // >= kMaxClasses: one thread per class in the class phase

#define LR_NEG_INF_D (-__builtin_inf())

struct NbestPlan {
  int half;             // threads of one recursion: the states rounded up to whole waves, kHalfMax at the most
  int sstride;          // doubles between two frames' rows of a table
  size_t off_coef, off_alpha, off_beta, bytes;   // ll at offset 0
};

int nbest_plan(int B, int T, int C, int N, int max_hyp_len, NbestPlan* p) {
  if (B < 1 || T < 1 || C < 1 || C > kMaxClasses || N < 1 || N > kMaxSlots || max_hyp_len < 0 || max_hyp_len > kMaxLen)
    return LR_ERR_UNSUPPORTED;
  if ((int64_t)B * T > 0x7fffffff || (int64_t)B * N > 0x7fffffff) return LR_ERR_UNSUPPORTED;   // one workgroup each
  const int S = 2 * max_hyp_len + 1;
  p->half = (int)lr_align_up((size_t)S, LR_WAVE);
  if (p->half > kHalfMax) p->half = kHalfMax;
  p->sstride = (int)lr_align_up((size_t)S, 8);
  const size_t slots = (size_t)B * N;
  const size_t table = slots * (size_t)T * p->sstride * sizeof(double);
  p->off_coef = slots * sizeof(double);
  p->off_alpha = lr_align_up(2 * slots * sizeof(double), 256);
  p->off_beta = p->off_alpha + table;
  p->bytes = p->off_beta + table;
  return LR_OK;
}

struct NbestArgs {
  const float* lp;
  const int32_t* sizes;
  const int32_t* hyps;
  const int32_t* hyp_lens;
  const float* risk;
  float* hyp_ll;
  float* post;
  int32_t* hyp_status;
  float* utt_risk;
  float* out_loss;
  int32_t* out_status;
  float* grad_weight;
  const float* grad_scale;
  float* grad;
  double* ll;      // [B][N] workspace
  double* coef;    // [B][N] workspace: post * (risk - utt_risk), 0 for unused slots
  double* alpha;   // [B][N][T][sstride] workspace
  double* beta;
  int64_t stride_b, stride_t, hyp_stride_b, hyp_stride_n, lens_stride_b;
  int B, T, C, N, max_hyp_len, blank, reduction, sstride;
};

__device__ __forceinline__ double lse3d(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  if (m == LR_NEG_INF_D) return LR_NEG_INF_D;
  return log(exp(a - m) + exp(b - m) + exp(c - m)) + m;
}

__device__ __forceinline__ int frames_of(const NbestArgs& a, int b) {
  // sizes outside [0, T] are clamped: no frame outside the block is ever addressed
  const int n = a.sizes ? a.sizes[b] : a.T;
  return n < 0 ? 0 : (n > a.T ? a.T : n);
}

// ---- forward: alpha and beta of one (utterance, slot) ----------------------------------------------------------------
__global__ __launch_bounds__(2 * kHalfMax) void nbest_lattice_kernel(const NbestArgs a) {
  __shared__ int32_t y[kMaxLen];
  __shared__ double row[2][2][kMaxStates + 3];   // [recursion][frame parity][1 + state]: a -inf cell in front and two behind
  const int slot = blockIdx.x;                   // b * N + n
  const int b = slot / a.N, n = slot % a.N;
  const int tid = threadIdx.x, nthreads = blockDim.x, half = nthreads >> 1;
  const int len = a.hyp_lens[(int64_t)b * a.lens_stride_b + n];
  const float r = a.risk[slot];
  const int32_t* ids = a.hyps + (int64_t)b * a.hyp_stride_b + (int64_t)n * a.hyp_stride_n;
  const int frames = frames_of(a, b);

  // the slot's status, decided by the whole workgroup from uniform values (every thread takes the same branch)
  int status = 0;
  if (len < 0) {
    status = LR_NBEST_EMPTY;
  } else if (len > a.max_hyp_len || !isfinite(r)) {
    status = LR_NBEST_REJECTED;
  } else {
    int bad = 0;
    for (int i = tid; i < len; i += nthreads) {
      const int32_t c = ids[i];
      bad |= (c < 0 || c >= a.C || c == a.blank);
      y[i] = c;
    }
    if (__syncthreads_or(bad)) status = LR_NBEST_REJECTED;     // (the barrier also publishes y)
  }
  if (status == 0) {
    // adjacent equal ids each need a blank frame between them
    int rep = 0;
    for (int i0 = 0; i0 < len; i0 += nthreads) {
      const int i = i0 + tid;
      rep += __syncthreads_count(i >= 1 && i < len && y[i] == y[i - 1]);
    }
    if (frames == 0 || frames < len + rep) status = LR_NBEST_INFEASIBLE;
  }
  if (status != 0) {
    if (tid == 0) {
      a.hyp_status[slot] = status;
      a.hyp_ll[slot] = LR_NEG_INF;
      a.ll[slot] = LR_NEG_INF_D;
    }
    return;
  }

  const int S = 2 * len + 1;
  const int dir = tid >= half;            // 0: alpha, 1: beta (whole waves: half is a multiple of 64)
  const int lt = tid - dir * half;
  const float* lpb = a.lp + (int64_t)b * a.stride_b;
  double* table = (dir ? a.beta : a.alpha) + (int64_t)slot * a.T * a.sstride;
  double (*buf)[kMaxStates + 3] = row[dir];

  // what a thread needs to know about its (at most two) states
  int cls[2];
  bool skip[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int s = lt + k * half;
    cls[k] = a.blank;
    skip[k] = false;
    if (s < S && (s & 1)) {
      const int i = (s - 1) >> 1;
      cls[k] = y[i];
      // alpha comes from s - 2, beta goes to s + 2: allowed between two DIFFERENT characters
      if (!dir) skip[k] = i >= 1 && y[i] != y[i - 1];
      else skip[k] = i + 1 < len && y[i] != y[i + 1];
    }
  }
  for (int i = tid; i < 2 * 2 * (kMaxStates + 3); i += nthreads) (&row[0][0][0])[i] = LR_NEG_INF_D;
  __syncthreads();

  const int t_first = dir ? frames - 1 : 0, step = dir ? -1 : 1;
  float e[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) e[k] = lt + k * half < S ? lpb[(int64_t)t_first * a.stride_t + cls[k]] : 0.f;
  for (int it = 0; it < frames; ++it) {
    const int t = t_first + it * step;
    const double* prev = buf[(it & 1) ^ 1] + 1;
    double* cur = buf[it & 1] + 1;
    float e_next[2] = {0.f, 0.f};
    if (it + 1 < frames) {   // the next frame's emissions, in flight while this frame's cells are computed
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (lt + k * half < S) e_next[k] = lpb[(int64_t)(t + step) * a.stride_t + cls[k]];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int s = lt + k * half;
      if (s >= S) continue;
      double v;
      if (it == 0) {
        const bool start = dir ? (s >= S - 2) : (s <= 1);
        v = start ? (double)e[k] : LR_NEG_INF_D;
      } else {
        const double n1 = prev[s - step];                                  // alpha: s - 1, beta: s + 1
        const double n2 = skip[k] ? prev[s - 2 * step] : LR_NEG_INF_D;
        const double m = lse3d(prev[s], n1, n2);
        v = m == LR_NEG_INF_D ? m : m + (double)e[k];
      }
      cur[s] = v;
      table[(int64_t)t * a.sstride + s] = v;
    }
    e[0] = e_next[0];
    e[1] = e_next[1];
    lr_lds_barrier();
  }
  if (tid == 0) {
    const double* last = row[0][(frames - 1) & 1] + 1;
    const double m = fmax(last[S - 1], last[S - 2]);   // (S == 1: last[-1] is the -inf cell in front)
    const double ll = m == LR_NEG_INF_D ? m : m + log(exp(last[S - 1] - m) + exp(last[S - 2] - m));
    a.ll[slot] = ll;
    a.hyp_ll[slot] = (float)ll;
    // -inf log-probabilities can empty a lattice that the frame count allows: infeasible all the same
    a.hyp_status[slot] = ll == LR_NEG_INF_D ? LR_NBEST_INFEASIBLE : LR_NBEST_USED;
  }
}

// ---- forward: softmax over the slots, expected risk, loss -----------------------------------------------------------
__global__ __launch_bounds__(kReduceThreads) void nbest_reduce_kernel(const NbestArgs a) {
  __shared__ double part[kReduceThreads];
  __shared__ int used_part[kReduceThreads];
  const int tid = threadIdx.x;
  double sum = 0.0;
  int used = 0;
  for (int b = tid; b < a.B; b += kReduceThreads) {
    const int o = b * a.N;
    double m = LR_NEG_INF_D;
    int any = 0;
    for (int n = 0; n < a.N; ++n)
      if (a.hyp_status[o + n] == 0) {
        m = fmax(m, a.ll[o + n]);
        any = 1;
      }
    double z = 0.0, R = 0.0;
    for (int n = 0; n < a.N; ++n)
      if (a.hyp_status[o + n] == 0) z += exp(a.ll[o + n] - m);
    for (int n = 0; n < a.N; ++n)
      if (a.hyp_status[o + n] == 0) R += exp(a.ll[o + n] - m) / z * (double)a.risk[o + n];
    for (int n = 0; n < a.N; ++n) {
      const bool ok = a.hyp_status[o + n] == 0;
      const double p = ok ? exp(a.ll[o + n] - m) / z : 0.0;
      a.post[o + n] = (float)p;
      a.coef[o + n] = ok ? p * ((double)a.risk[o + n] - R) : 0.0;
    }
    a.utt_risk[b] = any ? (float)R : 0.f;
    if (any) sum += R;
    used += any;
  }
  part[tid] = sum;
  used_part[tid] = used;
  __syncthreads();
  for (int w = kReduceThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      part[tid] += part[tid + w];
      used_part[tid] += used_part[tid + w];
    }
    __syncthreads();
  }
  const int U = used_part[0];
  const double w = a.reduction == LR_CTC_MEAN ? 1.0 / (double)(U > 0 ? U : 1) : 1.0;
  if (tid == 0) {
    a.out_loss[0] = U > 0 ? (float)(part[0] * w) : 0.f;
    a.out_status[0] = U > 0 ? 0 : 1;
  }
  for (int b = tid; b < a.B; b += kReduceThreads) {
    int any = 0;
    for (int n = 0; n < a.N; ++n) any |= a.hyp_status[b * a.N + n] == 0;
    a.grad_weight[b] = any ? (float)w : 0.f;
  }
}

// ---- backward: one (utterance, frame) row of the gradient ------------------------------------------------------------
__global__ __launch_bounds__(kGradThreads) void nbest_grad_kernel(const NbestArgs a) {
  __shared__ int32_t y[kMaxLen];
  __shared__ double v[kMaxStates];
  const int b = blockIdx.x / a.T, t = blockIdx.x % a.T;
  const int tid = threadIdx.x;
  float* out = a.grad + (int64_t)b * a.stride_b + (int64_t)t * a.stride_t;
  const float gw = a.grad_weight[b];
  if (t >= frames_of(a, b) || gw == 0.f) {
    if (tid < a.C) out[tid] = 0.f;
    return;
  }
  const float* lpr = a.lp + (int64_t)b * a.stride_b + (int64_t)t * a.stride_t;
  const double scale = (double)(a.grad_scale ? a.grad_scale[0] : 1.f) * (double)gw;
  double acc = 0.0;
  for (int n = 0; n < a.N; ++n) {
    const int slot = b * a.N + n;
    if (a.hyp_status[slot] != 0) continue;     // (uniform)
    const double coef = a.coef[slot];
    const int len = a.hyp_lens[(int64_t)b * a.lens_stride_b + n];
    if (len < 0 || len > a.max_hyp_len) continue;   // (a used slot never has one: nothing is addressed by a stray length)
    const int S = 2 * len + 1;
    const int32_t* ids = a.hyps + (int64_t)b * a.hyp_stride_b + (int64_t)n * a.hyp_stride_n;
    const double ll = a.ll[slot];
    const double* al = a.alpha + ((int64_t)slot * a.T + t) * a.sstride;
    const double* be = a.beta + ((int64_t)slot * a.T + t) * a.sstride;
    __syncthreads();                           // the class phase of the slot before is over
    for (int i = tid; i < len; i += kGradThreads) y[i] = ids[i];
    for (int s = tid; s < S; s += kGradThreads) {
      const int c = (s & 1) ? ids[(s - 1) >> 1] : a.blank;
      const double x = al[s], z = be[s];
      // alpha and beta both hold the frame's emission: take it out once
      v[s] = (x == LR_NEG_INF_D || z == LR_NEG_INF_D) ? 0.0 : exp(x + z - (double)lpr[c] - ll);
    }
    __syncthreads();
    if (tid < a.C) {
      double occ = 0.0;
      if (tid == a.blank) {
        for (int s = 0; s < S; s += 2) occ += v[s];
      } else {
        for (int i = 0; i < len; ++i)
          if (y[i] == tid) occ += v[2 * i + 1];
      }
      acc += coef * occ;
    }
  }
  if (tid < a.C) out[tid] = (float)(scale * acc);
}

int nbest_args(NbestArgs* a, const NbestPlan& p, const float* log_probs, int64_t stride_b, int64_t stride_t,
               const int32_t* sizes, const int32_t* hyps, int64_t hyp_stride_b, int64_t hyp_stride_n,
               const int32_t* hyp_lens, int64_t lens_stride_b, const float* risk, int blank, int reduction,
               float* hyp_ll, float* post, int32_t* hyp_status, float* utt_risk, float* out_loss, int32_t* out_status,
               float* grad_weight, void* workspace, size_t workspace_bytes, int B, int T, int C, int N,
               int max_hyp_len) {
  LR_CHECK_ARG(blank >= 0 && blank < C && (reduction == LR_CTC_SUM || reduction == LR_CTC_MEAN));
  LR_CHECK_ARG(stride_b >= 0 && stride_t >= 0 && hyp_stride_b >= 0 && hyp_stride_n >= 0 && lens_stride_b >= 0);
  if (workspace_bytes < p.bytes) return LR_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  a->lp = log_probs; a->sizes = sizes; a->hyps = hyps; a->hyp_lens = hyp_lens; a->risk = risk;
  a->hyp_ll = hyp_ll; a->post = post; a->hyp_status = hyp_status; a->utt_risk = utt_risk;
  a->out_loss = out_loss; a->out_status = out_status; a->grad_weight = grad_weight;
  a->grad_scale = nullptr; a->grad = nullptr;
  a->ll = reinterpret_cast<double*>(ws);
  a->coef = reinterpret_cast<double*>(ws + p.off_coef);
  a->alpha = reinterpret_cast<double*>(ws + p.off_alpha);
  a->beta = reinterpret_cast<double*>(ws + p.off_beta);
  a->stride_b = stride_b; a->stride_t = stride_t; a->hyp_stride_b = hyp_stride_b; a->hyp_stride_n = hyp_stride_n;
  a->lens_stride_b = lens_stride_b;
  a->B = B; a->T = T; a->C = C; a->N = N; a->max_hyp_len = max_hyp_len; a->blank = blank; a->reduction = reduction;
  a->sstride = p.sstride;
  return LR_OK;
}

}  // namespace

extern "C" size_t lr_ctc_nbest_workspace_bytes(int B, int T, int C, int N, int max_hyp_len) {
  NbestPlan p;
  if (nbest_plan(B, T, C, N, max_hyp_len, &p) != LR_OK) return 0;
  return p.bytes;
}

extern "C" int lr_ctc_nbest_risk(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                 const int32_t* hyps, int64_t hyp_stride_b, int64_t hyp_stride_n,
                                 const int32_t* hyp_lens, int64_t lens_stride_b, const float* risk, int blank,
                                 int reduction, float* hyp_ll, float* post, int32_t* hyp_status, float* utt_risk,
                                 float* out_loss, int32_t* out_status, float* grad_weight, void* workspace,
                                 size_t workspace_bytes, int B, int T, int C, int N, int max_hyp_len,
                                 lr_stream_t stream) {
  LR_CHECK_ARG(log_probs && hyps && hyp_lens && risk && hyp_ll && post && hyp_status && utt_risk && out_loss &&
               out_status && grad_weight && workspace);
  NbestPlan p;
  int ok = nbest_plan(B, T, C, N, max_hyp_len, &p);
  if (ok != LR_OK) return ok;
  NbestArgs a;
  ok = nbest_args(&a, p, log_probs, stride_b, stride_t, sizes, hyps, hyp_stride_b, hyp_stride_n, hyp_lens,
                  lens_stride_b, risk, blank, reduction, hyp_ll, post, hyp_status, utt_risk, out_loss, out_status,
                  grad_weight, workspace, workspace_bytes, B, T, C, N, max_hyp_len);
  if (ok != LR_OK) return ok;
  LR_LAUNCH(nbest_lattice_kernel, dim3(B * N), dim3(2 * p.half), 0, stream, a);
  ok = lr_launch_status();
  if (ok != LR_OK) return ok;
  LR_LAUNCH(nbest_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream, a);
  return lr_launch_status();
}

extern "C" int lr_ctc_nbest_risk_grad(const float* log_probs, int64_t stride_b, int64_t stride_t,
                                      const int32_t* sizes, const int32_t* hyps, int64_t hyp_stride_b,
                                      int64_t hyp_stride_n, const int32_t* hyp_lens, int64_t lens_stride_b,
                                      const float* risk, int blank, int reduction, const float* hyp_ll,
                                      const float* post, const int32_t* hyp_status, const float* utt_risk,
                                      const float* grad_weight, const float* grad_scale, float* grad, void* workspace,
                                      size_t workspace_bytes, int B, int T, int C, int N, int max_hyp_len,
                                      lr_stream_t stream) {
  LR_CHECK_ARG(log_probs && hyps && hyp_lens && risk && hyp_ll && post && hyp_status && utt_risk && grad_weight &&
               grad && workspace);
  NbestPlan p;
  int ok = nbest_plan(B, T, C, N, max_hyp_len, &p);
  if (ok != LR_OK) return ok;
  NbestArgs a;
  ok = nbest_args(&a, p, log_probs, stride_b, stride_t, sizes, hyps, hyp_stride_b, hyp_stride_n, hyp_lens,
                  lens_stride_b, risk, blank, reduction, const_cast<float*>(hyp_ll), const_cast<float*>(post),
                  const_cast<int32_t*>(hyp_status), const_cast<float*>(utt_risk), nullptr, nullptr,
                  const_cast<float*>(grad_weight), workspace, workspace_bytes, B, T, C, N, max_hyp_len);
  if (ok != LR_OK) return ok;
  a.grad_scale = grad_scale; a.grad = grad;
  LR_LAUNCH(nbest_grad_kernel, dim3(B * T), dim3(kGradThreads), 0, stream, a);
  return lr_launch_status();
}
