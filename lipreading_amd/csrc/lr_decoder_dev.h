// lr_decoder_dev.h — the forward pieces of one attention-decoder step, shared by lr_decoder.hip (the
// training / eval loop) and lr_attn_beam.hip (beam search).  Internal: every includer gets its own copy of
// the kernels (anonymous namespace).
#pragma once
#include "lr_common.h"

namespace {

enum { ATT_NONE = 0, ATT_DOT = 1, ATT_GENERAL = 2, ATT_1LNN = 3, ATT_CONCAT = 4 };
constexpr int OUT_ROWS = 8;   // rows per workgroup of dec_out_fwd_kernel

// gates[b][i][:] = EW[id][:] for steps i0 + blockIdx.x; id = teacher-forced token or the previous
// step's sample (step 0 always reads tokens: the reference feeds BOS)
__global__ __launch_bounds__(256) void dec_gather_kernel(const float* __restrict__ EW,
                                                         const int32_t* __restrict__ tokens,
                                                         const int32_t* __restrict__ sampled,
                                                         int32_t* __restrict__ ids_used,
                                                         float* __restrict__ gates, int L, int GH, int V, int i0,
                                                         int teacher) {
  const int i = i0 + blockIdx.x, b = blockIdx.y;
  int id = (teacher || i == 0) ? tokens[(int64_t)b * L + i] : sampled[(int64_t)b * L + i - 1];
  if (id < 0 || id >= V) id = 0;
  if (threadIdx.x == 0) ids_used[(int64_t)b * L + i] = id;
  const float4* src = reinterpret_cast<const float4*>(EW + (int64_t)id * GH);
  float4* dst = reinterpret_cast<float4*>(gates + ((int64_t)b * L + i) * GH);
  for (int c = threadIdx.x; c < GH / 4; c += blockDim.x) dst[c] = src[c];
}

// concat attention: logits[b][i][t] = w2 . tanh(PE[b][t][:] + ph[b][i][:]) + b2.  grid (steps, B)
__global__ __launch_bounds__(256) void dec_concat_logits_kernel(const float* __restrict__ PE,
                                                                const float* __restrict__ ph,
                                                                const float* __restrict__ w2,
                                                                const float* __restrict__ b2,
                                                                float* __restrict__ logits, int L, int T, int A,
                                                                int i0) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* phs = reinterpret_cast<float*>(smem_raw);   // [A]
  float* w2s = phs + A;                              // [A]
  const int i = i0 + blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = (int64_t)b * L + i;
  for (int r = tid; r < A; r += 256) { phs[r] = ph[row * A + r]; w2s[r] = w2[r]; }
  __syncthreads();
  const float* peb = PE + (int64_t)b * T * A;
  for (int t = wave; t < T; t += 4) {
    float s = 0.f;
    for (int r = lane; r < A; r += 64) s += w2s[r] * tanhf(peb[(int64_t)t * A + r] + phs[r]);
    s = lr_wave_sum(s);
    if (lane == 0) logits[row * T + t] = s + b2[0];
  }
}

// One wave per (sample, step) row: finish the raw logits (1_layer_nn: se[b][t] + w_h . h + b;
// general: + cE[b][t]), then allennlp masked_softmax: softmax(logits * mask) * mask / (sum + 1e-13).
// grid (steps, B), 64 threads.
__global__ __launch_bounds__(64) void dec_attn_softmax_kernel(int type, const float* __restrict__ hs,
                                                              const int32_t* __restrict__ enc_lens,
                                                              const float* __restrict__ cterm,
                                                              const float* __restrict__ wvec,
                                                              const float* __restrict__ bias_p,
                                                              float* __restrict__ logits,
                                                              float* __restrict__ wts, int L, int T, int Hd,
                                                              int i0) {
  const int i = i0 + blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int64_t row = (int64_t)b * L + i;
  float* lg = logits + row * T;
  if (type == ATT_1LNN) {
    const float* h = hs + row * Hd;
    float s = 0.f;
    for (int k = lane; k < Hd; k += 64) s += h[k] * wvec[k];
    const float sh = lr_wave_sum(s) + bias_p[0];
    for (int t = lane; t < T; t += 64) lg[t] = cterm[(int64_t)b * T + t] + sh;
  } else if (type == ATT_GENERAL) {
    for (int t = lane; t < T; t += 64) lg[t] += cterm[(int64_t)b * T + t];
  }
  // (each lane re-reads only the entries it wrote)
  const int len = min(enc_lens[b], T);
  float mx = LR_NEG_INF;
  for (int t = lane; t < T; t += 64) mx = fmaxf(mx, t < len ? lg[t] : 0.f);
  mx = lr_wave_max(mx);
  float se = 0.f, sv = 0.f;
  for (int t = lane; t < T; t += 64) {
    const float e = expf((t < len ? lg[t] : 0.f) - mx);
    se += e;
    if (t < len) sv += e;
  }
  const float Z = lr_wave_sum(se);
  const float S = lr_wave_sum(sv) / Z;   // sum of the masked probabilities
  float* w = wts + row * T;
  for (int t = lane; t < T; t += 64) w[t] = t < len ? (expf(lg[t] - mx) / Z) / (S + 1e-13f) : 0.f;
}

__device__ __forceinline__ float hash_uniform(uint64_t seed, uint32_t step, uint32_t sample) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)step * 0x100000001B3ull + sample + 1);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (float)(x >> 40) * (1.f / 16777216.f);   // 24 random bits -> [0,1)
}

// `nrows` (<= OUT_ROWS) rows per workgroup: new_h = tanh(pre) (stored back), logits = W_o new_h +
// b_o + log(mask + 1e-45), log-softmax, multinomial draw.  With has_attn == 0 the input rows are
// the RNN states themselves (no tanh).  Rows of the segment [i0, i0 + n): q -> (b = q / n, i = i0 + q % n).
// DRAW = false (beam search) stops after the log-probabilities: no draw, `sampled` is not written.
template <bool DRAW>
__global__ __launch_bounds__(256) void dec_out_fwd_kernel(float* __restrict__ nh, const float* __restrict__ w_o,
                                                          const float* __restrict__ b_o,
                                                          const float* __restrict__ mask,
                                                          float* __restrict__ log_probs,
                                                          int32_t* __restrict__ sampled, int L, int Hd, int V,
                                                          int i0, int n, int total, int nrows, int has_attn,
                                                          uint64_t seed) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* x = reinterpret_cast<float*>(smem_raw);   // [nrows][Hd]
  float* lg = x + (size_t)nrows * Hd;              // [nrows][V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * nrows;
  const int H4 = Hd >> 2;
  for (int idx = tid; idx < nrows * H4; idx += 256) {
    const int r = idx / H4, k4 = idx - r * H4;
    const int q = q0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < total) {
      const int64_t row = (int64_t)(q / n) * L + i0 + q % n;
      float4* src = reinterpret_cast<float4*>(nh + row * Hd) + k4;
      v = *src;
      if (has_attn) {
        v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w);
        *src = v;
      }
    }
    *reinterpret_cast<float4*>(&x[(size_t)r * Hd + 4 * k4]) = v;
  }
  __syncthreads();
  // 4 lanes per output class, each a quarter of the k range in 16-byte pieces; all loads of a
  // class row are independent, so they are in flight together
  const int q4 = tid & 3;
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
          if (r < nrows) {
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
        if (r < nrows) lg[(size_t)r * V + v] = acc[r] + add;
    }
  }
  __syncthreads();
  for (int r = wave; r < nrows; r += 4) {
    const int q = q0 + r;
    if (q >= total) continue;   // wave-uniform
    const int b = q / n, i = i0 + q % n;
    const int64_t row = (int64_t)b * L + i;
    float* l = lg + (size_t)r * V;
    float m = LR_NEG_INF;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, l[v]);
    m = lr_wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(l[v] - m);
    s = lr_wave_sum(s);
    const float lse = m + logf(s);
    float* out = log_probs + row * V;
    float tot = 0.f;
    for (int v = lane; v < V; v += 64) {
      const float lp = l[v] - lse;
      l[v] = lp;
      out[v] = lp;
      tot += expf(lp);
    }
    if constexpr (!DRAW) continue;
    tot = lr_wave_sum(tot);
    // multinomial(1) over exp(log_probs): first class whose cumulative mass exceeds u * total
    const float u = hash_uniform(seed, (uint32_t)i, (uint32_t)b);
    float running = 0.f;
    int pick = V - 1;
    bool found = false;
    for (int vc = 0; vc < V; vc += 64) {
      const int v = vc + lane;
      float c = v < V ? expf(l[v]) : 0.f;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const float t = __shfl_up(c, d, 64);
        if (lane >= d) c += t;
      }
      const unsigned long long hit = __ballot(v < V && u * tot < running + c);
      if (!found && hit) {
        pick = vc + __ffsll((long long)hit) - 1;
        found = true;
      }
      running += __shfl(c, 63, 64);
    }
    if (lane == 0) sampled[row] = pick;
  }
}

}  // namespace
