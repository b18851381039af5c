// lr_attention.hip — fused multi-head self-attention on the bf16 matrix cores (BASELINE
// configs[4] "transformer encoder over per-frame conv features (self-attn MFMA path)").
//
// BUILD-DEFINED: the reference has no transformer encoder; the specification is
// torch.nn.MultiheadAttention's core as lipreading_amd/transformer.py composes it: per (sample, head)
//   P = softmax_keys(scale * Q K^T, keys >= key_lens[b] masked),  O = P V
// and its backward.  A lip-reading clip is T <= 96 frames, so a whole (sample, head) problem is ONE tile
// set: a workgroup stages Q, K, V (and dO) as bf16 in LDS, runs every contraction on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation, and keeps the softmax (and its backward) in registers:
// the scores are produced TRANSPOSED (keys along MFMA rows), so the 96 keys of a query live in two lanes
// (48 accumulator registers each) and a row reduction is 47 in-lane operations + one lane exchange.
// The T x T probability matrix never touches HBM — the backward recomputes it from Q, K (36 MFMAs) —
// against 4 batched fp32 GEMM launches + 2 softmax launches + 2 x (B, heads, T, T) fp32 round trips of
// the unfused path (lr_sgemm_batched + lr_attn_softmax_*), which stays as the fp32 option.
// Precision: bf16 operands (Q, K, V, dO, P, dS rounded to bf16), fp32 accumulation and softmax:
// ~1e-2 relative on the outputs — the build-defined regime's own precision (its conv stack is bf16).
//
// All six products have both operands K-contiguous in LDS ("NT": C[m][n] = sum_k A[m][k] Bt[n][k]):
//   forward   S^T[key][q] = K[key][:] . Q[q][:]          O[q][d]    = P[q][:]    . V^T[d][:]
//   backward  dP^T[key][q] = V[key][:] . dO[q][:]        dV[key][d] = P^T[key][:] . dO^T[d][:]
//             dK[key][d]  = dS^T[key][:] . Q^T[d][:]     dQ[q][d]   = dS[q][:]   . K^T[d][:]
#include "lr_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short bf16_t;

constexpr int TP = 96;           // padded sequence length: 3 tiles of 32
constexpr int LDT = TP + 8;      // bf16 per row of a [*][TP] buffer (208 B: 16-byte aligned rows)
constexpr int DH_MAX = 64;
constexpr int LDD = DH_MAX + 8;  // bf16 per row of a [TP][dh] buffer (144 B)

__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(bf16_t, h);
}

// one 32x32 output tile: acc += A[m0 + .][0 .. 16 ksteps) . Bt[n0 + .][same]; lane: row/col = lane & 31, k group = lane >> 5
__device__ __forceinline__ void tile_nt(const bf16_t* A, int lda, const bf16_t* Bt, int ldb, int m0, int n0, int ksteps,
                                        f32x16& acc) {
  const int lane = threadIdx.x & 63, lr = lane & 31, kg = lane >> 5;
  const bf16_t* ap = A + (m0 + lr) * lda + 8 * kg;
  const bf16_t* bp = Bt + (n0 + lr) * ldb + 8 * kg;
  for (int ks = 0; ks < ksteps; ++ks) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + 16 * ks);
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(bp + 16 * ks);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
}
// C/D layout of 32x32: column = lane & 31, row of register r = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// rows [0, T) of one head's slice of a [B][T][ld] fp32 tensor -> bf16 row-major dst[TP][LDD] (rows >= T zero) and,
// when dstT != nullptr, transposed dstT[dh][LDT] (columns >= T zero)
__device__ __forceinline__ void stage(const float* __restrict__ src, int ld, int T, int dh, bf16_t* dst, bf16_t* dstT) {
  // 4 consecutive d per thread: one 16-byte global load, one 8-byte LDS store (row-major), four 2-byte stores
  // (transposed); the head slice starts 16-byte aligned (dh % 4 == 0, ld % 4 == 0)
  const int dq = dh >> 2;
  for (int i = threadIdx.x; i < TP * dq; i += blockDim.x) {
    const int t = i / dq, d = 4 * (i - t * dq);
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < T) f = *reinterpret_cast<const float4*>(src + (int64_t)t * ld + d);
    ushort4 v;
    v.x = f2bf(f.x); v.y = f2bf(f.y); v.z = f2bf(f.z); v.w = f2bf(f.w);
    if (dst) *reinterpret_cast<ushort4*>(dst + t * LDD + d) = v;
    if (dstT) {
      dstT[d * LDT + t] = v.x;
      dstT[(d + 1) * LDT + t] = v.y;
      dstT[(d + 2) * LDT + t] = v.z;
      dstT[(d + 3) * LDT + t] = v.w;
    }
  }
}

// softmax over the keys of one query from transposed score tiles: s[kt][r] = score of key 32 kt + crow(r, h); the other
// 48 keys of the query sit in lane ^ 32.  Keys outside the query's window [lo, hi) are masked (lr_attn_window; an empty
// window gives a zero row).  Returns probabilities in place.
// CHUNKED = false: lo is 0 at compile time — the code of the plain key-length mask, instruction for instruction.
template <bool CHUNKED>
__device__ __forceinline__ void softmax_keys(f32x16 (&s)[3], int h, int lo, int hi, float scale) {
  float m = LR_NEG_INF;
#pragma unroll
  for (int kt = 0; kt < 3; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = 32 * kt + crow(r, h);
      s[kt][r] = ((!CHUNKED || key >= lo) && key < hi) ? s[kt][r] * scale : LR_NEG_INF;
      m = fmaxf(m, s[kt][r]);
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (m == LR_NEG_INF) m = 0.f;     // (no valid key: a padded query under the chunk mask; exp(-inf) = 0 below, a zero row)
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < 3; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[kt][r] = __expf(s[kt][r] - m);
      sum += s[kt][r];
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
  for (int kt = 0; kt < 3; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kt][r] *= inv;
}

// ---- forward: grid (nhead, B), 256 threads -----------------------------------------------------------------
template <bool CHUNKED>
__global__ __launch_bounds__(256) void attn_fused_fwd_kernel(const float* __restrict__ qkv,
                                                             const int32_t* __restrict__ key_lens,
                                                             float* __restrict__ out, float scale, int T, int nhead,
                                                             int dh, int chunk, int left_chunks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Qs = reinterpret_cast<bf16_t*>(smem);          // [TP][LDD]
  bf16_t* Ks = Qs + TP * LDD;                            // [TP][LDD]
  bf16_t* Vt = Ks + TP * LDD;                            // [DH_MAX][LDT]
  bf16_t* Ps = Vt + DH_MAX * LDT;                        // [TP][LDT]   P[q][key]
  const int head = blockIdx.x, b = blockIdx.y;
  const int D = nhead * dh, D3 = 3 * D;
  const float* base = qkv + (int64_t)b * T * D3 + head * dh;
  stage(base, D3, T, dh, Qs, nullptr);
  stage(base + D, D3, T, dh, Ks, nullptr);
  stage(base + 2 * D, D3, T, dh, nullptr, Vt);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, h = lane >> 5;
  const int len = min(max(key_lens[b], 1), T);   // a sample of length 0 attends to key 0, as lr_attn_softmax_forward has it
  int lo = 0, hi = len;                          // the window of this lane's query 32 wave + lr
  if (CHUNKED) lr_attn_window(32 * wave + lr, len, chunk, left_chunks, lo, hi);
  if (wave < 3) {     // query tile `wave`: all three key tiles, so a query's 96 scores sit in two lanes
    f32x16 s[3];
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
      tile_nt(Ks, LDD, Qs, LDD, 32 * kt, 32 * wave, dh / 16, s[kt]);
    }
    softmax_keys<CHUNKED>(s, h, lo, hi, scale);
    bf16_t* prow = Ps + (32 * wave + lr) * LDT;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {      // registers 4g .. 4g+3 = keys 32 kt + 8 g + 4 h + {0,1,2,3}
        ushort4 v;
        v.x = f2bf(s[kt][4 * g]); v.y = f2bf(s[kt][4 * g + 1]); v.z = f2bf(s[kt][4 * g + 2]); v.w = f2bf(s[kt][4 * g + 3]);
        *reinterpret_cast<ushort4*>(prow + 32 * kt + 8 * g + 4 * h) = v;
      }
  }
  __syncthreads();
  // O[q][d] = P[q][:] . V^T[d][:]: 3 query tiles x dh/32 column tiles over the four waves
  const int ntile = dh / 32;
  for (int tile = wave; tile < 3 * ntile; tile += 4) {
    const int qt = tile / ntile, dt = tile - qt * ntile;
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    tile_nt(Ps, LDT, Vt, LDT, 32 * qt, 32 * dt, TP / 16, o);
    float* orow = out + (int64_t)b * T * D + head * dh + 32 * dt + lr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = 32 * qt + crow(r, h);
      if (q < T) orow[(int64_t)q * D] = o[r];
    }
  }
}

// ---- backward: grid (nhead, B), 256 threads ----------------------------------------------------------------
template <bool CHUNKED>
__global__ __launch_bounds__(256) void attn_fused_bwd_kernel(const float* __restrict__ qkv,
                                                             const int32_t* __restrict__ key_lens,
                                                             const float* __restrict__ dout, float* __restrict__ dqkv,
                                                             float scale, int T, int nhead, int dh, int chunk,
                                                             int left_chunks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16_t* Qs = reinterpret_cast<bf16_t*>(smem);          // [TP][LDD]
  bf16_t* Ks = Qs + TP * LDD;                            // [TP][LDD]
  bf16_t* Vs = Ks + TP * LDD;                            // [TP][LDD]   } dead after the score products:
  bf16_t* dOs = Vs + TP * LDD;                           // [TP][LDD]   } dS [TP][LDT] aliases this pair
  bf16_t* QsT = dOs + TP * LDD;                          // [DH_MAX][LDT]
  bf16_t* KsT = QsT + DH_MAX * LDT;                      // [DH_MAX][LDT]
  bf16_t* dOT = KsT + DH_MAX * LDT;                      // [DH_MAX][LDT]
  bf16_t* Pt = dOT + DH_MAX * LDT;                       // [TP][LDT]   P^T[key][q]
  bf16_t* dSt = Pt + TP * LDT;                           // [TP][LDT]   dS^T[key][q]
  bf16_t* dS = Vs;                                       // [TP][LDT]   dS[q][key]   (2 * TP * LDD >= TP * LDT)
  const int head = blockIdx.x, b = blockIdx.y;
  const int D = nhead * dh, D3 = 3 * D;
  const float* base = qkv + (int64_t)b * T * D3 + head * dh;
  stage(base, D3, T, dh, Qs, QsT);
  stage(base + D, D3, T, dh, Ks, KsT);
  stage(base + 2 * D, D3, T, dh, Vs, nullptr);
  stage(dout + (int64_t)b * T * D + head * dh, D, T, dh, dOs, dOT);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, h = lane >> 5;
  const int len = min(max(key_lens[b], 1), T);   // a sample of length 0 attends to key 0, as lr_attn_softmax_forward has it
  int lo = 0, hi = len;                          // the window of this lane's query 32 wave + lr
  if (CHUNKED) lr_attn_window(32 * wave + lr, len, chunk, left_chunks, lo, hi);
  f32x16 p[3], dp[3];
  if (wave < 3) {
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) p[kt][r] = dp[kt][r] = 0.f;
      tile_nt(Ks, LDD, Qs, LDD, 32 * kt, 32 * wave, dh / 16, p[kt]);      // S^T
      tile_nt(Vs, LDD, dOs, LDD, 32 * kt, 32 * wave, dh / 16, dp[kt]);    // dP^T
    }
    softmax_keys<CHUNKED>(p, h, lo, hi, scale);
    // dS = P o (dP - sum_keys P o dP) * scale   (softmax backward of scale * S)
    float delta = 0.f;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) delta += p[kt][r] * dp[kt][r];
    delta += __shfl_xor(delta, 32, 64);
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[kt][r] = p[kt][r] * (dp[kt][r] - delta) * scale;
  }
  __syncthreads();   // every wave is done reading Vs / dOs: dS may overwrite them
  if (wave < 3) {
    const int q = 32 * wave + lr;
    bf16_t* srow = dS + q * LDT;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        ushort4 v;
        v.x = f2bf(dp[kt][4 * g]); v.y = f2bf(dp[kt][4 * g + 1]); v.z = f2bf(dp[kt][4 * g + 2]); v.w = f2bf(dp[kt][4 * g + 3]);
        *reinterpret_cast<ushort4*>(srow + 32 * kt + 8 * g + 4 * h) = v;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = 32 * kt + crow(r, h);
        Pt[key * LDT + q] = f2bf(p[kt][r]);
        dSt[key * LDT + q] = f2bf(dp[kt][r]);
      }
    }
  }
  __syncthreads();
  // dV[key][d], dK[key][d], dQ[q][d]: 3 x (3 row tiles x dh/32 column tiles) over the four waves
  const int ntile = dh / 32, per = 3 * ntile;
  float* dbase = dqkv + (int64_t)b * T * D3 + head * dh;
  for (int tile = wave; tile < 3 * per; tile += 4) {
    const int which = tile / per, rem = tile - which * per, mt = rem / ntile, dt = rem - mt * ntile;
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    if (which == 0) tile_nt(Pt, LDT, dOT, LDT, 32 * mt, 32 * dt, TP / 16, o);        // dV
    else if (which == 1) tile_nt(dSt, LDT, QsT, LDT, 32 * mt, 32 * dt, TP / 16, o);  // dK
    else tile_nt(dS, LDT, KsT, LDT, 32 * mt, 32 * dt, TP / 16, o);                   // dQ
    float* orow = dbase + (which == 0 ? 2 * D : (which == 1 ? D : 0)) + 32 * dt + lr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = 32 * mt + crow(r, h);
      if (t < T) orow[(int64_t)t * D3] = o[r];
    }
  }
}

constexpr size_t FWD_LDS = (size_t)(2 * TP * LDD + DH_MAX * LDT + TP * LDT) * sizeof(bf16_t);
constexpr size_t BWD_LDS = (size_t)(4 * TP * LDD + 3 * DH_MAX * LDT + 2 * TP * LDT) * sizeof(bf16_t);
static_assert(2 * TP * LDD >= TP * LDT, "dS must fit the V + dO staging area");

}  // namespace

extern "C" int lr_attn_fused_supported(int T, int dh) { return T >= 1 && T <= TP && (dh == 32 || dh == 64) ? 1 : 0; }

extern "C" int lr_attn_fused_forward_chunked(const float* qkv, const int32_t* key_lens, float* out, float scale, int B,
                                             int T, int nhead, int dh, int chunk, int left_chunks, lr_stream_t stream) {
  LR_CHECK_ARG(qkv && key_lens && out && B > 0 && nhead > 0 && chunk >= 0 && left_chunks >= 0);
  if (!lr_attn_fused_supported(T, dh)) return LR_ERR_UNSUPPORTED;
  static bool attr_set = false;
  lr_clear_error();
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)attn_fused_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)FWD_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)attn_fused_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)FWD_LDS) != hipSuccess)
      return LR_ERR_LAUNCH;
    attr_set = true;
  }
  // (a chunk or a left context past T is T: the same windows, and the kernel's products stay inside an int)
  if (chunk > 0)
    LR_LAUNCH(attn_fused_fwd_kernel<true>, dim3(nhead, B), dim3(256), FWD_LDS, stream, qkv, key_lens, out, scale, T, nhead,
              dh, min(chunk, TP), min(left_chunks, TP));
  else
    LR_LAUNCH(attn_fused_fwd_kernel<false>, dim3(nhead, B), dim3(256), FWD_LDS, stream, qkv, key_lens, out, scale, T, nhead,
              dh, 0, 0);
  return lr_launch_status();
}
extern "C" int lr_attn_fused_forward(const float* qkv, const int32_t* key_lens, float* out, float scale, int B, int T,
                                     int nhead, int dh, lr_stream_t stream) {
  return lr_attn_fused_forward_chunked(qkv, key_lens, out, scale, B, T, nhead, dh, 0, 0, stream);
}

extern "C" int lr_attn_fused_backward_chunked(const float* qkv, const int32_t* key_lens, const float* dout, float* dqkv,
                                              float scale, int B, int T, int nhead, int dh, int chunk, int left_chunks,
                                              lr_stream_t stream) {
  LR_CHECK_ARG(qkv && key_lens && dout && dqkv && B > 0 && nhead > 0 && chunk >= 0 && left_chunks >= 0);
  if (!lr_attn_fused_supported(T, dh)) return LR_ERR_UNSUPPORTED;
  static bool attr_set = false;
  lr_clear_error();
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)attn_fused_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)BWD_LDS) != hipSuccess ||
        hipFuncSetAttribute((const void*)attn_fused_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)BWD_LDS) != hipSuccess)
      return LR_ERR_LAUNCH;
    attr_set = true;
  }
  if (chunk > 0)
    LR_LAUNCH(attn_fused_bwd_kernel<true>, dim3(nhead, B), dim3(256), BWD_LDS, stream, qkv, key_lens, dout, dqkv, scale, T,
              nhead, dh, min(chunk, TP), min(left_chunks, TP));
  else
    LR_LAUNCH(attn_fused_bwd_kernel<false>, dim3(nhead, B), dim3(256), BWD_LDS, stream, qkv, key_lens, dout, dqkv, scale, T,
              nhead, dh, 0, 0);
  return lr_launch_status();
}
extern "C" int lr_attn_fused_backward(const float* qkv, const int32_t* key_lens, const float* dout, float* dqkv,
                                      float scale, int B, int T, int nhead, int dh, lr_stream_t stream) {
  return lr_attn_fused_backward_chunked(qkv, key_lens, dout, dqkv, scale, B, T, nhead, dh, 0, 0, stream);
}
