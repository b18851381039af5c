// Landmark-space augmentation of a collated batch (lr_lmk_augment_f32; the specification is the header's "Landmark
// augmentation" block, DESIGN.md §27 has the measurements).
//
// Two launches.  aug_stats_kernel: one workgroup per clip, its waves stride over the clip's rows.  A wave judges a row
// EMPTY or LIVE with a ballot over all the row's values; every lane keeps float64 sums of the values it owns over its
// wave's LIVE rows in ascending order (one butterfly per wave, not one per row), the lanes are added in a fixed 64-lane
// butterfly (a + b == b + a, so all lanes hold the same bits) and the waves' partials in wave order through LDS: centre,
// RMS radius and the LIVE count, 8 float64 words of the workspace per clip.  aug_apply_kernel: one wave owns one row.
// It reads the WHOLE row into its own LDS stage before it stores anything (the mirror permutation, the EMPTY test and
// in-place use all need that), re-derives EMPTY from what it holds and spreads its lanes over the npts * 3 outputs.
//
// A lane owns the 16-byte chunks lane, lane + 64, lane + 128 of a row (256 points * 12 bytes = 192 chunks), by one
// 16-byte load each where npts is a multiple of 4 and x is 16-byte aligned, by element loads otherwise: the ownership,
// and with it the order of every sum, is the same either way.
#include "lr_common.h"

namespace {
constexpr int AUG_WORDS = 8;          // per clip: c (3), r, LIVE rows, 3 spare
constexpr int AUG_STAT_WAVES = 16;
constexpr int AUG_STAT_ROWS = 4;      // rows a wave of the statistics launch has in flight
constexpr int AUG_APPLY_WAVES = 4;
constexpr int AUG_CHUNKS = LR_LMK_AUG_MAX_POINTS * 3 / 4 / 64;   // chunks a lane owns
static_assert(AUG_CHUNKS * 64 * 4 == LR_LMK_AUG_MAX_POINTS * 3, "a wave's chunks cover the largest row exactly");
static_assert(AUG_WORDS * sizeof(double) * 4 == 256, "the workspace is sized in 256-byte units");

// Six 64-lane butterfly sums side by side: the six exchanges of a step are in flight together, not one behind the other.
__device__ __forceinline__ void aug_wave_sums(double (&v)[6]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    double other[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) other[k] = __shfl_xor(v[k], o, 64);
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += other[k];
  }
}

// This lane's values of the row at X (zeros past the row's end).
__device__ __forceinline__ void aug_load_row(const float* X, int feat, int vec, int lane, float (&v)[AUG_CHUNKS][4]) {
#pragma unroll
  for (int i = 0; i < AUG_CHUNKS; ++i) {
    const int e = (lane + 64 * i) * 4;
    if (vec) {                                   // uniform; feat is a multiple of 4, so a chunk is whole or absent
      const float4 q = e < feat ? *reinterpret_cast<const float4*>(X + e) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[i][u] = e + u < feat ? X[e + u] : 0.f;
    }
  }
}

// Whether any of this lane's values is non-zero / not finite.
__device__ __forceinline__ void aug_row_flags(const float (&v)[AUG_CHUNKS][4], bool& nonzero, bool& nonfinite) {
  nonzero = nonfinite = false;
#pragma unroll
  for (int i = 0; i < AUG_CHUNKS; ++i)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      nonzero |= v[i][u] != 0.f;                 // (a NaN is non-zero here and not finite below)
      nonfinite |= !isfinite(v[i][u]);
    }
}

__device__ __forceinline__ int aug_len(const int32_t* lens, int b, int t_max) { return min(max(lens[b], 0), t_max); }

__global__ __launch_bounds__(AUG_STAT_WAVES * 64) void aug_stats_kernel(const float* __restrict__ x,
                                                                        const int32_t* __restrict__ lens,
                                                                        double* __restrict__ work,
                                                                        double* __restrict__ clip_stats, int t_max,
                                                                        int npts, int vec) {
  __shared__ double part[AUG_STAT_WAVES][7];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  const int feat = npts * 3;
  const int len = aug_len(lens, b, t_max);
  const float* X = x + (int64_t)b * t_max * feat;
  // element e = 4 * (lane + 64 i) + u is coordinate (lane + i + u) % 3 (4 and 256 are 1 mod 3): the sums are kept by
  // m = (i + u) % 3, a compile-time index, and turned to coordinates once, behind the loop
  double s[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
  int live = 0;
  // AUG_STAT_ROWS of the wave's rows are loaded before the first is judged: their latencies overlap.  They are still
  // added in ascending order
  for (int t0 = wave; t0 < len; t0 += AUG_STAT_WAVES * AUG_STAT_ROWS) {   // uniform per wave
    float v[AUG_STAT_ROWS][AUG_CHUNKS][4];
#pragma unroll
    for (int g = 0; g < AUG_STAT_ROWS; ++g) {
      const int t = min(t0 + g * AUG_STAT_WAVES, len - 1);   // (a row past the clip: re-read the last one, not used)
      aug_load_row(X + (int64_t)t * feat, feat, vec, lane, v[g]);
    }
#pragma unroll
    for (int g = 0; g < AUG_STAT_ROWS; ++g) {
      bool nz, nf;
      aug_row_flags(v[g], nz, nf);
      if (t0 + g * AUG_STAT_WAVES >= len || __any(nf) || !__any(nz)) continue;   // past the clip, or EMPTY
      ++live;
#pragma unroll
      for (int i = 0; i < AUG_CHUNKS; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double d = (double)v[g][i][u];
          s[(i + u) % 3] += d;
          q[(i + u) % 3] += d * d;
        }
    }
  }
  const int c0 = lane % 3;                                   // coordinate k is m = (k - c0) mod 3
  double sums[6];                                            // sum x, y, z, then sum x^2, y^2, z^2
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int m = (k - c0 + 3) % 3;
    sums[k] = m == 0 ? s[0] : m == 1 ? s[1] : s[2];
    sums[3 + k] = m == 0 ? q[0] : m == 1 ? q[1] : q[2];
  }
  aug_wave_sums(sums);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) part[wave][k] = sums[k];
    part[wave][6] = (double)live;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int w = 0; w < AUG_STAT_WAVES; ++w)                   // wave order
#pragma unroll
    for (int k = 0; k < 7; ++k) tot[k] += part[w][k];
  double c[3] = {0.0, 0.0, 0.0}, r = 0.0;
  if (tot[6] > 0.0) {
    const double n = tot[6] * (double)npts;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = tot[k] / n;
    const double m2 = (tot[3] + tot[4] + tot[5]) / n;
    r = sqrt(fmax(m2 - (c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), 0.0));
  }
  double* W = work + (int64_t)b * AUG_WORDS;
  W[0] = c[0]; W[1] = c[1]; W[2] = c[2]; W[3] = r; W[4] = tot[6]; W[5] = W[6] = W[7] = 0.0;
  if (clip_stats) {
    double* C = clip_stats + (int64_t)b * 4;
    C[0] = c[0]; C[1] = c[1]; C[2] = c[2]; C[3] = r;
  }
}

// splitmix64's finaliser (augment._mix)
__device__ __forceinline__ uint64_t aug_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// x and y may be the same buffer: neither is __restrict__
__global__ __launch_bounds__(AUG_APPLY_WAVES * 64) void aug_apply_kernel(const float* x, const int32_t* __restrict__ lens,
                                                                         const double* __restrict__ rec,
                                                                         const uint64_t* __restrict__ rec_words,
                                                                         const int32_t* __restrict__ perm,
                                                                         const double* __restrict__ work, float* y,
                                                                         int64_t rows, int t_max, int npts, int vec) {
  __shared__ __attribute__((aligned(16))) float stage[AUG_APPLY_WAVES][LR_LMK_AUG_MAX_POINTS * 3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * AUG_APPLY_WAVES + wave;
  const bool active = n < rows;                              // uniform per wave
  const int feat = npts * 3;
  float* S = stage[wave];
  float v[AUG_CHUNKS][4];
  bool nz = false, nf = false;
  if (active) {
    aug_load_row(x + n * feat, feat, vec, lane, v);
    aug_row_flags(v, nz, nf);
#pragma unroll
    for (int i = 0; i < AUG_CHUNKS; ++i) {
      const int e = (lane + 64 * i) * 4;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e + u < feat) S[e + u] = v[i][u];
    }
  }
  __syncthreads();                                           // the whole row is staged before anything is stored
  if (!active) return;
  const int b = (int)(n / t_max), t = (int)(n - (int64_t)b * t_max);
  const bool live = t < aug_len(lens, b, t_max) && !__any(nf) && __any(nz);
  const double* R = rec + (int64_t)b * LR_LMK_AUG_REC_WORDS;
  const double* W = work + (int64_t)b * AUG_WORDS;
  const double jitter = R[12], r = W[3];
  const bool mirror = R[13] != 0.0;
  const uint64_t key = rec_words[(int64_t)b * LR_LMK_AUG_REC_WORDS + 14] + 0x9E3779B97F4A7C15ull;
  float* Y = y + n * feat;
#pragma unroll
  for (int i = 0; i < AUG_CHUNKS; ++i) {
    const int e0 = (lane + 64 * i) * 4;
    if (e0 >= feat) break;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u;
        if (e >= feat) break;
        const int j = e / 3, k = e - j * 3;
        const int src = mirror ? min(max(perm[j], 0), npts - 1) : j;   // whatever perm holds, a point of this row
        const double d0 = (double)S[src * 3] - W[0], d1 = (double)S[src * 3 + 1] - W[1], d2 = (double)S[src * 3 + 2] - W[2];
        const double a0 = k == 0 ? R[0] : k == 1 ? R[3] : R[6];
        const double a1 = k == 0 ? R[1] : k == 1 ? R[4] : R[7];
        const double a2 = k == 0 ? R[2] : k == 1 ? R[5] : R[8];
        const double ck = k == 0 ? W[0] : k == 1 ? W[1] : W[2];
        double add = k == 0 ? R[9] : k == 1 ? R[10] : R[11];
        if (jitter != 0.0) {
          const uint64_t z = aug_mix(key + (uint64_t)(((int64_t)t * npts + j) * 3 + k));
          const int sum16 = (int)(z & 0xFFFFu) + (int)((z >> 16) & 0xFFFFu) + (int)((z >> 32) & 0xFFFFu) + (int)(z >> 48);
          add += jitter * ((double)(sum16 - 131070) * 2.6428997921303014e-05);
        }
        o[u] = (float)((a0 * d0 + a1 * d1 + a2 * d2) + ck + r * add);
      }
    }
    if (vec) {
      *reinterpret_cast<float4*>(Y + e0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u < feat) Y[e0 + u] = o[u];
    }
  }
}
}  // namespace

extern "C" size_t lr_lmk_augment_workspace_bytes(int B) {
  if (B < 1) return 0;
  return lr_align_up((size_t)B * AUG_WORDS * sizeof(double), 256);
}

extern "C" int lr_lmk_augment_f32(const float* x, const int32_t* lens, const void* rec, const int32_t* mirror_perm,
                                  float* y, double* clip_stats, void* workspace, size_t workspace_bytes, int B, int t_max,
                                  int npts, lr_stream_t stream) {
  LR_CHECK_ARG(x && lens && rec && mirror_perm && y && workspace);
  if (npts < 1 || npts > LR_LMK_AUG_MAX_POINTS || B < 1 || t_max < 1 || (int64_t)B * t_max > INT32_MAX)
    return LR_ERR_UNSUPPORTED;
  const int64_t rows = (int64_t)B * t_max;
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
  const uintptr_t bytes = (uintptr_t)rows * npts * 3 * sizeof(float);
  LR_CHECK_ARG(xa == ya || xa + bytes <= ya || ya + bytes <= xa);
  LR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(rec) & 7) == 0);
  if (workspace_bytes < lr_lmk_augment_workspace_bytes(B)) return LR_ERR_WORKSPACE;
  const int vec = npts % 4 == 0 && ((xa | ya) & 15) == 0;
  double* work = (double*)workspace;
  LR_LAUNCH(aug_stats_kernel, dim3((unsigned)B), dim3(AUG_STAT_WAVES * 64), 0, stream, x, lens, work, clip_stats, t_max,
            npts, vec);
  const int st = lr_launch_status();
  if (st != LR_OK) return st;
  LR_LAUNCH(aug_apply_kernel, dim3((unsigned)((rows + AUG_APPLY_WAVES - 1) / AUG_APPLY_WAVES)), dim3(AUG_APPLY_WAVES * 64),
            0, stream, x, lens, (const double*)rec, (const uint64_t*)rec, mirror_perm, work, y, rows, t_max, npts, vec);
  return lr_launch_status();
}
