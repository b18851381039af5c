// Head-pose normalisation of landmarks inside the collate launch (lr_lmk_pose_collate_f32; the specification is the
// header's "Landmark pose" block, DESIGN.md §26 has the measurements).
//
// Two launches.  pose_stats_kernel: one wave per source row, lanes over the rigid points; centroid, the 3x3 cross
// covariance with the template and the spread, every sum a fixed 64-lane butterfly in float64 (a + b == b + a, so all
// lanes hold the same bits), into 14 float64 words of the workspace.  pose_apply_kernel: one wave per (sample, frame)
// pair; it sums the window's statistics in ascending row order, solves for the rotation — Horn's 4x4 symmetric matrix,
// a fixed number of cyclic Jacobi sweeps, every lane for itself since all of it is uniform: no LDS, no barrier — and
// spreads its lanes over the npts * 3 outputs.  The wave of pair (b, t) also writes `pose` and `status` of row t of
// sample b (and of rows t + t_max, ... should lens[b] exceed t_max), so every row has them whatever the map says; in a
// batch without a map that row is the pair's source row and the one solve serves both.
#include "lr_common.h"

namespace {
constexpr int POSE_WORDS = 14;    // per row: centroid (3), M row-major (9), v, BAD
constexpr int POSE_SWEEPS = 6;    // cyclic Jacobi on a 4x4 converges quadratically: float64 inside these (8 give the same bits)

struct PoseRigid { uint32_t word[LR_POSE_MAX_RIGID / 4]; };   // the rigid indices, one byte each (npts <= 256)

__device__ __forceinline__ double pose_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One Jacobi rotation of the symmetric A in the (P, Q) plane, accumulated into the eigenvector columns of V.
template <int P, int Q>
__host__ __device__ __forceinline__ void pose_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // an overflowing theta: t = 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = A[k][P], b = A[k][Q];
    A[k][P] = c * a - s * b;
    A[k][Q] = s * a + c * b;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = A[P][k], b = A[Q][k];
    A[P][k] = c * a - s * b;
    A[Q][k] = s * a + c * b;
  }
  A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = V[k][P], b = V[k][Q];
    V[k][P] = c * a - s * b;
    V[k][Q] = s * a + c * b;
  }
}

// The proper rotation R (row-major) that maximises tr(R M^T), M = sum (q - qbar)(p - pbar)^T: the unit quaternion that
// is the eigenvector of Horn's matrix with the largest eigenvalue.  M = 0 gives the identity.
__host__ __device__ __forceinline__ void pose_rotation(const double* M, double* R) {
  // Horn's S = sum p q^T = M^T
  const double Sxx = M[0], Syx = M[1], Szx = M[2], Sxy = M[3], Syy = M[4], Szy = M[5], Sxz = M[6], Syz = M[7], Szz = M[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
  for (int sweep = 0; sweep < POSE_SWEEPS; ++sweep) {
    pose_rotate<0, 1>(A, V);
    pose_rotate<0, 2>(A, V);
    pose_rotate<0, 3>(A, V);
    pose_rotate<1, 2>(A, V);
    pose_rotate<1, 3>(A, V);
    pose_rotate<2, 3>(A, V);
  }
  double best = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > best) {
      best = A[k][k];
      w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k];
    }
  const double inv = 1.0 / (w * w + x * x + y * y + z * z);   // V is orthogonal: 1 up to rounding
  R[0] = (w * w + x * x - y * y - z * z) * inv;
  R[1] = 2.0 * (x * y - w * z) * inv;
  R[2] = 2.0 * (x * z + w * y) * inv;
  R[3] = 2.0 * (x * y + w * z) * inv;
  R[4] = (w * w - x * x + y * y - z * z) * inv;
  R[5] = 2.0 * (y * z - w * x) * inv;
  R[6] = 2.0 * (x * z - w * y) * inv;
  R[7] = 2.0 * (y * z + w * x) * inv;
  R[8] = (w * w - x * x - y * y + z * z) * inv;
}

// stats [rows][POSE_WORDS] and, behind them, the template's rigid centroid (3 words, written by row 0's wave).
__global__ __launch_bounds__(256) void pose_stats_kernel(const float* __restrict__ lmk, const float* __restrict__ tmpl,
                                                         PoseRigid rigid, int n_rigid, double* __restrict__ stats,
                                                         int64_t rows, int npts) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= rows) return;                     // uniform per wave
  const float* L = lmk + n * npts * 3;
  int bad = 0;
  for (int k = lane; k < npts * 3; k += 64) bad |= !isfinite(L[k]);
  bad = __any(bad);
  // this lane's rigid index (a select per word: indexing the argument by lane would put it into scratch)
  uint32_t word = 0;
#pragma unroll
  for (int w = 0; w < LR_POSE_MAX_RIGID / 4; ++w) word = (lane >> 2) == w ? rigid.word[w] : word;
  const int j = (int)((word >> (8 * (lane & 3))) & 255u);
  const bool on = lane < n_rigid;            // (j < npts: the entry checked every index)
  double p[3], q[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p[c] = on ? (double)L[j * 3 + c] : 0.0;
    q[c] = on ? (double)tmpl[j * 3 + c] : 0.0;
  }
  const double cnt = (double)n_rigid;
  double pb[3], qb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pb[c] = pose_wave_sum(p[c]) / cnt;
    qb[c] = pose_wave_sum(q[c]) / cnt;
    p[c] = on ? p[c] - pb[c] : 0.0;
    q[c] = on ? q[c] - qb[c] : 0.0;
  }
  double M[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[a * 3 + c] = pose_wave_sum(q[a] * p[c]);
  const double v = pose_wave_sum(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  if (lane == 0) {
    double* S = stats + n * POSE_WORDS;
#pragma unroll
    for (int c = 0; c < 3; ++c) S[c] = pb[c];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[3 + k] = M[k];
    S[12] = v;
    S[13] = bad ? 1.0 : 0.0;
    if (n == 0) {
      double* Q = stats + rows * POSE_WORDS;
      Q[0] = qb[0]; Q[1] = qb[1]; Q[2] = qb[2];
    }
  }
}

__global__ __launch_bounds__(64) void pose_apply_kernel(const float* __restrict__ lmk, const double* __restrict__ stats,
                                                        const int64_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ lens,
                                                        const int32_t* __restrict__ tmap, float* __restrict__ out,
                                                        float* __restrict__ pose, int32_t* __restrict__ status,
                                                        int64_t rows, int t_max, int npts, int radius, int scale) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x / t_max, t = blockIdx.x - b * t_max;
  const int feat = npts * 3;
  float* O = out + (int64_t)blockIdx.x * feat;
  const int64_t first = offsets[b];
  int len = lens[b];
  if (first < 0 || first >= rows || len <= 0) len = 0;      // uniform; never outside lmk, the workspace or tmap
  len = (int)min((int64_t)len, rows - first);
  int m = -1;                                // the map value: < 0 is a frame of zeros
  if (t < min(len, t_max)) m = tmap ? tmap[first + t] : t;
  const int src = min(max(m, 0), len - 1);   // whatever the map holds, the row is one of sample b's
  const double* Q = stats + rows * POSE_WORDS;
  const double qb0 = Q[0], qb1 = Q[1], qb2 = Q[2];
  bool written = false;
  // rows t, t + t_max, ... of the sample (their pose and status), then the source row if it was not among them
  for (int i = t;; i += t_max) {
    const bool own = i < len;
    if (!own && (m < 0 || written)) break;
    const int r = own ? i : src;
    const double* S = stats + (first + r) * POSE_WORDS;
    const bool bad = S[13] != 0.0;
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, v = 0.0;
    int used = 0;
    const int j1 = min(len - 1, r + radius);
    for (int j = max(0, r - radius); j <= j1; ++j) {         // ascending, the non-BAD rows only
      const double* W = stats + (first + j) * POSE_WORDS;
      if (W[13] != 0.0) continue;
#pragma unroll
      for (int k = 0; k < 9; ++k) M[k] += W[3 + k];
      v += W[12];
      ++used;
    }
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, s = 1.0;
    double pb0 = 0.0, pb1 = 0.0, pb2 = 0.0;
    int st = LR_POSE_BAD_ROW;
    if (!bad) {
      pb0 = S[0]; pb1 = S[1]; pb2 = S[2];
      st = LR_POSE_DEGENERATE;
      if (used > 0 && v != 0.0) {
        st = LR_POSE_OK;
        pose_rotation(M, R);
        if (scale) {
          double tr = 0.0;
#pragma unroll
          for (int k = 0; k < 9; ++k) tr += R[k] * M[k];
          s = tr / v;
        }
      }
    }
    if (own && lane == 0) {
      status[first + r] = st;
      if (pose) {
        float* P = pose + (first + r) * 13;
#pragma unroll
        for (int k = 0; k < 9; ++k) P[k] = (float)R[k];
        P[9] = (float)s;
        P[10] = (float)pb0; P[11] = (float)pb1; P[12] = (float)pb2;
      }
    }
    if (m >= 0 && r == src && !written) {
      written = true;
      const float* L = lmk + (first + r) * feat;
      for (int k = lane; k < feat; k += 64) {
        const int pt = k / 3, c = k - pt * 3;
        const double x0 = (double)L[pt * 3] - pb0, x1 = (double)L[pt * 3 + 1] - pb1, x2 = (double)L[pt * 3 + 2] - pb2;
        const double r0 = c == 0 ? R[0] : c == 1 ? R[3] : R[6];
        const double r1 = c == 0 ? R[1] : c == 1 ? R[4] : R[7];
        const double r2 = c == 0 ? R[2] : c == 1 ? R[5] : R[8];
        const double qc = c == 0 ? qb0 : c == 1 ? qb1 : qb2;
        O[k] = bad ? 0.f : (float)(s * (r0 * x0 + r1 * x1 + r2 * x2) + qc);
      }
    }
    if (!own) break;
  }
  if (!written)                              // padding or a masked frame
    for (int k = lane; k < feat; k += 64) O[k] = 0.f;
}
}  // namespace

extern "C" size_t lr_lmk_pose_workspace_bytes(int64_t rows, int n_rigid, int radius) {
  if (rows <= 0 || rows > INT32_MAX || n_rigid < 3 || n_rigid > LR_POSE_MAX_RIGID || radius < 0 ||
      radius > LR_POSE_MAX_RADIUS)
    return 0;
  return lr_align_up(((size_t)rows * POSE_WORDS + 3) * sizeof(double), 256);   // the rows' statistics, the template's centroid
}

extern "C" int lr_lmk_pose_collate_f32(const float* lmk, const int64_t* offsets, const int32_t* lens, const int32_t* tmap,
                                       const float* tmpl, const int32_t* rigid_host, int n_rigid, float* out, float* pose,
                                       int32_t* status, void* workspace, size_t workspace_bytes, int B, int64_t rows,
                                       int t_max, int npts, int radius, int flags, lr_stream_t stream) {
  LR_CHECK_ARG(lmk && offsets && lens && tmpl && rigid_host && out && status && workspace);
  if (n_rigid < 3 || n_rigid > LR_POSE_MAX_RIGID || npts < 1 || npts > LR_POSE_MAX_POINTS || radius < 0 ||
      radius > LR_POSE_MAX_RADIUS || (flags & ~LR_POSE_SCALE))
    return LR_ERR_UNSUPPORTED;
  PoseRigid rigid;
  __builtin_memset(&rigid, 0, sizeof(rigid));
  bool seen[LR_POSE_MAX_POINTS] = {false};
  for (int i = 0; i < n_rigid; ++i) {
    const int32_t j = rigid_host[i];
    LR_CHECK_ARG(j >= 0 && j < npts && !seen[j]);
    seen[j] = true;
    rigid.word[i >> 2] |= (uint32_t)j << (8 * (i & 3));
  }
  LR_CHECK_ARG(B > 0 && rows > 0 && t_max > 0 && (int64_t)B * t_max <= INT32_MAX);
  const size_t need = lr_lmk_pose_workspace_bytes(rows, n_rigid, radius);
  LR_CHECK_ARG(need > 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  if (workspace_bytes < need) return LR_ERR_WORKSPACE;
  double* stats = (double*)workspace;
  LR_LAUNCH(pose_stats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, lmk, tmpl, rigid, n_rigid, stats,
            rows, npts);
  const int st = lr_launch_status();
  if (st != LR_OK) return st;
  LR_LAUNCH(pose_apply_kernel, dim3(B * t_max), dim3(64), 0, stream, lmk, stats, offsets, lens, tmap, out, pose, status,
            rows, t_max, npts, radius, (flags & LR_POSE_SCALE) ? 1 : 0);
  return lr_launch_status();
}
