// lr_transducer.hip — the transducer head (BUILD-DEFINED; include/lipreading_hip.h A6i): the RNN-T loss
// with its gradients and the greedy decoder.
//
// Layout of the loss.  A TILE is 32 lattice nodes of one frame: (t, u0 .. u0 + 31).  For a tile the joint stage runs in
// LDS: Z[32][J] = tanh(e_t + p_u), the logits Z . W^T on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation: a
// k-ordered fmaf chain), bias and class mask, and a log-sum-exp per node.  The forward keeps three floats per node
// (log p(blank), log p(next label), the log-sum-exp); alpha and beta walk the anti-diagonals in log space and fp64 (the
// occupancies exp(alpha + lp + beta - log Z) cancel three numbers that reach the hundreds), one workgroup per sample,
// the previous diagonal in LDS.  The backward recomputes a tile's Z and logits, turns them into
// the gradient at the logits G from the occupancies, and runs two more products per tile: dZ = G . W (then
// d pre-activation = dZ (1 - Z^2), summed over the tile's u for d_e and over the workgroup's frames for d_p) and
// dW += G^T . Z.  Every sum that crosses workgroups goes through a slab per workgroup and a fixed-order combine; there
// is no atomic anywhere, so two runs give the same bits.
#include "lr_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;         // nodes per tile; also the MFMA tile edge
constexpr int kMinFrames = 4;     // a backward workgroup walks at least this many frames (fewer, larger slabs)
constexpr int kMaxSlabs = 512;    // about this many backward workgroups = weight-gradient slabs

struct Plan {
  int B, T, U, U1, V1, J, V1p, Jp, UB, TS, tchunk;
  size_t nodes;                                   // B * T * U1
  size_t off_wp, off_lpb, off_lpl, off_lse, off_alpha, off_beta, off_logz, off_gw, off_de, off_dp, off_dw, off_db;   // floats
  size_t bytes, lds;
};

int make_plan(int B, int T, int U, int V1, int J, Plan* p) {
  if (B < 1 || T < 1 || U < 0 || V1 < 2 || J < 1) return LR_ERR_INVALID_ARG;
  if (B > 65535 || T > LR_RNNT_MAX_T || U > LR_RNNT_MAX_U || V1 > LR_RNNT_MAX_CLASSES || J > LR_RNNT_MAX_JOINT)
    return LR_ERR_UNSUPPORTED;
  p->B = B; p->T = T; p->U = U; p->U1 = U + 1; p->V1 = V1; p->J = J;
  p->V1p = (V1 + 31) / 32 * 32;
  p->Jp = (J + 31) / 32 * 32;
  p->UB = (p->U1 + kTile - 1) / kTile;
  int ts = kMaxSlabs / (B * p->UB);
  const int ts_max = (T + kMinFrames - 1) / kMinFrames;
  ts = ts < 1 ? 1 : (ts > ts_max ? ts_max : ts);
  p->tchunk = (T + ts - 1) / ts;
  p->TS = (T + p->tchunk - 1) / p->tchunk;
  if (p->TS > 65535 || T > 65535) return LR_ERR_UNSUPPORTED;
  p->nodes = (size_t)B * T * p->U1;
  const size_t nwg = (size_t)B * p->TS * p->UB;
  size_t o = 0;
  auto take = [&](size_t n) { size_t at = o; o += lr_align_up(n, 4); return at; };
  p->off_wp = take((size_t)p->V1p * p->Jp);
  p->off_lpb = take(p->nodes);
  p->off_lpl = take(p->nodes);
  p->off_lse = take(p->nodes);
  p->off_alpha = take(2 * p->nodes);   // fp64
  p->off_beta = take(2 * p->nodes);    // fp64
  p->off_logz = take(2 * (size_t)B);   // fp64
  p->off_gw = take(B);
  p->off_de = take((size_t)p->UB * B * T * p->Jp);
  p->off_dp = take((size_t)p->TS * B * p->U1 * p->Jp);
  p->off_dw = take(nwg * p->V1p * p->Jp);
  p->off_db = take(nwg * p->V1p);
  p->bytes = o * sizeof(float);
  p->lds = ((size_t)kTile * (p->Jp + 4) + (size_t)kTile * (p->V1p + 4)) * sizeof(float);
  return LR_OK;
}

struct Args {
  const float* e; int64_t e_sb, e_st;
  const float* p;            // [B][U1][J]
  const float* w;            // [V1][J]
  const float* bias;         // [V1]
  const float* mask;         // [V1], 0 = masked
  const int32_t* labels; int64_t l_sb;
  const int32_t* flens;
  const int32_t* llens;
  float* nll; int32_t* sstat; float* loss; int32_t* bstat;
  const float* gscale;
  float *d_e, *d_p, *d_w, *d_b;
  float *wp, *lpb, *lpl, *lse, *gw, *de_s, *dp_s, *dw_s, *db_s;
  double *alpha, *beta, *logz;
  int B, T, U, U1, V1, J, V1p, Jp, UB, TS, tchunk, reduction, accumulate;
};

void fill_args(Args* a, const Plan& p, void* workspace) {
  float* ws = (float*)workspace;
  a->wp = ws + p.off_wp; a->lpb = ws + p.off_lpb; a->lpl = ws + p.off_lpl; a->lse = ws + p.off_lse;
  a->alpha = (double*)(ws + p.off_alpha); a->beta = (double*)(ws + p.off_beta); a->logz = (double*)(ws + p.off_logz);
  a->gw = ws + p.off_gw; a->de_s = ws + p.off_de;
  a->dp_s = ws + p.off_dp; a->dw_s = ws + p.off_dw; a->db_s = ws + p.off_db;
  a->B = p.B; a->T = p.T; a->U = p.U; a->U1 = p.U1; a->V1 = p.V1; a->J = p.J; a->V1p = p.V1p; a->Jp = p.Jp;
  a->UB = p.UB; a->TS = p.TS; a->tchunk = p.tchunk;
}

// ---- launch 1 of the forward: the zero-padded weight operand and the per-sample status ---------------------------------
__global__ void __launch_bounds__(kThreads) rnnt_prep_kernel(Args a, int pack_blocks) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < pack_blocks) {
    const int idx = blockIdx.x * kThreads + tid;
    if (idx < a.V1p * a.Jp) {
      const int k = idx / a.Jp, j = idx % a.Jp;
      a.wp[idx] = (k < a.V1 && j < a.J) ? a.w[(int64_t)k * a.J + j] : 0.f;
    }
    return;
  }
  const int b = blockIdx.x - pack_blocks;
  const int Tb = a.flens[b], Ub = a.llens[b];
  int st = 0;
  if (Tb < 1 || Tb > a.T || Ub < 0 || Ub > a.U) {
    st = LR_RNNT_BAD_LENGTH;
  } else {
    int bad = 0;
    for (int u = tid; u < Ub; u += kThreads) {
      const int y = a.labels[b * a.l_sb + u];
      if (y <= 0 || y >= a.V1 || a.mask[y] == 0.f) bad = 1;
    }
    if (__syncthreads_or(bad)) st = LR_RNNT_BAD_ID;
  }
  if (tid == 0) a.sstat[b] = st;
}

// ---- the joint stage of one tile: Z and the masked logits into LDS ---------------------------------------------------
__device__ __forceinline__ void joint_tile(const Args& a, int b, int t, int u0, float* Z, float* L) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ZS = a.Jp + 4, LS = a.V1p + 4;
  const float* er = a.e + b * a.e_sb + t * a.e_st;
  const float* pb = a.p + (int64_t)b * a.U1 * a.J;
  for (int idx = tid; idx < kTile * a.Jp; idx += kThreads) {
    const int n = idx / a.Jp, j = idx % a.Jp, u = u0 + n;
    float z = 0.f;
    if (j < a.J && u <= a.U) z = tanhf(er[j] + pb[(int64_t)u * a.J + j]);
    Z[n * ZS + j] = z;
  }
  __syncthreads();
  const int r32 = lane & 31, h = lane >> 5;
  for (int ct = wave; ct < a.V1p / 32; ct += 4) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* zr = Z + r32 * ZS + 4 * h;
    const float* wr = a.wp + (int64_t)(ct * 32 + r32) * a.Jp + 4 * h;
    // lane half h contracts k = k8 + 4h .. k8 + 4h + 3 of every group of 8: both operands from the same k
    for (int k8 = 0; k8 < a.Jp; k8 += 8) {
      const f32x4 av = *(const f32x4*)(zr + k8);
      const f32x4 bv = *(const f32x4*)(wr + k8);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], bv[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], bv[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], bv[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], bv[3], acc, 0, 0, 0);
    }
    const int cls = ct * 32 + r32;
    const bool live = cls < a.V1 && a.mask[cls < a.V1 ? cls : 0] != 0.f;
    const float bi = cls < a.V1 ? a.bias[cls] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      L[row * LS + cls] = live ? acc[r] + bi : LR_NEG_INF;
    }
  }
  __syncthreads();
}

// ---- launch 2 of the forward: one tile per workgroup -> log p(blank), log p(next label), log-sum-exp per node ----------
__global__ void __launch_bounds__(kThreads) rnnt_joint_kernel(Args a) {
  extern __shared__ float lds[];
  float* Z = lds;
  float* L = lds + kTile * (a.Jp + 4);
  const int ub = blockIdx.x, t = blockIdx.y, b = blockIdx.z;
  if (a.sstat[b] != 0) return;
  const int Tb = a.flens[b], Ub = a.llens[b], u0 = ub * kTile;
  if (t >= Tb || u0 > Ub) return;
  joint_tile(a, b, t, u0, Z, L);
  const int tid = threadIdx.x, n = tid >> 3, part = tid & 7, LS = a.V1p + 4;
  const float* row = L + n * LS;
  float m = LR_NEG_INF;
  for (int k = part; k < a.V1; k += 8) m = fmaxf(m, row[k]);
  for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.f;
  for (int k = part; k < a.V1; k += 8) s += expf(row[k] - m);
  for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o, 64);
  const int u = u0 + n;
  if (part == 0 && u <= Ub) {
    const float lse = m + logf(s);
    const int64_t at = ((int64_t)b * a.T + t) * a.U1 + u;
    a.lse[at] = lse;
    a.lpb[at] = row[0] - lse;
    a.lpl[at] = u < Ub ? row[a.labels[b * a.l_sb + u]] - lse : LR_NEG_INF;
  }
}

__device__ __forceinline__ double lse2d(double a, double b) {
  double m = fmax(a, b);
  if (m == (double)LR_NEG_INF) return m;
  return m + log(exp(a - m) + exp(b - m));
}

// ---- alpha (forward launch 3) / beta (backward launch 1): anti-diagonals, one workgroup per sample ---------------------
template <bool BETA>
__global__ void __launch_bounds__(kThreads) rnnt_lattice_kernel(Args a) {
  __shared__ double diag[2][LR_RNNT_MAX_U + 2];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.sstat[b] != 0) {
    if (!BETA && tid == 0) a.nll[b] = 0.f;
    return;
  }
  const int Tb = a.flens[b], Ub = a.llens[b];
  const int64_t base = (int64_t)b * a.T * a.U1;
  const float* lpb = a.lpb + base;
  const float* lpl = a.lpl + base;
  double* out = (BETA ? a.beta : a.alpha) + base;
  const int last = Tb - 1 + Ub;
  // the two transition terms of node (d - u, u): they do not depend on the recursion, so those of the next diagonal
  // are fetched before this one's barrier
  auto terms = [&](int d, int u, float& x, float& y) {
    const int t = d - u;
    x = LR_NEG_INF; y = LR_NEG_INF;
    if (d < 0 || d > last || u > Ub || u > d || t >= Tb) return;
    if (!BETA) {
      if (t > 0) x = lpb[(int64_t)(t - 1) * a.U1 + u];
      if (u > 0) y = lpl[(int64_t)t * a.U1 + u - 1];
    } else {
      if (t + 1 < Tb || u == Ub) x = lpb[(int64_t)t * a.U1 + u];
      if (u < Ub) y = lpl[(int64_t)t * a.U1 + u];
    }
  };
  int cur = 0;
  float nx, ny;
  terms(BETA ? last : 0, tid, nx, ny);
  for (int i = 0; i <= last; ++i) {
    const int d = BETA ? last - i : i;
    const double* prev = diag[cur ^ 1];
    double* now = diag[cur];
    float x0 = nx, y0 = ny;
    terms(BETA ? d - 1 : d + 1, tid, nx, ny);
    for (int u = tid; u <= Ub && u <= d; u += kThreads) {
      const int t = d - u;
      if (t >= Tb) continue;
      float x, y;
      if (u == tid) { x = x0; y = y0; } else terms(d, u, x, y);
      double v;
      if (!BETA) {
        if (d == 0) {
          v = 0.0;
        } else {
          const double ax = t > 0 ? prev[u] + (double)x : (double)LR_NEG_INF;
          const double ay = u > 0 ? prev[u - 1] + (double)y : (double)LR_NEG_INF;
          v = lse2d(ax, ay);
        }
        if (d == last) {
          const double lz = v + (double)lpb[(int64_t)t * a.U1 + u];
          a.logz[b] = lz;
          a.nll[b] = (float)-lz;
        }
      } else {
        if (d == last) {
          v = x;
        } else {
          const double bx = t + 1 < Tb ? prev[u] + (double)x : (double)LR_NEG_INF;
          const double by = u < Ub ? prev[u + 1] + (double)y : (double)LR_NEG_INF;
          v = lse2d(bx, by);
        }
      }
      now[u] = v;
      out[(int64_t)t * a.U1 + u] = v;
    }
    lr_lds_barrier();
    cur ^= 1;
  }
}

// ---- forward launch 4: the batch reduction, in a fixed order ----------------------------------------------------------
__global__ void __launch_bounds__(kThreads) rnnt_reduce_kernel(Args a) {
  __shared__ float part[kThreads];
  __shared__ int used[kThreads];
  const int tid = threadIdx.x;
  float s = 0.f;
  int n = 0;
  for (int b = tid; b < a.B; b += kThreads)
    if (a.sstat[b] == 0) { s += a.nll[b]; ++n; }
  part[tid] = s; used[tid] = n;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) { part[tid] += part[tid + o]; used[tid] += used[tid + o]; }
    __syncthreads();
  }
  const int nu = used[0];
  const float w = a.reduction == LR_CTC_MEAN ? 1.f / (float)(nu > 0 ? nu : 1) : 1.f;
  if (tid == 0) {
    a.loss[0] = part[0] * w;
    a.bstat[0] = nu == 0 ? 1 : 0;
  }
  for (int b = tid; b < a.B; b += kThreads) a.gw[b] = a.sstat[b] == 0 ? w : 0.f;
}

// ---- backward launch 2: workgroup (u block, frame chunk, sample) walks its frames ----------------------------------------
__global__ void __launch_bounds__(kThreads) rnnt_grad_kernel(Args a) {
  extern __shared__ float lds[];
  float* Z = lds;
  float* G = lds + kTile * (a.Jp + 4);
  const int ub = blockIdx.x, ts = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, h = lane >> 5;
  const int ZS = a.Jp + 4, LS = a.V1p + 4, njt = a.Jp / 32, nct = a.V1p / 32;
  const int64_t wg = ((int64_t)b * a.TS + ts) * a.UB + ub;
  float* dw = a.dw_s + wg * a.V1p * a.Jp;
  const int u0 = ub * kTile;
  const bool good = a.sstat[b] == 0;
  const int Tb = good ? a.flens[b] : 0, Ub = good ? a.llens[b] : 0;
  const float gs = good ? a.gw[b] * (a.gscale ? a.gscale[0] : 1.f) : 0.f;
  const double logZ = good ? a.logz[b] : 0.0;
  const int64_t base = (int64_t)b * a.T * a.U1;
  f32x16 dp_acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dp_acc[i][r] = 0.f;
  float db_acc = 0.f;
  bool first = true;
  const int t1 = min(a.T, (ts + 1) * a.tchunk);
  for (int t = ts * a.tchunk; t < t1; ++t) {
    float* de = a.de_s + (((int64_t)ub * a.B + b) * a.T + t) * a.Jp;
    if (!good || t >= Tb || u0 > Ub) {
      for (int j = tid; j < a.Jp; j += kThreads) de[j] = 0.f;
      continue;
    }
    joint_tile(a, b, t, u0, Z, G);
    {  // logits -> gradient at the logits, in place
      const int n = tid >> 3, part = tid & 7, u = u0 + n;
      float* row = G + n * LS;
      float ob = 0.f, ol = 0.f, lse = 0.f;
      int y = -1;
      if (u <= Ub) {
        const int64_t at = base + (int64_t)t * a.U1 + u;
        const double al = a.alpha[at];
        lse = a.lse[at];
        if (t + 1 < Tb) ob = expf((float)(al + (double)a.lpb[at] + a.beta[at + a.U1] - logZ));
        else if (u == Ub) ob = expf((float)(al + (double)a.lpb[at] - logZ));
        if (u < Ub) {
          ol = expf((float)(al + (double)a.lpl[at] + a.beta[at + 1] - logZ));
          y = a.labels[b * a.l_sb + u];
        }
      }
      const float on = ob + ol;
      for (int k = part; k < a.V1p; k += 8) {
        float g = 0.f;
        if (u <= Ub) {
          g = on * expf(row[k] - lse);
          if (k == 0) g -= ob;
          if (k == y) g -= ol;
          g *= gs;
        }
        row[k] = g;
      }
    }
    __syncthreads();
    if (tid < a.V1p) {
      float s = 0.f;
      for (int n = 0; n < kTile; ++n) s += G[n * LS + tid];
      db_acc += s;
    }
    // dZ = G . W, then the pre-activation gradient: rows are the tile's u, columns j
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int jt = wave + 4 * i;
      if (jt < njt) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float* gr = G + r32 * LS + 4 * h;
        const float* wc = a.wp + jt * 32 + r32;
        for (int k8 = 0; k8 < a.V1p; k8 += 8) {
          const f32x4 av = *(const f32x4*)(gr + k8);
          const float* wk = wc + (int64_t)(k8 + 4 * h) * a.Jp;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], wk[0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], wk[a.Jp], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], wk[2 * a.Jp], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], wk[3 * a.Jp], acc, 0, 0, 0);
        }
        const int j = jt * 32 + r32;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
          const float z = Z[row * ZS + j];
          const float dpre = acc[r] * (1.f - z * z);
          dp_acc[i][r] += dpre;
          s += dpre;
        }
        s += __shfl_xor(s, 32, 64);
        if (h == 0) de[j] = s;
      }
    }
    // dW += G^T . Z: the workgroup's own slab, the same lane reads back what it wrote a frame earlier
    for (int tl = wave; tl < nct * njt; tl += 4) {
      const int ct = tl / njt, jt = tl % njt;
      float* slab = dw + (int64_t)(ct * 32) * a.Jp + jt * 32 + r32;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        acc[r] = first ? 0.f : slab[(int64_t)row * a.Jp];
      }
      const float* gc = G + ct * 32 + r32;
      const float* zc = Z + jt * 32 + r32;
#pragma unroll
      for (int n2 = 0; n2 < kTile; n2 += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(gc[(n2 + h) * LS], zc[(n2 + h) * ZS], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        slab[(int64_t)row * a.Jp] = acc[r];
      }
    }
    first = false;
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int jt = wave + 4 * i;
    if (jt < njt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int u = u0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (u <= a.U) a.dp_s[(((int64_t)ts * a.B + b) * a.U1 + u) * a.Jp + jt * 32 + r32] = dp_acc[i][r];
      }
    }
  }
  if (tid < a.V1p) a.db_s[wg * a.V1p + tid] = db_acc;
  if (first)
    for (int i = tid; i < a.V1p * a.Jp; i += kThreads) dw[i] = 0.f;
}

// ---- backward launch 3: the slabs added in slab order ------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) rnnt_combine_kernel(Args a) {
  const int64_t n_e = (int64_t)a.B * a.T * a.J, n_p = (int64_t)a.B * a.U1 * a.J, n_w = (int64_t)a.V1 * a.J;
  const int64_t nwg = (int64_t)a.B * a.TS * a.UB;
  int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_e) {
    const int64_t bt = i / a.J;
    const int j = (int)(i % a.J);
    float s = 0.f;
    for (int ub = 0; ub < a.UB; ++ub) s += a.de_s[((int64_t)ub * a.B * a.T + bt) * a.Jp + j];
    a.d_e[i] = s;
    return;
  }
  i -= n_e;
  if (i < n_p) {
    const int64_t bu = i / a.J;
    const int j = (int)(i % a.J);
    float s = 0.f;
    for (int ts = 0; ts < a.TS; ++ts) s += a.dp_s[((int64_t)ts * a.B * a.U1 + bu) * a.Jp + j];
    a.d_p[i] = s;
    return;
  }
  i -= n_p;
  if (i < n_w) {
    const int k = (int)(i / a.J), j = (int)(i % a.J);
    float s = 0.f;
    for (int64_t g = 0; g < nwg; ++g) s += a.dw_s[(g * a.V1p + k) * a.Jp + j];
    a.d_w[i] = a.accumulate ? a.d_w[i] + s : s;
    return;
  }
  i -= n_w;
  if (i < a.V1) {
    float s = 0.f;
    for (int64_t g = 0; g < nwg; ++g) s += a.db_s[g * a.V1p + i];
    a.d_b[i] = a.accumulate ? a.d_b[i] + s : s;
  }
}

// ---- the greedy decoder: one launch, one workgroup per sample ------------------------------------------------------------
struct GreedyArgs {
  const float* e; int64_t e_sb, e_st;
  const int32_t* sizes;
  const float* tables;       // [context][V1][J], the prediction bias folded into table 0
  const float* w; const float* bias; const float* mask;
  int32_t* state;            // [B][context] or NULL
  const int32_t* frame_base; // [B] or NULL
  int32_t* ids; int32_t* frames; float* logp; int32_t* out_lens; int32_t* forced;
  int B, T, V1, J, context, max_symbols, max_out;
};

__global__ void __launch_bounds__(kThreads) rnnt_greedy_kernel(GreedyArgs a) {
  __shared__ float z[LR_RNNT_MAX_JOINT];
  __shared__ float logit[LR_RNNT_MAX_CLASSES];
  __shared__ float s_logp;
  __shared__ int s_best;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int size = a.sizes ? a.sizes[b] : a.T;
  size = size < 0 ? 0 : (size > a.T ? a.T : size);
  int c0 = 0, c1 = 0, n_out = 0, n_forced = 0;
  if (a.state) {
    c0 = a.state[b * a.context];
    if (a.context == 2) c1 = a.state[b * a.context + 1];
    if (c0 < 0 || c0 >= a.V1) c0 = 0;
    if (c1 < 0 || c1 >= a.V1) c1 = 0;
    n_out = a.out_lens[b] < 0 ? 0 : a.out_lens[b];
    n_forced = a.forced[b] < 0 ? 0 : a.forced[b];
  }
  const int fbase = a.frame_base ? a.frame_base[b] : 0;
  for (int t = 0; t < size; ++t) {
    const float* er = a.e + b * a.e_sb + t * a.e_st;
    for (int s = 0; s < a.max_symbols; ++s) {
      const float* t0 = a.tables + (int64_t)c0 * a.J;
      const float* t1 = a.tables + ((int64_t)a.V1 + c1) * a.J;
      for (int j = tid; j < a.J; j += kThreads) {
        float v = er[j] + t0[j];
        if (a.context == 2) v += t1[j];
        z[j] = tanhf(v);
      }
      __syncthreads();
      for (int k = wave; k < a.V1; k += 4) {
        const float* wr = a.w + (int64_t)k * a.J;
        float acc = 0.f;
        for (int j = lane; j < a.J; j += 64) acc = fmaf(wr[j], z[j], acc);
        acc = lr_wave_sum(acc);
        if (lane == 0) logit[k] = a.mask[k] != 0.f ? acc + a.bias[k] : LR_NEG_INF;
      }
      __syncthreads();
      if (wave == 0) {
        float bv = LR_NEG_INF;
        int bk = a.V1;
        for (int k = lane; k < a.V1; k += 64) {   // ascending k: a later equal value does not replace an earlier one
          const float v = logit[k];
          if (v > bv || (v == bv && k < bk)) { bv = v; bk = k; }
        }
        for (int o = 32; o > 0; o >>= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int ok = __shfl_xor(bk, o, 64);
          if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
        }
        float se = 0.f;
        for (int k = lane; k < a.V1; k += 64) se += expf(logit[k] - bv);
        se = lr_wave_sum(se);
        if (lane == 0) {
          s_best = bk < a.V1 ? bk : 0;
          s_logp = -logf(se);
        }
      }
      __syncthreads();
      const int best = s_best;
      const float lp = s_logp;
      __syncthreads();
      if (best == 0) break;
      if (tid == 0 && n_out < a.max_out) {
        a.ids[(int64_t)b * a.max_out + n_out] = best;
        a.frames[(int64_t)b * a.max_out + n_out] = fbase + t;
        a.logp[(int64_t)b * a.max_out + n_out] = lp;
      }
      ++n_out;
      c1 = c0;
      c0 = best;
      if (s == a.max_symbols - 1) ++n_forced;
    }
  }
  if (tid == 0) {
    a.out_lens[b] = n_out;
    a.forced[b] = n_forced;
    if (a.state) {
      a.state[b * a.context] = c0;
      if (a.context == 2) a.state[b * a.context + 1] = c1;
    }
  }
}

int set_lds(const void* fn, size_t bytes) {
  if (bytes > LR_LDS_BUDGET &&
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return LR_ERR_LAUNCH;
  return LR_OK;
}

}  // namespace

extern "C" size_t lr_rnnt_workspace_bytes(int B, int T, int U, int V1, int J) {
  Plan p;
  if (make_plan(B, T, U, V1, J, &p) != LR_OK) return 0;
  return p.bytes;
}

extern "C" int lr_rnnt_loss_forward(const float* e, int64_t e_stride_b, int64_t e_stride_t, const float* p,
                                    const float* joint_w, const float* joint_b, const float* class_mask,
                                    const int32_t* labels, int64_t label_stride, const int32_t* frame_lens,
                                    const int32_t* label_lens, int reduction, float* nll, int32_t* sample_status,
                                    float* out_loss, int32_t* out_status, void* workspace, size_t workspace_bytes,
                                    int B, int T, int U, int V1, int J, lr_stream_t stream) {
  LR_CHECK_ARG(e && p && joint_w && joint_b && class_mask && frame_lens && label_lens && nll && sample_status &&
               out_loss && out_status && workspace);
  LR_CHECK_ARG(labels || U == 0);
  LR_CHECK_ARG(e_stride_b >= 0 && e_stride_t >= 0 && label_stride >= 0);
  LR_CHECK_ARG(reduction == LR_CTC_SUM || reduction == LR_CTC_MEAN);
  LR_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  Plan pl;
  int ok = make_plan(B, T, U, V1, J, &pl);
  if (ok != LR_OK) return ok;
  if (workspace_bytes < pl.bytes) return LR_ERR_WORKSPACE;
  Args a = {};
  fill_args(&a, pl, workspace);
  a.e = e; a.e_sb = e_stride_b; a.e_st = e_stride_t; a.p = p; a.w = joint_w; a.bias = joint_b; a.mask = class_mask;
  a.labels = labels; a.l_sb = label_stride; a.flens = frame_lens; a.llens = label_lens;
  a.nll = nll; a.sstat = sample_status; a.loss = out_loss; a.bstat = out_status; a.reduction = reduction;
  ok = set_lds((const void*)rnnt_joint_kernel, pl.lds);
  if (ok != LR_OK) return ok;
  const int pack_blocks = (pl.V1p * pl.Jp + kThreads - 1) / kThreads;
  LR_LAUNCH(rnnt_prep_kernel, dim3(pack_blocks + B), dim3(kThreads), 0, stream, a, pack_blocks);
  ok = lr_launch_status();
  if (ok != LR_OK) return ok;
  LR_LAUNCH(rnnt_joint_kernel, dim3(pl.UB, T, B), dim3(kThreads), pl.lds, stream, a);
  ok = lr_launch_status();
  if (ok != LR_OK) return ok;
  LR_LAUNCH(rnnt_lattice_kernel<false>, dim3(B), dim3(kThreads), 0, stream, a);
  ok = lr_launch_status();
  if (ok != LR_OK) return ok;
  LR_LAUNCH(rnnt_reduce_kernel, dim3(1), dim3(kThreads), 0, stream, a);
  return lr_launch_status();
}

extern "C" int lr_rnnt_loss_backward(const float* e, int64_t e_stride_b, int64_t e_stride_t, const float* p,
                                     const float* joint_w, const float* joint_b, const float* class_mask,
                                     const int32_t* labels, int64_t label_stride, const int32_t* frame_lens,
                                     const int32_t* label_lens, const float* nll, const int32_t* sample_status,
                                     const float* grad_scale, float* d_e, float* d_p, float* d_joint_w,
                                     float* d_joint_b, int accumulate, void* workspace, size_t workspace_bytes, int B,
                                     int T, int U, int V1, int J, lr_stream_t stream) {
  LR_CHECK_ARG(e && p && joint_w && joint_b && class_mask && frame_lens && label_lens && nll && sample_status && d_e &&
               d_p && d_joint_w && d_joint_b && workspace);
  LR_CHECK_ARG(labels || U == 0);
  LR_CHECK_ARG(e_stride_b >= 0 && e_stride_t >= 0 && label_stride >= 0);
  LR_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  Plan pl;
  int ok = make_plan(B, T, U, V1, J, &pl);
  if (ok != LR_OK) return ok;
  if (workspace_bytes < pl.bytes) return LR_ERR_WORKSPACE;
  Args a = {};
  fill_args(&a, pl, workspace);
  a.e = e; a.e_sb = e_stride_b; a.e_st = e_stride_t; a.p = p; a.w = joint_w; a.bias = joint_b; a.mask = class_mask;
  a.labels = labels; a.l_sb = label_stride; a.flens = frame_lens; a.llens = label_lens;
  a.nll = const_cast<float*>(nll); a.sstat = const_cast<int32_t*>(sample_status);
  a.gscale = grad_scale; a.d_e = d_e; a.d_p = d_p; a.d_w = d_joint_w; a.d_b = d_joint_b; a.accumulate = accumulate ? 1 : 0;
  ok = set_lds((const void*)rnnt_grad_kernel, pl.lds);
  if (ok != LR_OK) return ok;
  LR_LAUNCH(rnnt_lattice_kernel<true>, dim3(B), dim3(kThreads), 0, stream, a);
  ok = lr_launch_status();
  if (ok != LR_OK) return ok;
  LR_LAUNCH(rnnt_grad_kernel, dim3(pl.UB, pl.TS, B), dim3(kThreads), pl.lds, stream, a);
  ok = lr_launch_status();
  if (ok != LR_OK) return ok;
  const int64_t outs = (int64_t)B * T * J + (int64_t)B * pl.U1 * J + (int64_t)V1 * J + V1;
  LR_LAUNCH(rnnt_combine_kernel, dim3((unsigned)((outs + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a);
  return lr_launch_status();
}

extern "C" int lr_rnnt_greedy_decode(const float* e, int64_t e_stride_b, int64_t e_stride_t, const int32_t* sizes,
                                     const float* tables, const float* joint_w, const float* joint_b,
                                     const float* class_mask, int32_t* state, const int32_t* frame_base, int32_t* ids,
                                     int32_t* frames, float* logp, int32_t* out_lens, int32_t* forced, int B, int T,
                                     int V1, int J, int context, int max_symbols, int max_out, lr_stream_t stream) {
  LR_CHECK_ARG(e && tables && joint_w && joint_b && class_mask && ids && frames && logp && out_lens && forced);
  LR_CHECK_ARG(B >= 1 && T >= 1 && V1 >= 2 && J >= 1 && max_symbols >= 1 && max_out >= 1);
  LR_CHECK_ARG(e_stride_b >= 0 && e_stride_t >= 0);
  LR_CHECK_ARG(context == 1 || context == 2);
  if (B > 65535 || T > LR_RNNT_MAX_T || V1 > LR_RNNT_MAX_CLASSES || J > LR_RNNT_MAX_JOINT) return LR_ERR_UNSUPPORTED;
  GreedyArgs a;
  a.e = e; a.e_sb = e_stride_b; a.e_st = e_stride_t; a.sizes = sizes; a.tables = tables; a.w = joint_w; a.bias = joint_b;
  a.mask = class_mask; a.state = state; a.frame_base = frame_base; a.ids = ids; a.frames = frames; a.logp = logp;
  a.out_lens = out_lens; a.forced = forced; a.B = B; a.T = T; a.V1 = V1; a.J = J; a.context = context;
  a.max_symbols = max_symbols; a.max_out = max_out;
  LR_LAUNCH(rnnt_greedy_kernel, dim3(B), dim3(kThreads), 0, stream, a);
  return lr_launch_status();
}
