// lr_transducer_beam.hip — time-synchronous beam search over the transducer head (BUILD-DEFINED; include/lipreading_hip.h
// A6j).
//
// One workgroup per sample walks the sample's frames.  Inside a frame every hypothesis is (a ROOT: one entry of the beam
// the frame started with, a SUFFIX: the at most LR_RNNT_BEAM_MAX_SYMBOLS labels emitted in this frame, one byte each in a
// 64-bit word), so the sets A, C and F of the specification are small arrays in LDS and no label string moves before the
// frame's end.  A round stages tanh(e_t + table rows) of the live hypotheses as a [32][J] operand in LDS and multiplies it
// with joint_w^T on v_mfma_f32_32x32x2_f32 (the loss's tile; the zero-padded weight operand is read through L2), then a
// row's mask, log-sum-exp and candidate scores.  Both selections are ranks by counting: a candidate's place is the
// number of candidates that beat it (larger float64 score, or the same score and an earlier place in the specified
// order), first inside its row (only a row's first beam_width can reach the round's), then among the rows' survivors.
// F is merged by exact string comparison (root labels in LDS), added in insertion order in float64, and ranked the same
// way.  Nothing is atomic and every order is fixed: two runs give the same bits.
//
// The beam's labels live in LDS (one byte each, double buffered); its emission frames live in global memory, one buffer
// the state's own, the other in the workspace.
#include "lr_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 32;                 // hypotheses per round = the MFMA tile's rows
constexpr int kMagic = 0x314d4252;        // "RBM1"
constexpr int kHeaderInts = 8;            // magic, B, beam_width, max_out, context, status, 0, 0
constexpr size_t kLdsMax = 160 * 1024;

// byte offsets of the kernel's arrays in dynamic LDS
struct Lay {
  int z, l, mk, asc, fsc, fown, skey, bsc, asuf, fsuf, ai, fi, snk, blen, rowcnt, bsrc, ids, bytes;
};

__host__ __device__ inline Lay layout(int Jp, int V1p, int W, int NF, int max_out) {
  Lay y;
  int o = 0;
#define LR_TAKE(field, nbytes) do { y.field = o; o += ((nbytes) + 15) & ~15; } while (0)
  LR_TAKE(z, kRows * (Jp + 4) * 4);       // Z [32][Jp + 4] fp32
  LR_TAKE(l, kRows * (V1p + 4) * 4);      // logits, then log-probabilities [32][V1p + 4] fp32
  LR_TAKE(mk, V1p * 4);                   // the class mask
  LR_TAKE(asc, 2 * kRows * 8);            // A: scores (fp64), double buffered
  LR_TAKE(fsc, NF * 8);                   // F: scores (fp64; merged in place)
  LR_TAKE(fown, NF * 8);                  // F: each offer's own, unmerged score
  LR_TAKE(skey, kRows * W * 8);           // the rows' survivors: scores
  LR_TAKE(bsc, 2 * kRows * 8);            // the beam's scores, double buffered
  LR_TAKE(asuf, 2 * kRows * 8);           // A: suffixes
  LR_TAKE(fsuf, NF * 8);                  // F: suffixes
  LR_TAKE(ai, 5 * 2 * kRows * 4);         // A: root, suffix length, length, c0, c1
  LR_TAKE(fi, 5 * NF * 4);                // F: root, suffix length, length, first equal entry, frames' source
  LR_TAKE(snk, kRows * W * 4);            // the rows' survivors: (row << 8) | class
  LR_TAKE(blen, 2 * kRows * 4);           // the beam's lengths, double buffered
  LR_TAKE(rowcnt, kRows * 4);             // survivors per row
  LR_TAKE(bsrc, kRows * 4);               // the F entry a new beam slot is built from
  LR_TAKE(ids, 2 * W * max_out);          // the beam's labels, one byte each, double buffered
#undef LR_TAKE
  y.bytes = o;
  return y;
}

// ---- the sizes: host arithmetic only (exercised under a sanitizer by a stand-alone program) -----------------------------
int check_dims(int B, int V1, int J, int W, int S) {
  if (B < 1 || V1 < 2 || J < 1 || W < 1 || S < 1) return LR_ERR_INVALID_ARG;
  if (B > 65535 || V1 > LR_RNNT_MAX_CLASSES || J > LR_RNNT_MAX_JOINT || W > LR_RNNT_BEAM_MAX_WIDTH ||
      S > LR_RNNT_BEAM_MAX_SYMBOLS)
    return LR_ERR_UNSUPPORTED;
  return LR_OK;
}

size_t state_bytes(int B, int W, int max_out) {
  if (B < 1 || B > 65535 || W < 1 || W > LR_RNNT_BEAM_MAX_WIDTH || max_out < 1 || max_out > LR_RNNT_MAX_U) return 0;
  const size_t bw = (size_t)B * W;
  // header, scores (fp64), count, lens, ids, frames
  return kHeaderInts * 4 + bw * 8 + (size_t)B * 4 + bw * 4 + 2 * bw * max_out * 4;
}

size_t packed_w_bytes(int V1, int J) {
  const size_t V1p = (V1 + 31) / 32 * 32, Jp = (J + 31) / 32 * 32;
  return lr_align_up(V1p * Jp * 4, 16);
}

size_t workspace_bytes(int B, int V1, int J, int W, int S) {
  if (check_dims(B, V1, J, W, S) != LR_OK) return 0;
  return packed_w_bytes(V1, J) + (size_t)B * W * LR_RNNT_MAX_U * 4;   // the second frames buffer, any max_out
}

struct BeamArgs {
  const float* e; int64_t e_sb, e_st;
  const int32_t* sizes;
  const float* tables;       // [context][V1][J]
  const float* w;            // [V1][J]
  float* wp;                 // [V1p][Jp], zero padded (workspace)
  const float* bias; const float* mask;
  int32_t* state; int fresh;
  const int32_t* frame_base;
  int32_t *out_ids, *out_frames, *out_lens; float* out_scores; int32_t* out_count; int32_t* truncated;
  int32_t* wframes;          // [B][W][LR_RNNT_MAX_U] (workspace), used as [W][max_out] per sample
  int B, T, V1, J, V1p, Jp, context, W, S, nbest, max_out;
};

__global__ void __launch_bounds__(kThreads) rnnt_beam_pack_kernel(BeamArgs a) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx < a.V1p * a.Jp) {
    const int k = idx / a.Jp, j = idx % a.Jp;
    a.wp[idx] = (k < a.V1 && j < a.J) ? a.w[(int64_t)k * a.J + j] : 0.f;
  }
}

__device__ __forceinline__ double beam_lse2(double x, double y) {
  const double m = fmax(x, y);
  if (m == (double)LR_NEG_INF) return m;
  return m + log(exp(x - m) + exp(y - m));
}

// Are the label strings of two in-frame hypotheses (root, suffix) equal?  `len` is the whole length; ids the beam's labels.
__device__ __forceinline__ bool same_prefix(int ri, int ni, uint64_t si, int rj, int nj, uint64_t sj, int len,
                                            const unsigned char* ids, int MO) {
  if (ri == rj) return ni == nj && si == sj;
  if (ni == nj) return false;   // two roots of one length are different strings: the beam holds no string twice
  if (ni > nj) {                // make i the hypothesis with the longer root
    int t = ri; ri = rj; rj = t;
    t = ni; ni = nj; nj = t;
    const uint64_t u = si; si = sj; sj = u;
  }
  const int d = nj - ni, Lj = len - nj;   // the shorter root's length; the longer root's is Lj + d
  if ((d < 8 ? sj >> (8 * d) : (uint64_t)0) != si) return false;   // d == 8 only with ni == 0
  const unsigned char* pi = ids + ri * MO;
  const unsigned char* pj = ids + rj * MO;
  for (int q = 0; q < d; ++q)
    if (pi[Lj + q] != (unsigned char)(sj >> (8 * q))) return false;
  for (int q = Lj - 1; q >= 0; --q)   // beams differ near their ends: backwards
    if (pi[q] != pj[q]) return false;
  return true;
}

__global__ void __launch_bounds__(kThreads) rnnt_beam_kernel(BeamArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int W = a.W, S = a.S, MO = a.max_out, NF = (S + 1) * W;
  const Lay y = layout(a.Jp, a.V1p, W, NF, MO);
  float* Z = (float*)(smem + y.z);
  float* L = (float*)(smem + y.l);
  float* mk = (float*)(smem + y.mk);
  double* a_sc = (double*)(smem + y.asc);
  double* f_sc = (double*)(smem + y.fsc);
  double* f_own = (double*)(smem + y.fown);
  double* s_key = (double*)(smem + y.skey);
  double* b_sc = (double*)(smem + y.bsc);
  uint64_t* a_suf = (uint64_t*)(smem + y.asuf);
  uint64_t* f_suf = (uint64_t*)(smem + y.fsuf);
  int* a_root = (int*)(smem + y.ai);
  int* a_nsuf = a_root + 2 * kRows;
  int* a_len = a_nsuf + 2 * kRows;
  int* a_c0 = a_len + 2 * kRows;
  int* a_c1 = a_c0 + 2 * kRows;
  int* f_root = (int*)(smem + y.fi);
  int* f_nsuf = f_root + NF;
  int* f_len = f_nsuf + NF;
  int* f_canon = f_len + NF;
  int* f_src = f_canon + NF;
  int* s_nk = (int*)(smem + y.snk);
  int* b_len = (int*)(smem + y.blen);
  int* rowcnt = (int*)(smem + y.rowcnt);
  int* b_src = (int*)(smem + y.bsrc);
  unsigned char* ids = smem + y.ids;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ZS = a.Jp + 4, LS = a.V1p + 4;

  // the state's arrays
  int32_t* hdr = a.state;
  const size_t bw = (size_t)a.B * W;
  double* st_scores = (double*)(a.state + kHeaderInts) + (size_t)b * W;
  int32_t* st_count = a.state + kHeaderInts + 2 * bw + b;
  int32_t* st_lens = a.state + kHeaderInts + 2 * bw + a.B + (size_t)b * W;
  int32_t* st_ids = a.state + kHeaderInts + 2 * bw + a.B + bw + (size_t)b * W * MO;
  int32_t* st_frames = st_ids + bw * MO;

  bool ok = true;
  if (!a.fresh) ok = hdr[0] == kMagic && hdr[1] == a.B && hdr[2] == W && hdr[3] == MO && hdr[4] == a.context;
  if (b == 0 && tid == 0) {
    if (a.fresh) {
      hdr[0] = kMagic; hdr[1] = a.B; hdr[2] = W; hdr[3] = MO; hdr[4] = a.context; hdr[6] = 0; hdr[7] = 0;
    }
    hdr[5] = ok ? 0 : LR_RNNT_BEAM_BAD_STATE;
  }
  const int nbest = a.nbest;
  int32_t* o_ids = a.out_ids + (size_t)b * nbest * MO;
  int32_t* o_frames = a.out_frames + (size_t)b * nbest * MO;
  if (!ok) {   // a state of another geometry: nothing of it is read, the answer is empty
    for (int i = tid; i < nbest * MO; i += kThreads) { o_ids[i] = 0; o_frames[i] = 0; }
    for (int i = tid; i < nbest; i += kThreads) {
      a.out_lens[b * nbest + i] = 0;
      a.out_scores[b * nbest + i] = LR_NEG_INF;
    }
    if (tid == 0) a.out_count[b] = 0;
    return;
  }

  // zero the small integer arrays: a slot that a NaN score leaves unwritten then still holds indices in range
  for (int i = tid; i < 5 * 2 * kRows; i += kThreads) a_root[i] = 0;
  for (int i = tid; i < 5 * NF; i += kThreads) f_root[i] = 0;
  for (int i = tid; i < kRows * W; i += kThreads) s_nk[i] = 0;
  for (int i = tid; i < 2 * kRows; i += kThreads) { b_len[i] = 0; b_sc[i] = 0.0; }
  if (tid < kRows) { rowcnt[tid] = 0; b_src[tid] = 0; }
  for (int k = tid; k < a.V1p; k += kThreads) mk[k] = k < a.V1 ? a.mask[k] : 0.f;
  for (int i = tid; i < kRows * ZS; i += kThreads) Z[i] = 0.f;   // the padding columns stay zero for the whole call
  __syncthreads();
  int nvalid = 0;   // label classes that are not masked
  for (int k = 1; k < a.V1; ++k) nvalid += mk[k] != 0.f ? 1 : 0;

  int size = a.sizes ? a.sizes[b] : a.T;
  size = size < 0 ? 0 : (size > a.T ? a.T : size);
  const int fbase = a.frame_base ? a.frame_base[b] : 0;
  int nb = 1, bc = 0, trunc = 0;
  int32_t* fcur = st_frames;
  int32_t* falt = a.wframes + (size_t)b * W * LR_RNNT_MAX_U;
  if (!a.fresh) {
    nb = *st_count;
    nb = nb < 1 ? 1 : (nb > W ? W : nb);
    trunc = a.truncated[b] < 0 ? 0 : a.truncated[b];
    if (tid < nb) {
      const int len = st_lens[tid];
      b_len[tid] = len < 0 ? 0 : (len > MO ? MO : len);
      b_sc[tid] = st_scores[tid];
    }
    for (int i = tid; i < nb * MO; i += kThreads) {
      const int v = st_ids[i];
      ids[i] = (unsigned char)((v < 0 || v >= a.V1) ? 0 : v);
    }
  }
  __syncthreads();

  for (int t = 0; t < size; ++t) {
    const float* er = a.e + b * a.e_sb + t * a.e_st;
    const unsigned char* idc = ids + bc * W * MO;
    int ac = 0, nA = nb, nF = 0;
    if (tid < nb) {
      const int len = b_len[bc * kRows + tid];
      a_root[tid] = tid; a_nsuf[tid] = 0; a_suf[tid] = 0; a_len[tid] = len; a_sc[tid] = b_sc[bc * kRows + tid];
      a_c0[tid] = len > 0 ? idc[tid * MO + len - 1] : 0;
      a_c1[tid] = len > 1 ? idc[tid * MO + len - 2] : 0;
    }
    __syncthreads();
    for (int s = 0; s <= S && nA > 0; ++s) {
      const int ao = ac * kRows;
      // the operand: one row per hypothesis of A (rows below keep older, finite values: a row of the product depends on
      // its own row of Z alone, and only A's rows are read).  A thread owns columns; the table rows of four hypotheses
      // are fetched before the first tanh, so their latencies overlap
      for (int j = tid; j < a.J; j += kThreads) {
        const float ev = er[j];
        for (int n0 = 0; n0 < nA; n0 += 4) {
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int n = n0 + q < nA ? n0 + q : nA - 1;
            v[q] = ev + a.tables[(int64_t)a_c0[ao + n] * a.J + j];
            if (a.context == 2) v[q] += a.tables[((int64_t)a.V1 + a_c1[ao + n]) * a.J + j];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (n0 + q < nA) Z[(n0 + q) * ZS + j] = tanhf(v[q]);
        }
      }
      __syncthreads();
      {  // the logits, class tile by class tile (lr_transducer.hip joint_tile)
        const int r32 = lane & 31, h = lane >> 5;
        for (int ct = wave; ct < a.V1p / 32; ct += 4) {
          f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          const float* zr = Z + r32 * ZS + 4 * h;
          const float* wr = a.wp + (int64_t)(ct * 32 + r32) * a.Jp + 4 * h;
          // 32 k per step (Jp is a multiple of 32); the next step's weights are fetched before this step's products.
          // The products keep their k order, so the sum is joint_tile's, bit for bit
          f32x4 bn[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) bn[q] = *(const f32x4*)(wr + 8 * q);
          for (int k32 = 0; k32 < a.Jp; k32 += 32) {
            f32x4 bv[4], av[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) bv[q] = bn[q];
            if (k32 + 32 < a.Jp) {
#pragma unroll
              for (int q = 0; q < 4; ++q) bn[q] = *(const f32x4*)(wr + k32 + 32 + 8 * q);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) av[q] = *(const f32x4*)(zr + k32 + 8 * q);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][0], bv[q][0], acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][1], bv[q][1], acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][2], bv[q][2], acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][3], bv[q][3], acc, 0, 0, 0);
            }
          }
          const int cls = ct * 32 + r32;
          const bool live = cls < a.V1 && mk[cls] != 0.f;
          const float bi = cls < a.V1 ? a.bias[cls] : 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            L[row * LS + cls] = live ? acc[r] + bi : LR_NEG_INF;
          }
        }
      }
      __syncthreads();
      {  // logits -> log-probabilities, eight lanes per row
        const int n = tid >> 3, part = tid & 7;
        float* row = L + n * LS;
        float m = LR_NEG_INF;
        for (int k = part; k < a.V1; k += 8) m = fmaxf(m, row[k]);
        for (int o = 1; o < 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float se = 0.f;
        for (int k = part; k < a.V1; k += 8) se += expf(row[k] - m);
        for (int o = 1; o < 8; o <<= 1) se += __shfl_xor(se, o, 64);
        const float lse = m + logf(se);
        for (int k = part; k < a.V1; k += 8) row[k] -= lse;
      }
      __syncthreads();
      // the blank: one offer per hypothesis, in A's order
      if (tid < nA) {
        const int i = nF + tid;
        const double sc = a_sc[ao + tid] + (double)L[tid * LS];
        f_root[i] = a_root[ao + tid]; f_nsuf[i] = a_nsuf[ao + tid]; f_suf[i] = a_suf[ao + tid];
        f_len[i] = a_len[ao + tid];
        f_sc[i] = sc; f_own[i] = sc;
      }
      nF += nA;
      if (s == S) break;
      // the labels
      const int per_row = nvalid < W ? nvalid : W;
      int full = 0;
      for (int n = 0; n < nA; ++n) full += a_len[ao + n] >= MO ? 1 : 0;
      trunc += full;
      if (tid < kRows) rowcnt[tid] = (tid < nA && a_len[ao + tid] < MO) ? per_row : 0;
      for (int idx = tid; idx < nA * a.V1; idx += kThreads) {   // a candidate's place in its row
        const int n = idx / a.V1, k = idx - n * a.V1;
        if (k == 0 || mk[k] == 0.f || a_len[ao + n] >= MO) continue;
        const float* row = L + n * LS;
        const double base = a_sc[ao + n], key = base + (double)row[k];
        int rank = 0;
        for (int k2 = 1; k2 < a.V1; ++k2) {
          if (mk[k2] == 0.f) continue;
          const double key2 = base + (double)row[k2];
          rank += (key2 > key || (key2 == key && k2 < k)) ? 1 : 0;
        }
        if (rank < W) { s_key[n * W + rank] = key; s_nk[n * W + rank] = (n << 8) | k; }
      }
      __syncthreads();
      int total = 0;
      for (int n = 0; n < nA; ++n) total += rowcnt[n];
      const int an = (ac ^ 1) * kRows;
      for (int idx = tid; idx < nA * W; idx += kThreads) {   // a survivor's place in the round
        const int n = idx / W, r = idx - n * W;
        if (r >= rowcnt[n]) continue;
        const double key = s_key[idx];
        const int nk = s_nk[idx];
        int rank = 0;
        for (int n2 = 0; n2 < nA; ++n2) {
          const int c2 = rowcnt[n2];
          for (int r2 = 0; r2 < c2; ++r2) {
            const double key2 = s_key[n2 * W + r2];
            rank += (key2 > key || (key2 == key && s_nk[n2 * W + r2] < nk)) ? 1 : 0;
          }
        }
        if (rank < W) {
          const int src = ao + (nk >> 8), k = nk & 255, ns = a_nsuf[src];
          a_root[an + rank] = a_root[src];
          a_nsuf[an + rank] = ns + 1;
          a_suf[an + rank] = a_suf[src] | ((uint64_t)k << (8 * ns));
          a_len[an + rank] = a_len[src] + 1;
          a_sc[an + rank] = key;
          a_c0[an + rank] = k;
          a_c1[an + rank] = a_c0[src];
        }
      }
      nA = total < W ? total : W;
      ac ^= 1;
      __syncthreads();
    }
    __syncthreads();
    // F: the first entry with the same string
    for (int i = tid; i < nF; i += kThreads) {
      int canon = i;
      const int ri = f_root[i], ni = f_nsuf[i], len = f_len[i];
      const uint64_t si = f_suf[i];
      for (int j = 0; j < i; ++j) {
        if (f_len[j] != len) continue;
        if (same_prefix(ri, ni, si, f_root[j], f_nsuf[j], f_suf[j], len, idc, MO)) { canon = j; break; }
      }
      f_canon[i] = canon;
    }
    __syncthreads();
    // the merge: scores added in insertion order, the frames of the constituent with the largest own score
    for (int i = tid; i < nF; i += kThreads) {
      if (f_canon[i] != i) continue;
      double sc = f_own[i], own = sc;
      int src = i;
      for (int j = i + 1; j < nF; ++j) {
        if (f_canon[j] != i) continue;
        const double oj = f_own[j];
        sc = beam_lse2(sc, oj);
        if (oj > own) { own = oj; src = j; }
      }
      f_sc[i] = sc;
      f_src[i] = src;
    }
    __syncthreads();
    const int bn = bc ^ 1;
    int ncanon = 0;
    for (int j = 0; j < nF; ++j) ncanon += f_canon[j] == j ? 1 : 0;
    for (int i = tid; i < nF; i += kThreads) {   // an entry's place in the next beam
      if (f_canon[i] != i) continue;
      const double sc = f_sc[i];
      int rank = 0;
      for (int j = 0; j < nF; ++j) {
        if (f_canon[j] != j) continue;
        const double s2 = f_sc[j];
        rank += (s2 > sc || (s2 == sc && j < i)) ? 1 : 0;
      }
      if (rank < W) { b_src[rank] = f_src[i]; b_sc[bn * kRows + rank] = sc; b_len[bn * kRows + rank] = f_len[i]; }
    }
    const int nb_new = ncanon < W ? ncanon : W;
    __syncthreads();
    unsigned char* idn = ids + bn * W * MO;
    for (int idx = tid; idx < nb_new * MO; idx += kThreads) {   // the next beam's labels and frames
      const int i = idx / MO, pos = idx - i * MO;
      if (pos >= b_len[bn * kRows + i]) continue;
      const int src = b_src[i], r = f_root[src], Lr = f_len[src] - f_nsuf[src];
      if (pos < Lr) {
        idn[idx] = idc[r * MO + pos];
        falt[idx] = fcur[r * MO + pos];
      } else {
        idn[idx] = (unsigned char)(f_suf[src] >> (8 * (pos - Lr)));
        falt[idx] = fbase + t;
      }
    }
    { int32_t* sw = fcur; fcur = falt; falt = sw; }
    bc = bn;
    nb = nb_new;
    __syncthreads();
  }

  // the state, every word of the sample's share, and the answer
  const unsigned char* idc = ids + bc * W * MO;
  for (int idx = tid; idx < W * MO; idx += kThreads) {
    const int i = idx / MO, pos = idx - i * MO;
    const bool live = i < nb && pos < b_len[bc * kRows + i];
    const int id = live ? idc[idx] : 0, fr = live ? fcur[idx] : 0;
    st_ids[idx] = id;
    st_frames[idx] = fr;
    if (i < nbest) { o_ids[idx] = id; o_frames[idx] = fr; }
  }
  if (tid < W) {
    const bool live = tid < nb;
    st_lens[tid] = live ? b_len[bc * kRows + tid] : 0;
    st_scores[tid] = live ? b_sc[bc * kRows + tid] : 0.0;
    if (tid < nbest) {
      a.out_lens[b * nbest + tid] = live ? b_len[bc * kRows + tid] : 0;
      a.out_scores[b * nbest + tid] = live ? (float)b_sc[bc * kRows + tid] : LR_NEG_INF;
    }
  }
  if (tid == 0) {
    *st_count = nb;
    a.out_count[b] = nb < nbest ? nb : nbest;
    a.truncated[b] = trunc;
  }
}

}  // namespace

extern "C" size_t lr_rnnt_beam_state_bytes(int B, int beam_width, int max_out) {
  return state_bytes(B, beam_width, max_out);
}

extern "C" size_t lr_rnnt_beam_workspace_bytes(int B, int V1, int J, int beam_width, int max_symbols) {
  return workspace_bytes(B, V1, J, beam_width, max_symbols);
}

extern "C" int lr_rnnt_beam_decode(const float* e, int64_t e_stride_b, int64_t e_stride_t, const int32_t* sizes,
                                   const float* tables, const float* joint_w, const float* joint_b,
                                   const float* class_mask, void* state, size_t state_bytes_given, int fresh,
                                   const int32_t* frame_base, int32_t* out_ids, int32_t* out_frames,
                                   int32_t* out_lens, float* out_scores, int32_t* out_count, int32_t* truncated,
                                   void* workspace, size_t workspace_bytes_given, int B, int T, int V1, int J,
                                   int context, int beam_width, int max_symbols, int nbest, int max_out,
                                   lr_stream_t stream) {
  LR_CHECK_ARG(e && tables && joint_w && joint_b && class_mask && state && out_ids && out_frames && out_lens &&
               out_scores && out_count && truncated && workspace);
  LR_CHECK_ARG(T >= 1 && max_out >= 1 && e_stride_b >= 0 && e_stride_t >= 0);
  LR_CHECK_ARG(context == 1 || context == 2);
  int ok = check_dims(B, V1, J, beam_width, max_symbols);
  if (ok != LR_OK) return ok;
  if (T > LR_RNNT_MAX_T || max_out > LR_RNNT_MAX_U) return LR_ERR_UNSUPPORTED;
  LR_CHECK_ARG(nbest >= 1 && nbest <= beam_width);
  LR_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)state & 7) == 0);
  LR_CHECK_ARG(state_bytes_given == state_bytes(B, beam_width, max_out));   // a buffer of another geometry
  if (workspace_bytes_given < workspace_bytes(B, V1, J, beam_width, max_symbols)) return LR_ERR_WORKSPACE;
  BeamArgs a;
  a.e = e; a.e_sb = e_stride_b; a.e_st = e_stride_t; a.sizes = sizes; a.tables = tables; a.w = joint_w;
  a.wp = (float*)workspace; a.bias = joint_b; a.mask = class_mask; a.state = (int32_t*)state; a.fresh = fresh ? 1 : 0;
  a.frame_base = frame_base; a.out_ids = out_ids; a.out_frames = out_frames; a.out_lens = out_lens;
  a.out_scores = out_scores; a.out_count = out_count; a.truncated = truncated;
  a.wframes = (int32_t*)((char*)workspace + packed_w_bytes(V1, J));
  a.B = B; a.T = T; a.V1 = V1; a.J = J; a.V1p = (V1 + 31) / 32 * 32; a.Jp = (J + 31) / 32 * 32; a.context = context;
  a.W = beam_width; a.S = max_symbols; a.nbest = nbest; a.max_out = max_out;
  const Lay y = layout(a.Jp, a.V1p, beam_width, (max_symbols + 1) * beam_width, max_out);
  if ((size_t)y.bytes > kLdsMax) return LR_ERR_UNSUPPORTED;
  if ((size_t)y.bytes > LR_LDS_BUDGET &&
      hipFuncSetAttribute((const void*)rnnt_beam_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, y.bytes) !=
          hipSuccess)
    return LR_ERR_LAUNCH;
  LR_LAUNCH(rnnt_beam_pack_kernel, dim3((a.V1p * a.Jp + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, a);
  ok = lr_launch_status();
  if (ok != LR_OK) return ok;
  LR_LAUNCH(rnnt_beam_kernel, dim3(B), dim3(kThreads), y.bytes, stream, a);
  return lr_launch_status();
}
