// lr_tfm_stream.hip — resumable transformer encoder sessions: the chunk-limited encoder stack of lr_transformer.hip (and
// the CTC head) advanced chunk by chunk from a caller-owned state, on gfx950 (include/lipreading_hip.h lr_tfm_stream_*,
// DESIGN.md §31).
//
// Under the chunk mask (lr_attn_window) a frame of attention chunk c sees chunk c to its end and left_chunks whole chunks
// before it, at every layer.  So a chunk's outputs are final once its last frame is in (or the stream ends), and all a
// later chunk needs of the past is, per layer, the keys and values of the last left_chunks * chunk positions.  A session
// keeps exactly that: per slot the input frames of the chunk that is not whole yet (the PENDING frames, at most chunk - 1)
// and per layer a RING of keys | values.  It only ever computes whole chunks (a short one at the end), which is why the
// bits cannot depend on how the stream was cut:
//   * the row-wise halves (input projection, QKV, out-projection, feed-forward, head: rows_linear_kernel below;
//     LayerNorm: one wave per row) compute a row from that row alone, in an order fixed by the widths — the tile a row
//     falls into, the rows beside it and the number of rows change nothing.  lr_fgemm's F32 products have the same
//     property at a fixed split-K count, but their 128 x 128 tiles walk K alone: 14 - 55 us per product for the 4 - 31
//     rows of an advance (measured: 670 - 950 us per advance).  rows_linear_kernel works on 16 x 16 tiles with K split
//     over a workgroup's four waves (v_mfma_f32_16x16x4_f32, exact fp32 operands, lr_rnn_stream.hip's geometry);
//   * attention: one workgroup per (head, new chunk, slot) stages the window's keys and values — ring positions and this
//     advance's rows, which hold the same bits — into LDS in window order; one wave per query row: a lane's scores are
//     serial sums over the head dimension, the reductions over the keys are butterflies over lanes that are window
//     positions, the context is a serial sum over the window;
//   * one commit launch at the end appends the new keys | values to the rings (the latest position of every ring index),
//     rewrites the pending frames (zero past the pending count: the bytes do not remember the cut) and the headers.
// Every kernel derives a slot's plan (rows to compute, positions, status) from the header as the advance found it; only
// the commit launch writes the state.  No workgroup waits for another, no atomics, every store a plain vector store.
#include "lr_common.h"

namespace {

constexpr int32_t kMagic = 0x4c525446;
constexpr int kHdrWords = 16;
enum { HD_MAGIC = 0, HD_I, HD_DM, HD_NHEAD, HD_F, HD_LAYERS, HD_CHUNK, HD_LEFT, HD_FRAMES, HD_EMITTED, HD_ENDED, HD_STATUS };
constexpr int kMaxChunk = 32, kMaxWindow = 128, kMaxDh = 64, kMaxClasses = 4096, kMaxChunkT = 1 << 16;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Cfg {
  int I, Dm, nhead, F, nl, C, Lc;
};

bool cfg_ok(const Cfg& c, int B) {
  if (B < 1 || B > 65535 || c.I < 1 || c.Dm < 1 || c.nhead < 1 || c.F < 1 || c.nl < 1) return false;
  if (c.C < 1 || c.C > kMaxChunk || c.Lc < 0 || ((int64_t)c.Lc + 1) * c.C > kMaxWindow) return false;
  if (c.Dm % c.nhead != 0) return false;
  const int dh = c.Dm / c.nhead;
  if (dh % 4 != 0 || dh > kMaxDh) return false;
  return lr_tfm_reserve_bytes(0, 1, 1, c.I, c.Dm, c.nhead, c.F, c.nl) != 0;   // the stack's own limits (tfm_dims_ok)
}

struct StateLayout {
  size_t pend_off, ring_off, slot_bytes, total;   // bytes; a slot = header | pending [C - 1][I] | rings [nl][ringN][2 Dm]
  int ringN;
};
bool state_layout(const Cfg& c, int B, StateLayout* s) {
  if (!cfg_ok(c, B)) return false;
  s->ringN = c.Lc * c.C;
  s->pend_off = kHdrWords * sizeof(int32_t);
  s->ring_off = lr_align_up(s->pend_off + (size_t)(c.C - 1) * c.I * sizeof(float), 16);
  s->slot_bytes = lr_align_up(s->ring_off + (size_t)c.nl * s->ringN * 2 * c.Dm * sizeof(float), 256);
  s->total = s->slot_bytes * B;
  return true;
}

inline size_t al64(size_t n) { return (n + 63) / 64 * 64; }
struct WsLayout {   // float offsets
  size_t X, PE, hA, hB, qkv, a, s1, h1, f1, s2, stats, logits, total;
  int rows;
  int64_t R;
};
bool ws_layout(const Cfg& c, int B, int chunk_T, int Cv, WsLayout* w) {
  if (!cfg_ok(c, B) || chunk_T < 0 || chunk_T > kMaxChunkT || Cv < 0 || Cv > kMaxClasses) return false;
  w->rows = chunk_T + c.C - 1;
  const int64_t R = w->R = (int64_t)B * w->rows;
  if (R > (1 << 20) - 16 || (w->rows + c.C - 1) / c.C > 65535) return false;   // (grid extents)
  size_t p = 0;
  w->X = p; p += al64((size_t)R * c.I);
  w->PE = p; p += al64((size_t)R * c.Dm);
  w->hA = p; p += al64((size_t)R * c.Dm);
  w->hB = p; p += al64((size_t)R * c.Dm);
  w->qkv = p; p += (size_t)c.nl * al64((size_t)R * 3 * c.Dm);
  w->a = p; p += al64((size_t)R * c.Dm);
  w->s1 = p; p += al64((size_t)R * c.Dm);
  w->h1 = p; p += al64((size_t)R * c.Dm);
  w->f1 = p; p += al64((size_t)R * c.F);
  w->s2 = p; p += al64((size_t)R * c.Dm);
  w->stats = p; p += al64((size_t)2 * R);
  w->logits = p; p += al64((size_t)R * Cv);
  w->total = (p > 64 ? p : 64) * sizeof(float);
  return true;
}

// what an advance does to a slot, from the header as the advance found it
struct Plan {
  bool ok;        // the slot takes part: rows may be emitted, the header and the payload are rewritten
  int status;     // bits to set (the slot keeps its bytes)
  int n0, e0, pend, take, emit, ended;
};
struct AdvArgs {
  const int32_t* sizes;
  const int32_t* end;
  char* state;
  size_t slot_bytes, pend_off, ring_off;
  Cfg c;
  int ringN, rows, chunk_T, pe_rows, B;
};
__device__ __forceinline__ const int32_t* hdr_of(const AdvArgs& a, int b) {
  return reinterpret_cast<const int32_t*>(a.state + (size_t)b * a.slot_bytes);
}
__device__ __forceinline__ bool hdr_is(const int32_t* h, const Cfg& c) {
  return h[HD_MAGIC] == kMagic && h[HD_I] == c.I && h[HD_DM] == c.Dm && h[HD_NHEAD] == c.nhead && h[HD_F] == c.F &&
         h[HD_LAYERS] == c.nl && h[HD_CHUNK] == c.C && h[HD_LEFT] == c.Lc;
}
__device__ __forceinline__ Plan make_plan(const AdvArgs& a, int b) {
  Plan p;
  p.ok = false;
  p.status = 0;
  p.n0 = p.e0 = p.pend = p.emit = p.ended = 0;
  int take = a.sizes ? a.sizes[b] : a.chunk_T;
  take = take < 0 ? 0 : take > a.chunk_T ? a.chunk_T : take;
  p.take = take;
  const bool ending = a.end && a.end[b] != 0;
  if (take == 0 && !ending) return p;   // idle: every bit stays
  const int32_t* h = hdr_of(a, b);
  if (!hdr_is(h, a.c)) {
    p.status = LR_TFM_STREAM_MISMATCH;
    return p;
  }
  if (h[HD_ENDED]) {                    // (an end repeated without frames changes nothing)
    if (take > 0) p.status = LR_TFM_STREAM_AFTER_END;
    return p;
  }
  p.n0 = h[HD_FRAMES];
  if ((int64_t)p.n0 + take > a.pe_rows) {
    p.status = LR_TFM_STREAM_FULL;
    return p;
  }
  p.ok = true;
  p.e0 = p.n0 / a.c.C * a.c.C;
  p.pend = p.n0 - p.e0;
  const int n1 = p.n0 + take;
  p.emit = (ending ? n1 : n1 / a.c.C * a.c.C) - p.e0;
  p.ended = ending ? 1 : 0;
  return p;
}

// row r = b * rows + i of the advance: the slot's i-th new output row, position e0 + i.  X[r] = its input frame (the
// pending frames first, then x), PE[r] = pe[e0 + i]; zero rows past the slot's emit count.  One workgroup per row.
__global__ __launch_bounds__(256) void gather_kernel(const AdvArgs a, const float* __restrict__ x, int64_t stride_b,
                                                     int64_t stride_t, const float* __restrict__ pe,
                                                     float* __restrict__ X, float* __restrict__ PE) {
  const int r = blockIdx.x, b = r / a.rows, i = r - b * a.rows;
  const Plan p = make_plan(a, b);
  const bool valid = p.ok && i < p.emit;
  const int I = a.c.I, Dm = a.c.Dm;
  const float* src = nullptr;
  if (valid)
    src = i < p.pend ? reinterpret_cast<const float*>(a.state + (size_t)b * a.slot_bytes + a.pend_off) + (size_t)i * I
                     : x + (int64_t)b * stride_b + (int64_t)(i - p.pend) * stride_t;
  for (int k = threadIdx.x; k < I; k += 256) X[(int64_t)r * I + k] = valid ? src[k] : 0.f;
  const float* per = pe + (int64_t)(p.e0 + i) * Dm;
  for (int d = threadIdx.x; d < Dm; d += 256) PE[(int64_t)r * Dm + d] = valid ? per[d] : 0.f;
}

// a lane's float4 of an operand row: row[k .. k + 3], zero at k >= lim; one load where the row allows it
__device__ __forceinline__ float4 ld4(const float* __restrict__ row, int k, int lim, bool vec) {
  if (vec && k + 3 < lim) return *reinterpret_cast<const float4*>(row + k);
  float4 v;
  v.x = k < lim ? row[k] : 0.f;
  v.y = k + 1 < lim ? row[k + 1] : 0.f;
  v.z = k + 2 < lim ? row[k + 2] : 0.f;
  v.w = k + 3 < lim ? row[k + 3] : 0.f;
  return v;
}

// y[r][n] = act(sum_k a[r][k] w[n][k] + bias[n] + addend[r][n]) for the few rows of an advance: grid (ceil(N / 16),
// ceil(R / 16)), a workgroup owns a 16 x 16 tile, its four waves split K — wave v takes the 16-k groups g = v, v + 4, ...
// in rising order, the four partial tiles are added in wave order.  A row's sum is fixed by K alone.
__global__ __launch_bounds__(256) void rows_linear_kernel(const float* __restrict__ a, int lda, int vec_a,
                                                          const float* __restrict__ w, int vec_w,
                                                          const float* __restrict__ bias,
                                                          const float* __restrict__ addend, int ldadd,
                                                          float* __restrict__ y, int ldy, int R, int N, int K, int relu) {
  __shared__ float red[4][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const bool a_in = r0 + row < R, w_in = n0 + row < N;
  const float* arow = a + (int64_t)(a_in ? r0 + row : 0) * lda;
  const float* wrow = w + (int64_t)(w_in ? n0 + row : 0) * K;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int g = wave; g * 16 < K; g += 4) {
    const int k = g * 16 + 4 * kq;
    const float4 av = a_in ? ld4(arow, k, K, vec_a != 0) : zero4;
    const float4 wv = w_in ? ld4(wrow, k, K, vec_w != 0) : zero4;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wv.w, acc, 0, 0, 0);
  }
  // C/D layout of 16x16x4: col = lane & 15, row = (lane >> 4) * 4 + i
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][kq * 4 + i][row] = acc[i];
  __syncthreads();
  const int rl = tid >> 4, cl = tid & 15, r = r0 + rl, n = n0 + cl;
  if (r >= R || n >= N) return;
  float out = ((red[0][rl][cl] + red[1][rl][cl]) + red[2][rl][cl]) + red[3][rl][cl];
  out += bias[n];
  if (addend) out += addend[(int64_t)r * ldadd + n];
  if (relu) out = fmaxf(out, 0.f);
  y[(int64_t)r * ldy + n] = out;
}

// Cached attention of one layer: workgroup (head, j, b) = the j-th new chunk of slot b, rows [j C, (j + 1) C) of the
// slot's rows.  qkv [R][3 Dm] are this advance's rows of the layer, a [R][Dm] receives the context (zero rows where the
// slot emits nothing).  LDS: Ks | Vs [Wmax][dh + 1] (the pitch keeps lanes = keys off one bank), Pw [4 waves][Wmax].
__global__ __launch_bounds__(256) void attn_kernel(const AdvArgs a, const float* __restrict__ qkv, float* __restrict__ ctx,
                                                   int layer, float scale) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int head = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.c.C, Dm = a.c.Dm, dh = Dm / a.c.nhead, pitch = dh + 1, Wmax = (a.c.Lc + 1) * C;
  float* Ks = lds;
  float* Vs = Ks + (size_t)Wmax * pitch;
  float* Pw = Vs + (size_t)Wmax * pitch;
  const Plan p = make_plan(a, b);
  const int i0 = j * C, i1 = min(i0 + C, a.rows);
  int nvalid = p.ok ? p.emit - i0 : 0;
  nvalid = nvalid < 0 ? 0 : nvalid > i1 - i0 ? i1 - i0 : nvalid;
  const int64_t r0 = (int64_t)b * a.rows;
  for (int idx = tid; idx < (i1 - i0 - nvalid) * dh; idx += 256)
    ctx[(r0 + i0 + nvalid + idx / dh) * Dm + head * dh + idx % dh] = 0.f;
  if (nvalid == 0) return;   // workgroup-uniform
  // the chunk's window: positions [lo, hi); those below e0 come from the ring, the others are rows of this advance
  const int c = p.e0 / C + j;
  const int lo = (c > a.c.Lc ? c - a.c.Lc : 0) * C, hi = p.e0 + i0 + nvalid, W = hi - lo;
  const float* ring = reinterpret_cast<const float*>(a.state + (size_t)b * a.slot_bytes + a.ring_off) +
                      (size_t)layer * a.ringN * 2 * Dm;
  // (four floats per load: the head's slice of a row starts 16-byte aligned — dh % 4 == 0, Dm % 4 == 0)
  const int dq = dh >> 2;
#pragma unroll 4
  for (int idx = tid; idx < W * dq; idx += 256) {
    const int kk = idx / dq, d = 4 * (idx - kk * dq), pos = lo + kk;
    const float* src = pos >= p.e0 ? qkv + (r0 + (pos - p.e0)) * 3 * Dm + Dm : ring + (size_t)(pos % a.ringN) * 2 * Dm;
    const float4 kv = *reinterpret_cast<const float4*>(src + head * dh + d);
    const float4 vv = *reinterpret_cast<const float4*>(src + Dm + head * dh + d);
    float* kd = Ks + kk * pitch + d;
    float* vd = Vs + kk * pitch + d;
    kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
    vd[0] = vv.x; vd[1] = vv.y; vd[2] = vv.z; vd[3] = vv.w;
  }
  __syncthreads();
  float* mine = Pw + wave * Wmax;
  for (int q0 = 0; q0 < nvalid; q0 += 4) {   // (the same trip count in every wave: the barriers below are uniform)
    const int qi = q0 + wave;
    const bool active = qi < nvalid;
    const int64_t r = r0 + i0 + (active ? qi : 0);
    if (active) {
      const float qv = lane < dh ? qkv[r * 3 * Dm + head * dh + lane] : 0.f;
      const int k0 = min(lane, W - 1), k1 = min(lane + 64, W - 1);
      float s0 = 0.f, s1 = 0.f;
      for (int d = 0; d < dh; ++d) {
        const float qd = __shfl(qv, d, 64);
        s0 += qd * Ks[k0 * pitch + d];
        s1 += qd * Ks[k1 * pitch + d];
      }
      s0 = lane < W ? s0 * scale : LR_NEG_INF;
      s1 = lane + 64 < W ? s1 * scale : LR_NEG_INF;
      const float m = lr_wave_max(fmaxf(s0, s1));   // W >= 1: finite
      const float e0 = lane < W ? expf(s0 - m) : 0.f, e1 = lane + 64 < W ? expf(s1 - m) : 0.f;
      const float z = lr_wave_sum(e0 + e1);
      if (lane < W) mine[lane] = e0 / z;
      if (lane + 64 < W) mine[lane + 64] = e1 / z;
    }
    __syncthreads();
    if (active && lane < dh) {
      float acc = 0.f;
      for (int k = 0; k < W; ++k) acc += mine[k] * Vs[k * pitch + lane];
      ctx[r * Dm + head * dh + lane] = acc;
    }
    __syncthreads();
  }
}

// h_out[r] = the last layer's row (zeros past the slot's emit count); log_probs[r] = log_softmax(logits[r] + log(mask +
// 1e-45)), past the emit count the head of the zero row (logits = the bias).  One wave per row.
__global__ __launch_bounds__(256) void finish_kernel(const AdvArgs a, const float* __restrict__ h,
                                                     const float* __restrict__ logits, const float* __restrict__ bias,
                                                     const float* __restrict__ mask, float* __restrict__ h_out,
                                                     float* __restrict__ log_probs, int64_t R, int Cv) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= R) return;
  const int b = (int)(r / a.rows), i = (int)(r - (int64_t)b * a.rows);
  const Plan p = make_plan(a, b);
  const bool valid = p.ok && i < p.emit;
  const int Dm = a.c.Dm;
  if (h_out)
    for (int d = lane; d < Dm; d += 64) h_out[r * Dm + d] = valid ? h[r * Dm + d] : 0.f;
  if (!log_probs) return;
  float m = LR_NEG_INF;
  for (int c = lane; c < Cv; c += 64) m = fmaxf(m, (valid ? logits[r * Cv + c] : bias[c]) + logf(mask[c] + 1e-45f));
  m = lr_wave_max(m);
  float z = 0.f;
  for (int c = lane; c < Cv; c += 64) z += expf((valid ? logits[r * Cv + c] : bias[c]) + logf(mask[c] + 1e-45f) - m);
  const float lse = m + logf(lr_wave_sum(z));
  for (int c = lane; c < Cv; c += 64)
    log_probs[r * Cv + c] = (valid ? logits[r * Cv + c] : bias[c]) + logf(mask[c] + 1e-45f) - lse;
}

// The one launch that writes the state: workgroup b = slot b.  Rings: index q receives the latest new position p with
// p % ringN == q.  Pending: the frames [E(after), n after), zeros behind them.  Header: counters, ended, status.
__global__ __launch_bounds__(256) void commit_kernel(const AdvArgs a, const float* __restrict__ x, int64_t stride_b,
                                                     int64_t stride_t, const float* __restrict__ qkv, size_t qkv_layer,
                                                     int32_t* __restrict__ counts) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const Plan p = make_plan(a, b);
  __syncthreads();   // every thread has read the header
  char* slot = a.state + (size_t)b * a.slot_bytes;
  int32_t* h = reinterpret_cast<int32_t*>(slot);
  if (!p.ok) {
    if (tid == 0) {
      counts[b] = 0;
      if (p.status) h[HD_STATUS] |= p.status;
    }
    return;
  }
  const int C = a.c.C, I = a.c.I, Dm = a.c.Dm;
  const int e1 = p.e0 + p.emit, n1 = p.n0 + p.take, npend = n1 - e1;
  float* pend = reinterpret_cast<float*>(slot + a.pend_off);
  for (int idx = tid; idx < (C - 1) * I; idx += 256) {
    const int jj = idx / I, k = idx - jj * I, pos = e1 + jj;
    float v = 0.f;
    if (jj < npend) v = pos < p.n0 ? pend[idx] : x[(int64_t)b * stride_b + (int64_t)(pos - p.n0) * stride_t + k];
    pend[idx] = v;   // (pos < n0 only with emit == 0, where pos - e0 == jj: the element itself)
  }
  if (p.emit > 0 && a.ringN > 0) {
    float* ring = reinterpret_cast<float*>(slot + a.ring_off);
    const int pmax = e1 - 1, D2 = 2 * Dm;
    const int64_t per_layer = (int64_t)a.ringN * D2, total = per_layer * a.c.nl;
    for (int64_t idx = tid; idx < total; idx += 256) {
      const int l = (int)(idx / per_layer);
      const int rem = (int)(idx - (int64_t)l * per_layer), q = rem / D2, d = rem - q * D2;
      if (pmax < q) continue;
      const int pos = pmax - (pmax - q) % a.ringN;
      if (pos < p.e0) continue;
      ring[idx] = qkv[(size_t)l * qkv_layer + ((int64_t)b * a.rows + (pos - p.e0)) * 3 * Dm + Dm + d];
    }
  }
  if (tid == 0) {
    h[HD_FRAMES] = n1;
    h[HD_EMITTED] += p.emit;
    h[HD_ENDED] = p.ended;
    counts[b] = p.emit;
  }
}

__global__ __launch_bounds__(256) void reset_kernel(char* state, size_t slot_bytes, const int32_t* __restrict__ mask,
                                                    const Cfg c) {
  const int b = blockIdx.x;
  if (mask && mask[b] == 0) return;
  int32_t* w = reinterpret_cast<int32_t*>(state + (size_t)b * slot_bytes);
  const int32_t hdr[kHdrWords] = {kMagic, c.I, c.Dm, c.nhead, c.F, c.nl, c.C, c.Lc, 0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t i = threadIdx.x; i < slot_bytes / 4; i += 256) w[i] = i < kHdrWords ? hdr[i] : 0;
}

__global__ void read_kernel(const char* __restrict__ state, size_t slot_bytes, const Cfg c, int B, int32_t* frames,
                            int32_t* emitted, int32_t* ended, int32_t* status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int32_t* h = reinterpret_cast<const int32_t*>(state + (size_t)b * slot_bytes);
  const bool ok = hdr_is(h, c);
  if (frames) frames[b] = ok ? h[HD_FRAMES] : 0;
  if (emitted) emitted[b] = ok ? h[HD_EMITTED] : 0;
  if (ended) ended[b] = ok ? h[HD_ENDED] : 0;
  if (status) status[b] = ok ? h[HD_STATUS] : (h[HD_MAGIC] == kMagic ? h[HD_STATUS] : 0) | LR_TFM_STREAM_MISMATCH;
}

#define LR_TRY_(expr)                   \
  do {                                  \
    const int lr_st_ = (expr);          \
    if (lr_st_ != LR_OK) return lr_st_; \
  } while (0)

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// y [R][N] = act(a [R][K] . w [N][K]^T + bias + addend [R][N])
int rows_linear(const float* a, const float* w, const float* bias, const float* addend, float* y, int R, int N, int K,
                int relu, hipStream_t st) {
  const int vec_a = K % 4 == 0 && aligned16(a), vec_w = K % 4 == 0 && aligned16(w);
  LR_LAUNCH(rows_linear_kernel, dim3((N + 15) / 16, (R + 15) / 16), dim3(256), 0, st, a, K, vec_a, w, vec_w, bias, addend, N,
            y, N, R, N, K, relu);
  return lr_launch_status();
}

}  // namespace

extern "C" size_t lr_tfm_stream_state_bytes(int B, int I, int Dm, int nhead, int F, int nlayers, int chunk,
                                            int left_chunks) {
  StateLayout s;
  return state_layout(Cfg{I, Dm, nhead, F, nlayers, chunk, left_chunks}, B, &s) ? s.total : 0;
}

extern "C" size_t lr_tfm_stream_workspace_bytes(int B, int chunk_T, int I, int Dm, int nhead, int F, int nlayers, int Cv,
                                                int chunk, int left_chunks) {
  WsLayout w;
  return ws_layout(Cfg{I, Dm, nhead, F, nlayers, chunk, left_chunks}, B, chunk_T, Cv, &w) ? w.total : 0;
}

extern "C" int lr_tfm_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int B, int I, int Dm, int nhead,
                                   int F, int nlayers, int chunk, int left_chunks, lr_stream_t stream) {
  LR_CHECK_ARG(state && aligned16(state));
  LR_CHECK_ARG(B >= 1 && I >= 1 && Dm >= 1 && nhead >= 1 && F >= 1 && nlayers >= 1 && chunk >= 1 && left_chunks >= 0);
  const Cfg c{I, Dm, nhead, F, nlayers, chunk, left_chunks};
  StateLayout s;
  if (!state_layout(c, B, &s)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total) return LR_ERR_WORKSPACE;
  LR_LAUNCH(reset_kernel, dim3(B), dim3(256), 0, stream, (char*)state, s.slot_bytes, mask, c);
  return lr_launch_status();
}

extern "C" int lr_tfm_stream_advance(const float* x, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                     const int32_t* end, const float* const* weights, const float* pe, int pe_rows,
                                     const float* head_w, const float* head_b, const float* head_mask, float* h_out,
                                     float* log_probs, int32_t* counts, void* state, size_t state_bytes, void* workspace,
                                     size_t workspace_bytes, int B, int chunk_T, int I, int Dm, int nhead, int F,
                                     int nlayers, int Cv, int chunk, int left_chunks, float eps, lr_stream_t stream_) {
  LR_CHECK_ARG(weights && pe && counts && state && workspace && (x || chunk_T == 0));
  LR_CHECK_ARG(B >= 1 && chunk_T >= 0 && I >= 1 && Dm >= 1 && nhead >= 1 && F >= 1 && nlayers >= 1 && Cv >= 0);
  LR_CHECK_ARG(chunk >= 1 && left_chunks >= 0 && pe_rows >= 1 && stride_b >= 0 && stride_t >= 0);
  LR_CHECK_ARG(aligned16(state) && aligned16(workspace) && (reinterpret_cast<uintptr_t>(x) & 3) == 0);
  const bool head = head_w || head_b || head_mask;
  if (head) LR_CHECK_ARG(head_w && head_b && head_mask && log_probs && Cv >= 1);
  else LR_CHECK_ARG(!log_probs);
  const Cfg c{I, Dm, nhead, F, nlayers, chunk, left_chunks};
  StateLayout s;
  WsLayout w;
  if (!state_layout(c, B, &s) || !ws_layout(c, B, chunk_T, head ? Cv : 0, &w)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total || workspace_bytes < w.total) return LR_ERR_WORKSPACE;
  for (int i = 0; i < 2 + 12 * nlayers; ++i) LR_CHECK_ARG(weights[i]);
  hipStream_t st = (hipStream_t)stream_;
  AdvArgs a;
  a.sizes = sizes; a.end = end; a.state = (char*)state;
  a.slot_bytes = s.slot_bytes; a.pend_off = s.pend_off; a.ring_off = s.ring_off;
  a.c = c; a.ringN = s.ringN; a.rows = w.rows; a.chunk_T = chunk_T; a.pe_rows = pe_rows; a.B = B;
  float* ws = (float*)workspace;
  const int R = (int)w.R, dh = Dm / nhead;
  const size_t qkv_layer = al64((size_t)R * 3 * Dm);
  if (R > 0) {
    LR_LAUNCH(gather_kernel, dim3(R), dim3(256), 0, st, a, x, stride_b, stride_t, pe, ws + w.X, ws + w.PE);
    LR_TRY_(lr_launch_status());
    float* h = ws + w.hA;
    float* hn = ws + w.hB;
    // h0 = x W_p^T + b_p + pe[position]
    LR_TRY_(rows_linear(ws + w.X, weights[0], weights[1], ws + w.PE, h, R, Dm, I, 0, st));
    static bool attr_set = false;
    const size_t lds = ((size_t)2 * (left_chunks + 1) * chunk * (dh + 1) + (size_t)4 * (left_chunks + 1) * chunk) * sizeof(float);
    if (!attr_set) {
      lr_clear_error();
      if (hipFuncSetAttribute((const void*)attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(((size_t)2 * kMaxWindow * (kMaxDh + 1) + 4 * kMaxWindow) * sizeof(float))) != hipSuccess)
        return LR_ERR_LAUNCH;
      attr_set = true;
    }
    const dim3 agrid(nhead, (w.rows + chunk - 1) / chunk, B);
    for (int l = 0; l < nlayers; ++l) {
      const float* const* W = weights + 2 + 12 * l;
      float* qkv = ws + w.qkv + (size_t)l * qkv_layer;
      LR_TRY_(rows_linear(h, W[0], W[1], nullptr, qkv, R, 3 * Dm, Dm, 0, st));
      LR_LAUNCH(attn_kernel, agrid, dim3(256), lds, st, a, (const float*)qkv, ws + w.a, l, 1.f / sqrtf((float)dh));
      LR_TRY_(lr_launch_status());
      LR_TRY_(rows_linear(ws + w.a, W[2], W[3], h, ws + w.s1, R, Dm, Dm, 0, st));             // s1 = a W_o^T + b_o + h
      LR_TRY_(lr_layernorm_forward(ws + w.s1, nullptr, W[8], W[9], ws + w.h1, ws + w.stats, R, Dm, eps, st));
      LR_TRY_(rows_linear(ws + w.h1, W[4], W[5], nullptr, ws + w.f1, R, F, Dm, 1, st));       // f1 = relu(h1 W_1^T + b_1)
      LR_TRY_(rows_linear(ws + w.f1, W[6], W[7], ws + w.h1, ws + w.s2, R, Dm, F, 0, st));     // s2 = f1 W_2^T + b_2 + h1
      LR_TRY_(lr_layernorm_forward(ws + w.s2, nullptr, W[10], W[11], hn, ws + w.stats, R, Dm, eps, st));
      float* t = h; h = hn; hn = t;
    }
    if (head) {
      LR_TRY_(rows_linear(h, head_w, head_b, nullptr, ws + w.logits, R, Cv, Dm, 0, st));
    }
    if (head || h_out) {
      LR_LAUNCH(finish_kernel, dim3((R + 3) / 4), dim3(256), 0, st, a, (const float*)h, (const float*)(ws + w.logits),
                head_b, head_mask, h_out, log_probs, (int64_t)R, Cv);
      LR_TRY_(lr_launch_status());
    }
  }
  LR_LAUNCH(commit_kernel, dim3(B), dim3(256), 0, st, a, x, stride_b, stride_t, (const float*)(ws + w.qkv), qkv_layer,
            counts);
  return lr_launch_status();
}

extern "C" int lr_tfm_stream_read(const void* state, size_t state_bytes, int32_t* frames, int32_t* emitted, int32_t* ended,
                                  int32_t* status, int B, int I, int Dm, int nhead, int F, int nlayers, int chunk,
                                  int left_chunks, lr_stream_t stream) {
  LR_CHECK_ARG(state && (frames || emitted || ended || status));
  LR_CHECK_ARG(B >= 1 && I >= 1 && Dm >= 1 && nhead >= 1 && F >= 1 && nlayers >= 1 && chunk >= 1 && left_chunks >= 0);
  const Cfg c{I, Dm, nhead, F, nlayers, chunk, left_chunks};
  StateLayout s;
  if (!state_layout(c, B, &s)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total) return LR_ERR_WORKSPACE;
  LR_LAUNCH(read_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, (const char*)state, s.slot_bytes, c, B, frames, emitted,
            ended, status);
  return lr_launch_status();
}
