// lr_rnn_bistream.hip — look-ahead sessions: a stacked BIDIRECTIONAL GRU / LSTM / tanh-RNN (and the CTC head) advanced
// chunk by chunk as a latency-controlled bidirectional RNN, on gfx950 (include/lipreading_hip.h lr_rnn_bistream_*,
// DESIGN.md §29).
//
// One advance hands slot b a window of window_T frames: it CONSUMES the first n_b = sizes[b] and SEES a_b = ahead[b]
// more, e_b = n_b + a_b.  The forward direction starts from the slot's carried state and runs over frames 0 .. e_b - 1
// (the layer above needs the look-ahead frames too); the state committed is the one after frame n_b - 1.  The backward
// direction starts from zero at frame e_b - 1, runs down to 0 and carries nothing.  Only consumed frames are returned.
//
// The step kernel is stream_step_kernel<G> of lr_rnn_stream.hip (16 slots x 16 units of all gates per workgroup, 8 waves
// splitting K over [x_t | h_{t-1}] against a fragment-major [W_ih | W_hh] pack, v_mfma_f32_16x16x4_f32 on exact fp32
// operands, a trip's loads all issued before its first MFMA, partial tiles meeting in LDS, fused cell).  What differs:
//   * both directions in one launch: grid (unit tiles, slot tiles, 2).  Launch k of a layer computes forward frame k
//     and, per slot, backward frame e_b - 1 - k.  layers x window_T step launches, at most one head launch, one commit
//     launch, linear on the caller's stream; no workgroup waits for another, no atomics, plain vector stores only.
//   * frame-indexed planes: the workspace holds one [B][Hp] plane per (layer, direction, frame); a plane is also the
//     layer above's input.  Every A-operand row pointer is per row: the backward h_prev of slot b is row b of plane
//     t + 1 of its own direction (zero at k = 0), the forward one plane k - 1 (the session state at k = 0).  A launch
//     never reads a row it writes: rows of plane t + 1 / k - 1 were written by the launch before.  A (slot, direction)
//     whose frame lies outside [0, e_b) loads zeros and stores nothing; nothing above reads what it leaves.
//   * upper layers contract over [fwd | bwd | h]: each part is padded to a multiple of 16 with zeros in the pack, so the
//     seam between the directions at H % 16 != 0 falls on a chunk border.
//   * the summation order of a (slot, unit) is fixed by (I, H, layer) alone: chunk c goes to wave c % 8, a wave adds its
//     chunks in rising order, the eight partial sums are added in wave order.  Neither B, the slot's position, chunk_T,
//     window_T, ahead nor the alignment of x changes a bit.
//   * the LSTM's c: element-wise per (slot, unit) — the thread that reads c_{t-1}[b][j] is the one that writes
//     c_t[b][j] — so it lives IN PLACE in one [B][Hp] plane per (layer, direction); the forward direction reads the
//     state's c at k = 0 and the backward one starts from 0.  The hazard a causal session does not have: the forward c
//     after frame n_b - 1 is overwritten by the look-ahead steps before the commit.  The forward step at t == n_b - 1
//     therefore stores c a second time, into a commit plane [layers][B][Hp] nobody else writes; the commit kernel copies
//     h from frame plane n_b - 1 and c from the commit plane.
#include "lr_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;        // slots and hidden units per workgroup
constexpr int RED_LD = 17;      // padded row of the cross-wave reduction buffer
constexpr int NW = 8;           // waves per workgroup: K is split NW ways
constexpr int UF = 6;           // chunks (16 k each) a wave keeps in flight per trip
constexpr int FRAG = 256;       // floats per 16 x 16 operand fragment
constexpr int kMaxLayers = 16;
constexpr int kMaxClasses = 256;
constexpr int kMaxChunk = 1 << 20;
constexpr int32_t kMagic = 0x4c524253;   // not the causal session's: either rejects the other's state
constexpr int kHdrWords = 8;    // magic, B, H, layers, cell, frames, status, 0
enum { HD_MAGIC = 0, HD_B, HD_H, HD_LAYERS, HD_CELL, HD_FRAMES, HD_STATUS };

__host__ __device__ inline int gates_of(int cell) { return cell == LR_RNN_GRU ? 3 : cell == LR_RNN_LSTM ? 4 : 1; }

struct StateLayout {
  size_t Hp, h_off, c_off, plane_bytes, total;   // byte offsets; plane = [layers][B][Hp] floats (forward direction)
};
bool state_layout(int mode, int B, int H, int layers, StateLayout* s) {
  if (mode < 0 || mode > LR_RNN_TANH || B < 1 || H < 1 || layers < 1 || layers > kMaxLayers) return false;
  if (B > 65535 * TILE || H > (1 << 20)) return false;
  s->Hp = ((size_t)H + 15) / 16 * 16;
  s->h_off = lr_align_up((size_t)B * kHdrWords * sizeof(int32_t), 256);
  s->plane_bytes = lr_align_up((size_t)layers * B * s->Hp * sizeof(float), 256);
  s->c_off = s->h_off + s->plane_bytes;
  s->total = s->c_off + (mode == LR_RNN_LSTM ? s->plane_bytes : 0);
  return true;
}

struct PackLayout {
  size_t w_off[kMaxLayers][2];   // float offsets of a (layer, direction)'s fragments [unit tile][chunk][gate][64][4]
  size_t bias_off;               // [layers][2][4][HT * 16]
  size_t total;                  // bytes
};
// chunks of 16 k a layer's input takes: x, or [fwd | bwd] of the layer below, each half padded apart
__host__ __device__ inline int in_chunks(int l, int I, int H) { return l == 0 ? (I + 15) / 16 : 2 * ((H + 15) / 16); }
bool pack_layout(int mode, int I, int H, int layers, PackLayout* p) {
  if (mode < 0 || mode > LR_RNN_TANH || I < 1 || H < 1 || layers < 1 || layers > kMaxLayers) return false;
  if (I > (1 << 20) || H > (1 << 20)) return false;
  const size_t G = gates_of(mode), HT = ((size_t)H + 15) / 16;
  size_t off = 0;
  for (int l = 0; l < layers; ++l)
    for (int d = 0; d < 2; ++d) {
      const size_t nchunk = (size_t)in_chunks(l, I, H) + HT;
      p->w_off[l][d] = off;
      off += lr_align_up(HT * nchunk * G * FRAG * sizeof(float), 256) / sizeof(float);
    }
  p->bias_off = off;
  off += lr_align_up((size_t)layers * 2 * 4 * HT * 16 * sizeof(float), 256) / sizeof(float);
  p->total = off * sizeof(float);
  return true;
}

struct WsLayout {
  // hs [layers][2][window_T][B][Hp]; LSTM: cs [layers][2][B][Hp] in place, cc [layers][B][Hp] for the commit
  size_t Hp, hs_off, cs_off, cc_off, total;
};
bool ws_layout(int mode, int B, int chunk_T, int window_T, int I, int H, int layers, int C, WsLayout* w) {
  StateLayout s;
  if (!state_layout(mode, B, H, layers, &s) || I < 1 || chunk_T < 0 || window_T < chunk_T || window_T > kMaxChunk || C < 0 ||
      C > kMaxClasses)
    return false;
  const bool lstm = mode == LR_RNN_LSTM;
  w->Hp = s.Hp;
  w->hs_off = 0;
  w->cs_off = lr_align_up((size_t)layers * 2 * (window_T > 0 ? window_T : 1) * B * s.Hp * sizeof(float), 256);
  w->cc_off = w->cs_off + (lstm ? lr_align_up((size_t)layers * 2 * B * s.Hp * sizeof(float), 256) : 0);
  w->total = w->cc_off + (lstm ? s.plane_bytes : 0);
  return true;
}

// the slot carries this call's configuration
__device__ __forceinline__ bool slot_ok(const int32_t* __restrict__ hdr, int b, int B, int H, int layers, int cell) {
  const int32_t* h = hdr + (int64_t)b * kHdrWords;
  return h[HD_MAGIC] == kMagic && h[HD_B] == B && h[HD_H] == H && h[HD_LAYERS] == layers && h[HD_CELL] == cell;
}
// frames consumed, 0 <= n <= chunk_T
__device__ __forceinline__ int frames_of(const int32_t* __restrict__ sizes, int b, int chunk_T) {
  if (!sizes) return chunk_T;
  const int n = sizes[b];
  return n < 0 ? 0 : n > chunk_T ? chunk_T : n;
}
// the end of the slot's own window, n <= e <= window_T
__device__ __forceinline__ int end_of(const int32_t* __restrict__ ahead, int b, int n, int window_T) {
  if (!ahead) return n;
  const int a = ahead[b], room = window_T - n;
  return n + (a < 0 ? 0 : a > room ? room : a);
}

// a lane's float4 of an A operand: row[k .. k + 3], zero at k >= lim (the row may be followed by anything).  Four
// floats in one load where the row allows it; the values are the same either way.
__device__ __forceinline__ float4 lda(const float* __restrict__ row, int k, int lim, bool vec) {
  if (vec && k + 3 < lim) return *reinterpret_cast<const float4*>(row + k);
  float4 v;
  v.x = k < lim ? row[k] : 0.f;
  v.y = k + 1 < lim ? row[k + 1] : 0.f;
  v.z = k + 2 < lim ? row[k + 2] : 0.f;
  v.w = k + 3 < lim ? row[k + 3] : 0.f;
  return v;
}

#define LR_MFMA4(accv, av, wv)                                                 \
  accv = __builtin_amdgcn_mfma_f32_16x16x4f32((av).x, (wv).x, accv, 0, 0, 0); \
  accv = __builtin_amdgcn_mfma_f32_16x16x4f32((av).y, (wv).y, accv, 0, 0, 0); \
  accv = __builtin_amdgcn_mfma_f32_16x16x4f32((av).z, (wv).z, accv, 0, 0, 0); \
  accv = __builtin_amdgcn_mfma_f32_16x16x4f32((av).w, (wv).w, accv, 0, 0, 0)

struct StepArgs {
  const float* x;         // layer 0: frame t of slot b at x + b * x_sb + t * x_st, I floats
  int64_t x_sb, x_st;
  int x_vec;              // every such row is 16-byte aligned
  const float* below;     // upper layers: the planes of the layer below, (direction d, frame t) at (d * window_T + t) * B * Hp
  const float* st_h;      // [B][Hp] the state's forward h of this layer (read at k = 0 only)
  const float* st_c;      // LSTM: c likewise
  float* hs;              // this layer's planes, indexed as `below`
  float* cs;              // LSTM: [2][B][Hp], in place
  float* cc;              // LSTM: [B][Hp], the forward c after the last consumed frame
  float* y;               // last layer, or NULL: [B][chunk_T][2 H]
  const float* w[2];      // the (layer, direction)'s fragments
  const float* bias[2];   // [4][HT * 16]
  const int32_t* hdr;     // the state's headers
  const int32_t* sizes;
  const int32_t* ahead;
  int cell, layers, B, I, H, Hp, k, chunk_T, window_T, upper;
};

template <int G>
__global__ __launch_bounds__(NW * 64) void bistream_step_kernel(StepArgs p) {
  constexpr int NA = G == 3 ? 4 : G;   // accumulators: GRU r, z, n_x, n_h
  __shared__ float red[NW * NA * TILE * RED_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * TILE, b0 = blockIdx.y * TILE, dir = blockIdx.z;
  const int H = p.H, Hp = p.Hp, B = p.B, k = p.k, W = p.window_T;
  const int HTp = gridDim.x * 16;
  const int64_t plane = (int64_t)B * Hp;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // ---- epilogue operands first (threads 0..255 own one (slot, hidden unit) each) ------------------------------------
  const int bl = (tid >> 4) & 15, jl = tid & 15;
  const int b = b0 + bl, j = j0 + jl;
  const bool epi = tid < 256 && b < B && j < H;
  float prev_h = 0.f, prev_c = 0.f, bs[4] = {0.f, 0.f, 0.f, 0.f};
  bool active = false;
  int n = 0, t = 0;
  if (epi) {
    int e = 0;
    if (slot_ok(p.hdr, b, B, H, p.layers, p.cell)) {
      n = frames_of(p.sizes, b, p.chunk_T);
      e = end_of(p.ahead, b, n, W);
    }
    active = k < e;
    t = dir ? e - 1 - k : k;
    if (active) {
      if (k > 0) {
        prev_h = p.hs[((int64_t)dir * W + (dir ? t + 1 : t - 1)) * plane + (int64_t)b * Hp + j];
        if (G == 4) prev_c = p.cs[(int64_t)dir * plane + (int64_t)b * Hp + j];
      } else if (!dir) {
        prev_h = p.st_h[(int64_t)b * Hp + j];
        if (G == 4) prev_c = p.st_c[(int64_t)b * Hp + j];
      }
    }
#pragma unroll
    for (int g = 0; g < (G == 3 ? 4 : G); ++g) bs[g] = p.bias[dir][g * HTp + j];
  }

  // ---- acc[g] (16 slots x 16 units) += [in_t | h_prev] (16 x K) . [W_ih | W_hh]_g^T (K x 16) ------------------------
  {
    f32x4 acc[NA];
#pragma unroll
    for (int g = 0; g < NA; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int rowi = lane & 15, kq = lane >> 4;
    const int HT = (H + 15) >> 4;
    const int nci = p.upper ? 2 * HT : (p.I + 15) >> 4, nchunk = nci + HT;
    const int ar = b0 + rowi;
    // this lane's row: the slot's own frame of this direction
    bool row_in = false;
    const float *in0 = p.st_h, *in1 = p.st_h, *hrow = nullptr;   // (any valid address; never read unless row_in)
    if (ar < B && slot_ok(p.hdr, ar, B, H, p.layers, p.cell)) {
      const int nr = frames_of(p.sizes, ar, p.chunk_T), er = end_of(p.ahead, ar, nr, W);
      if (k < er) {
        row_in = true;
        const int tr = dir ? er - 1 - k : k;
        if (p.upper) {
          in0 = p.below + (int64_t)tr * plane + (int64_t)ar * Hp;
          in1 = in0 + (int64_t)W * plane;
        } else {
          in0 = p.x + (int64_t)ar * p.x_sb + (int64_t)tr * p.x_st;
        }
        if (k > 0) hrow = p.hs + ((int64_t)dir * W + (dir ? tr + 1 : tr - 1)) * plane + (int64_t)ar * Hp;
        else if (!dir) hrow = p.st_h + (int64_t)ar * Hp;
      }
    }
    const int in_lim = p.upper ? H : p.I;
    const bool in_vec = p.upper || p.x_vec != 0;
    const float* wsrc = p.w[dir] + ((int64_t)blockIdx.x * nchunk) * (G * FRAG) + lane * 4;
    for (int c0 = wave; c0 < nchunk; c0 += NW * UF) {
      float4 a[UF], w[UF][G];
#pragma unroll
      for (int u = 0; u < UF; ++u) {
        const int c = c0 + u * NW;
        const bool ok = c < nchunk;
        a[u] = zero4;
        if (ok && row_in) {
          if (c < nci) {
            const bool second = p.upper && c >= HT;
            a[u] = lda(second ? in1 : in0, (second ? c - HT : c) * 16 + 4 * kq, in_lim, in_vec);
          } else if (hrow) {
            a[u] = lda(hrow, (c - nci) * 16 + 4 * kq, H, true);
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
          w[u][g] = ok ? *reinterpret_cast<const float4*>(wsrc + ((int64_t)c * G + g) * FRAG) : zero4;
      }
#pragma unroll
      for (int u = 0; u < UF; ++u) {
        const int c = c0 + u * NW;
        if (c < nchunk) {   // wave-uniform
          if (G == 3) {
            LR_MFMA4(acc[0], a[u], w[u][0]);
            LR_MFMA4(acc[1], a[u], w[u][1]);
            if (c < nci) {
              LR_MFMA4(acc[2], a[u], w[u][G - 1]);
            } else {
              LR_MFMA4(acc[NA - 1], a[u], w[u][G - 1]);
            }
          } else {
#pragma unroll
            for (int g = 0; g < G; ++g) { LR_MFMA4(acc[g], a[u], w[u][g]); }
          }
        }
      }
    }
    // C/D layout of 16x16x4: col = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
    for (int g = 0; g < NA; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((wave * NA + g) * TILE + kq * 4 + r) * RED_LD + rowi] = acc[g][r];
  }
  __syncthreads();
  if (!epi) return;

  float s[NA];
#pragma unroll
  for (int g = 0; g < NA; ++g) {
    s[g] = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s[g] += red[((w * NA + g) * TILE + bl) * RED_LD + jl];
  }
  float h, c = 0.f;
  if (G == 1) {
    h = tanhf(s[0] + bs[0]);
  } else if (G == 3) {
    const float r = lr_sigmoid(s[0] + bs[0]);
    const float z = lr_sigmoid(s[1] + bs[1]);
    const float nn = tanhf((s[2] + bs[2]) + r * (s[NA - 1] + bs[3]));
    h = (1.f - z) * nn + z * prev_h;
  } else {
    const float ig = lr_sigmoid(s[0] + bs[0]);
    const float fg = lr_sigmoid(s[1] + bs[1]);
    const float gg = tanhf(s[2] + bs[2]);
    const float og = lr_sigmoid(s[NA - 1] + bs[3]);
    c = fg * prev_c + ig * gg;
    h = og * tanhf(c);
  }
  if (active) {   // 0 <= t < e <= window_T
    p.hs[((int64_t)dir * W + t) * plane + (int64_t)b * Hp + j] = h;
    if (G == 4) {
      p.cs[(int64_t)dir * plane + (int64_t)b * Hp + j] = c;
      if (!dir && t == n - 1) p.cc[(int64_t)b * Hp + j] = c;
    }
  }
  if (p.y) {
    float* yb = p.y + (int64_t)b * p.chunk_T * 2 * H;
    if (!dir) {
      if (k < n) {
        yb[(int64_t)k * 2 * H + j] = h;
      } else if (k < p.chunk_T) {   // a row past the slot's frames: both halves are zero, written here once
        yb[(int64_t)k * 2 * H + j] = 0.f;
        yb[(int64_t)k * 2 * H + H + j] = 0.f;
      }
    } else if (active && t < n) {
      yb[(int64_t)t * 2 * H + H + j] = h;
    }
  }
}

// a lane's float4 of the row [f | g] (H floats each): k .. k + 3 of the 2 H wide concatenation, zero past it
__device__ __forceinline__ float4 lda2(const float* __restrict__ f, const float* __restrict__ g, int k, int H) {
  if (k + 3 < H) return *reinterpret_cast<const float4*>(f + k);
  if (k >= H && ((k - H) & 3) == 0 && k - H + 3 < H) return *reinterpret_cast<const float4*>(g + (k - H));
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kk = k + i;
    v[i] = kk < H ? f[kk] : kk < 2 * H ? g[kk - H] : 0.f;
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

// The head over 16-row blocks of the consumed frames (row r = b * chunk_T + t): log_softmax([fwd_t | bwd_t] W^T + bias +
// log(mask + 1e-45)), K = 2 H, wave w owning classes [16 w, 16 w + 16).  A row's arithmetic is one wave's walk over K in
// rising order, whatever the number of rows.  Rows past a slot's frames are the zero row.  (stream_head_kernel of
// lr_rnn_stream.hip reads ONE plane row of K floats; here a row is two rows of two planes, so the walk is written out.)
__global__ __launch_bounds__(1024) void bistream_head_kernel(const float* __restrict__ hs, const float* __restrict__ Wt,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ mask,
                                                             float* __restrict__ log_probs,
                                                             const int32_t* __restrict__ hdr,
                                                             const int32_t* __restrict__ sizes, int cell, int layers,
                                                             int B, int chunk_T, int window_T, int H, int Hp, int C,
                                                             int w_vec) {
  __shared__ float logits[16][kMaxClasses + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int row = lane & 15, q = lane >> 4;
  const int K = 2 * H;
  const int64_t R = (int64_t)B * chunk_T;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int64_t ra = r0 + row;
  const int64_t plane = (int64_t)B * Hp;
  bool live = false;
  const float *frow = hs, *grow = hs;
  if (ra < R) {
    const int b = (int)(ra / chunk_T), t = (int)(ra - (int64_t)b * chunk_T);
    live = slot_ok(hdr, b, B, H, layers, cell) && t < frames_of(sizes, b, chunk_T);
    frow = hs + (int64_t)t * plane + (int64_t)b * Hp;
    grow = frow + (int64_t)window_T * plane;
  }
  const int cls = min(16 * wave + row, C - 1);   // classes past C compute a copy of the last one (never stored)
  const float* wrow = Wt + (int64_t)cls * K;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int steps = (K + 15) >> 4;
  for (int s = 0; s < steps; ++s) {
    const int k = s * 16 + 4 * q;
    const float4 a = live ? lda2(frow, grow, k, H) : zero4;
    const float4 w = lda(wrow, k, K, w_vec != 0);
    LR_MFMA4(acc, a, w);
  }
  {
    const int c = 16 * wave + row;
    const float add = c < C ? bias[c] + logf(mask[c] + 1e-45f) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) logits[4 * q + i][c] = acc[i] + add;
  }
  __syncthreads();
  // sixteen lanes per row, four rows per wave and pass
  for (int rl = wave * 4 + q; rl < 16; rl += nw * 4) {
    const int64_t r = r0 + rl;
    float m = LR_NEG_INF;
    for (int c = row; c < C; c += 16) m = fmaxf(m, logits[rl][c]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float sum = 0.f;
    for (int c = row; c < C; c += 16) sum += expf(logits[rl][c] - m);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float lse = m + logf(sum);
    if (r < R)
      for (int c = row; c < C; c += 16) log_probs[r * C + c] = logits[rl][c] - lse;
  }
}

// Forward plane n_b - 1 of every layer (and the commit plane of c) -> the state; consumed frames counted (saturating).
// A slot with n_b == 0 keeps every bit; a slot with another configuration is left alone and flagged.
__global__ void bistream_commit_kernel(int32_t* hdr, float* sh, float* sc, const float* __restrict__ hs,
                                       const float* __restrict__ cc, const int32_t* __restrict__ sizes, int cell,
                                       int layers, int B, int chunk_T, int window_T, int H, int Hp) {
  const int64_t total = (int64_t)layers * B * Hp;
  const int64_t plane = (int64_t)B * Hp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % Hp);
    const int b = (int)((i / Hp) % B);
    const int l = (int)(i / ((int64_t)Hp * B));
    const bool ok = slot_ok(hdr, b, B, H, layers, cell);
    const int n = ok ? frames_of(sizes, b, chunk_T) : 0;
    if (n > 0 && j < H) {
      sh[i] = hs[((int64_t)l * 2 * window_T + (n - 1)) * plane + (int64_t)b * Hp + j];
      if (sc) sc[i] = cc[i];
    }
    if (l == 0 && j == 0) {
      int32_t* h = hdr + (int64_t)b * kHdrWords;
      if (!ok) {
        h[HD_STATUS] |= LR_RNN_STREAM_MISMATCH;
      } else if (n > 0) {
        const int64_t f = (int64_t)h[HD_FRAMES] + n;
        h[HD_FRAMES] = f > 0x7fffffff ? 0x7fffffff : (int32_t)f;
      }
    }
  }
}

__global__ void bistream_reset_kernel(int32_t* hdr, float* sh, float* sc, const int32_t* __restrict__ mask, int cell,
                                      int layers, int B, int H, int Hp) {
  const int64_t total = (int64_t)layers * B * Hp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % Hp);
    const int b = (int)((i / Hp) % B);
    const int l = (int)(i / ((int64_t)Hp * B));
    const bool mine = !mask || mask[b] != 0;
    const bool ok = !mask || slot_ok(hdr, b, B, H, layers, cell);
    if (mine && ok) {
      sh[i] = 0.f;
      if (sc) sc[i] = 0.f;
    }
    if (l == 0 && j == 0 && mine) {
      int32_t* h = hdr + (int64_t)b * kHdrWords;
      if (!mask) {
        h[HD_MAGIC] = kMagic;
        h[HD_B] = B;
        h[HD_H] = H;
        h[HD_LAYERS] = layers;
        h[HD_CELL] = cell;
        h[7] = 0;
      }
      if (ok) {
        h[HD_FRAMES] = 0;
        h[HD_STATUS] = 0;
      } else {
        h[HD_STATUS] |= LR_RNN_STREAM_MISMATCH;
      }
    }
  }
}

__global__ void bistream_read_kernel(const int32_t* __restrict__ hdr, const float* __restrict__ sh,
                                     const float* __restrict__ sc, float* __restrict__ h_out, float* __restrict__ c_out,
                                     int32_t* __restrict__ frames, int32_t* __restrict__ status, int layers, int B, int H,
                                     int Hp, int has_c) {
  const int64_t total = (int64_t)layers * B * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % H);
    const int b = (int)((i / H) % B);
    const int l = (int)(i / ((int64_t)H * B));
    const int32_t* h = hdr + (int64_t)b * kHdrWords;
    const int cell = h[HD_CELL];
    const bool ok = h[HD_MAGIC] == kMagic && h[HD_B] == B && h[HD_H] == H && h[HD_LAYERS] == layers && cell >= 0 &&
                    cell <= LR_RNN_TANH && (cell == LR_RNN_LSTM || !has_c);
    const int64_t src = ((int64_t)l * B + b) * Hp + j;
    if (h_out) h_out[i] = ok ? sh[src] : 0.f;
    if (c_out) c_out[i] = ok && sc ? sc[src] : 0.f;
    if (l == 0 && j == 0) {
      if (frames) frames[b] = ok ? h[HD_FRAMES] : 0;
      if (status) status[b] = ok ? h[HD_STATUS] : (h[HD_MAGIC] == kMagic ? h[HD_STATUS] : 0) | LR_RNN_STREAM_MISMATCH;
    }
  }
}

// [W_ih | W_hh] of one (layer, direction) -> fragment-major, zero past every part's end.  W_ih's columns are `parts`
// runs of `seg` (x: 1 x I; upper layers: 2 x H, fwd then bwd), each run padded to a multiple of 16 on its own:
//   out[(((jt * nchunk + c) * G + g) * 64 + l) * 4 + q] = W[g * H + jt * 16 + (l & 15)][col]
// with, SC = ceil(seg / 16), nci = parts * SC: for c < nci, W = W_ih and col = (c / SC) * seg + (c % SC) * 16 +
// 4 * (l >> 4) + q where that lies inside the run; for c >= nci, W = W_hh and col = (c - nci) * 16 + 4 * (l >> 4) + q.
// Any I, H; no alignment asked of the sources.
__global__ void bistream_pack_w_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                       float* __restrict__ out, int G, int seg, int parts, int H) {
  const int HT = (H + 15) >> 4, SC = (seg + 15) >> 4, nci = parts * SC, nchunk = nci + HT;
  const int64_t total = (int64_t)HT * nchunk * G * FRAG;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i & 3), l = (int)((i >> 2) & 63);
    int64_t r = i >> 8;
    const int g = (int)(r % G);
    r /= G;
    const int c = (int)(r % nchunk);
    const int jt = (int)(r / nchunk);
    const int unit = jt * 16 + (l & 15);
    float v = 0.f;
    if (unit < H) {
      if (c < nci) {
        const int part = c / SC, k = (c - part * SC) * 16 + 4 * (l >> 4) + q;
        if (k < seg) v = w_ih[((int64_t)g * H + unit) * ((int64_t)parts * seg) + (int64_t)part * seg + k];
      } else {
        const int k = (c - nci) * 16 + 4 * (l >> 4) + q;
        if (k < H) v = w_hh[((int64_t)g * H + unit) * H + k];
      }
    }
    out[i] = v;
  }
}

// bias[slot][HT * 16]: b_ih + b_hh per gate; the GRU's n gate keeps b_in in slot 2 and b_hn in slot 3
__global__ void bistream_pack_bias_kernel(const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                          float* __restrict__ out, int G, int H) {
  const int HTp = ((H + 15) >> 4) * 16;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * HTp) return;
  const int slot = i / HTp, j = i % HTp;
  float v = 0.f;
  if (j < H) {
    if (G == 3) {
      if (slot < 2) v = b_ih[slot * H + j] + b_hh[slot * H + j];
      else if (slot == 2) v = b_ih[2 * H + j];
      else v = b_hh[2 * H + j];
    } else if (slot < G) {
      v = b_ih[slot * H + j] + b_hh[slot * H + j];
    }
  }
  out[i] = v;
}

unsigned blocks_for(int64_t n, int threads) {
  int64_t b = (n + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : b > 65535 ? 65535 : b);
}

}  // namespace

extern "C" size_t lr_rnn_bistream_pack_bytes(int mode, int I, int H, int layers) {
  PackLayout p;
  return pack_layout(mode, I, H, layers, &p) ? p.total : 0;
}

extern "C" size_t lr_rnn_bistream_state_bytes(int mode, int B, int H, int layers) {
  StateLayout s;
  return state_layout(mode, B, H, layers, &s) ? s.total : 0;
}

extern "C" size_t lr_rnn_bistream_workspace_bytes(int mode, int B, int chunk_T, int window_T, int I, int H, int layers,
                                                  int C) {
  WsLayout w;
  return ws_layout(mode, B, chunk_T, window_T, I, H, layers, C, &w) ? w.total : 0;
}

extern "C" int lr_rnn_bistream_pack(void* out, size_t out_bytes, int mode, const float* const* w_ih,
                                    const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, int I,
                                    int H, int layers, lr_stream_t stream) {
  LR_CHECK_ARG(out && w_ih && w_hh && b_ih && b_hh);
  LR_CHECK_ARG(I >= 1 && H >= 1 && layers >= 1 && mode >= 0);
  PackLayout p;
  if (!pack_layout(mode, I, H, layers, &p)) return LR_ERR_UNSUPPORTED;
  if (out_bytes < p.total) return LR_ERR_WORKSPACE;
  for (int i = 0; i < 2 * layers; ++i) LR_CHECK_ARG(w_ih[i] && w_hh[i] && b_ih[i] && b_hh[i]);
  const int G = gates_of(mode), HT = (H + 15) / 16;
  float* o = (float*)out;
  for (int l = 0; l < layers; ++l)
    for (int d = 0; d < 2; ++d) {
      const int i = 2 * l + d;
      const int64_t total = (int64_t)HT * (in_chunks(l, I, H) + HT) * G * FRAG;
      LR_LAUNCH(bistream_pack_w_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, stream, w_ih[i], w_hh[i],
                o + p.w_off[l][d], G, l == 0 ? I : H, l == 0 ? 1 : 2, H);
      int st = lr_launch_status();
      if (st != LR_OK) return st;
      LR_LAUNCH(bistream_pack_bias_kernel, dim3((4 * HT * 16 + 255) / 256), dim3(256), 0, stream, b_ih[i], b_hh[i],
                o + p.bias_off + (size_t)i * 4 * HT * 16, G, H);
      st = lr_launch_status();
      if (st != LR_OK) return st;
    }
  return LR_OK;
}

extern "C" int lr_rnn_bistream_reset(void* state, size_t state_bytes, const int32_t* mask, int mode, int B, int H,
                                     int layers, lr_stream_t stream) {
  LR_CHECK_ARG(state);
  LR_CHECK_ARG(B >= 1 && H >= 1 && layers >= 1 && mode >= 0);
  StateLayout s;
  if (!state_layout(mode, B, H, layers, &s)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total) return LR_ERR_WORKSPACE;
  char* base = (char*)state;
  LR_LAUNCH(bistream_reset_kernel, dim3(blocks_for((int64_t)layers * B * s.Hp, 256)), dim3(256), 0, stream,
            (int32_t*)base, (float*)(base + s.h_off), mode == LR_RNN_LSTM ? (float*)(base + s.c_off) : (float*)nullptr,
            mask, mode, layers, B, H, (int)s.Hp);
  return lr_launch_status();
}

extern "C" int lr_rnn_bistream_advance(int mode, const float* x, int64_t stride_b, int64_t stride_t,
                                       const int32_t* sizes, const int32_t* ahead, const void* pack, size_t pack_bytes,
                                       const float* head_w, const float* head_b, const float* head_mask, float* y,
                                       float* log_probs, void* state, size_t state_bytes, void* workspace,
                                       size_t workspace_bytes, int B, int chunk_T, int window_T, int I, int H, int layers,
                                       int C, lr_stream_t stream) {
  LR_CHECK_ARG(x && pack && state && workspace);
  LR_CHECK_ARG(B >= 1 && chunk_T >= 0 && window_T >= chunk_T && I >= 1 && H >= 1 && layers >= 1 && C >= 0 && mode >= 0);
  LR_CHECK_ARG(stride_b >= 0 && stride_t >= 0);
  LR_CHECK_ARG(((reinterpret_cast<uintptr_t>(pack) | reinterpret_cast<uintptr_t>(state) |
                 reinterpret_cast<uintptr_t>(workspace)) & 15) == 0);
  const bool head = head_w || head_b || head_mask;
  if (head) LR_CHECK_ARG(head_w && head_b && head_mask && log_probs && C >= 1);
  else LR_CHECK_ARG(!log_probs);
  StateLayout s;
  PackLayout pk;
  WsLayout w;
  if (!state_layout(mode, B, H, layers, &s) || !pack_layout(mode, I, H, layers, &pk) ||
      !ws_layout(mode, B, chunk_T, window_T, I, H, layers, head ? C : 0, &w))
    return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total || pack_bytes < pk.total || workspace_bytes < w.total) return LR_ERR_WORKSPACE;
  if (chunk_T == 0) return LR_OK;
  char* sb = (char*)state;
  int32_t* hdr = (int32_t*)sb;
  const bool lstm = mode == LR_RNN_LSTM;
  const int Hp = (int)s.Hp, HT = Hp / 16;
  float* sh = (float*)(sb + s.h_off);
  float* sc = lstm ? (float*)(sb + s.c_off) : nullptr;
  float* hs = (float*)((char*)workspace + w.hs_off);
  float* cs = lstm ? (float*)((char*)workspace + w.cs_off) : nullptr;
  float* cc = lstm ? (float*)((char*)workspace + w.cc_off) : nullptr;
  const float* pf = (const float*)pack;
  const int64_t plane = (int64_t)B * Hp, layer_stride = plane * 2 * window_T;
  const dim3 grid(HT, (B + TILE - 1) / TILE, 2), block(NW * 64);
  const bool x_al = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && stride_b % 4 == 0 && stride_t % 4 == 0;
  for (int l = 0; l < layers; ++l) {
    StepArgs a;
    a.x = x;
    a.x_sb = stride_b;
    a.x_st = stride_t;
    a.x_vec = x_al ? 1 : 0;
    a.below = l > 0 ? hs + (int64_t)(l - 1) * layer_stride : nullptr;
    a.st_h = sh + (int64_t)l * plane;
    a.st_c = sc ? sc + (int64_t)l * plane : nullptr;
    a.hs = hs + (int64_t)l * layer_stride;
    a.cs = cs ? cs + (int64_t)l * 2 * plane : nullptr;
    a.cc = cc ? cc + (int64_t)l * plane : nullptr;
    a.y = (y && l == layers - 1) ? y : nullptr;
    for (int d = 0; d < 2; ++d) {
      a.w[d] = pf + pk.w_off[l][d];
      a.bias[d] = pf + pk.bias_off + (size_t)(2 * l + d) * 4 * Hp;
    }
    a.hdr = hdr;
    a.sizes = sizes;
    a.ahead = ahead;
    a.cell = mode;
    a.layers = layers;
    a.B = B;
    a.I = I;
    a.H = H;
    a.Hp = Hp;
    a.chunk_T = chunk_T;
    a.window_T = window_T;
    a.upper = l > 0 ? 1 : 0;
    for (int k = 0; k < window_T; ++k) {
      a.k = k;
      if (mode == LR_RNN_GRU) LR_LAUNCH(bistream_step_kernel<3>, grid, block, 0, stream, a);
      else if (lstm) LR_LAUNCH(bistream_step_kernel<4>, grid, block, 0, stream, a);
      else LR_LAUNCH(bistream_step_kernel<1>, grid, block, 0, stream, a);
      const int st = lr_launch_status();
      if (st != LR_OK) return st;
    }
  }
  if (head) {
    const int64_t R = (int64_t)B * chunk_T;
    const int nw = (C + 15) / 16;
    const int w_vec = (2 * H) % 4 == 0 && (reinterpret_cast<uintptr_t>(head_w) & 15) == 0;
    LR_LAUNCH(bistream_head_kernel, dim3((unsigned)((R + 15) / 16)), dim3(64 * nw), 0, stream,
              (const float*)(hs + (int64_t)(layers - 1) * layer_stride), head_w, head_b, head_mask, log_probs,
              (const int32_t*)hdr, sizes, mode, layers, B, chunk_T, window_T, H, Hp, C, w_vec);
    const int st = lr_launch_status();
    if (st != LR_OK) return st;
  }
  LR_LAUNCH(bistream_commit_kernel, dim3(blocks_for((int64_t)layers * plane, 256)), dim3(256), 0, stream, hdr, sh, sc,
            (const float*)hs, (const float*)cc, sizes, mode, layers, B, chunk_T, window_T, H, Hp);
  return lr_launch_status();
}

extern "C" int lr_rnn_bistream_read(const void* state, size_t state_bytes, float* h, float* c, int32_t* frames,
                                    int32_t* status, int B, int H, int layers, lr_stream_t stream) {
  LR_CHECK_ARG(state && (h || c || frames || status));
  LR_CHECK_ARG(B >= 1 && H >= 1 && layers >= 1);
  StateLayout s;
  const int mode = c ? LR_RNN_LSTM : LR_RNN_GRU;
  if (!state_layout(mode, B, H, layers, &s)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total) return LR_ERR_WORKSPACE;
  const char* base = (const char*)state;
  LR_LAUNCH(bistream_read_kernel, dim3(blocks_for((int64_t)layers * B * H, 256)), dim3(256), 0, stream,
            (const int32_t*)base, (const float*)(base + s.h_off), c ? (const float*)(base + s.c_off) : (const float*)nullptr,
            h, c, frames, status, layers, B, H, (int)s.Hp, c ? 1 : 0);
  return lr_launch_status();
}
