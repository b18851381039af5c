// lr_rnn_stream.hip — resumable encoder sessions: a stacked uni-directional GRU / LSTM / tanh-RNN (and the CTC head)
// advanced chunk by chunk from a caller-owned state, on gfx950 (include/lipreading_hip.h lr_rnn_stream_*).
//
// The geometry is the forward step kernel's of lr_rnn.hip: a workgroup owns a 16 (slots) x 16 (hidden units) tile of
// all gates, its 8 waves split K, v_mfma_f32_16x16x4_f32 on exact fp32 operands, a wave's loads of a trip are all
// issued before its first MFMA, the partial tiles meet in LDS and the cell is fused.  What differs:
//   * K runs over [x_t | h_{t-1}] against [W_ih | W_hh]: the input projection is inside the step, so that a frame's
//     arithmetic does not depend on how the stream was cut (lr_sgemm's split-K plan depends on its row count) and a
//     one-frame advance is `layers` launches.  The GRU's n gate keeps its x part and its h part in two accumulators
//     (r multiplies the h part only): four accumulators for the GRU and for the LSTM, one for the tanh RNN.
//   * nothing is kept for a backward; the weights come from a pack made once per weight set (lr_rnn_stream_pack).
//   * the summation order of a (slot, unit) is fixed by (I, H) alone: chunk c goes to wave c % 8, a wave adds its chunks
//     in rising order, the eight partial sums are added in wave order.  Rows of an MFMA are independent, so neither B,
//     the slot's position in the batch, chunk_T nor the alignment of x changes a bit.
//   * the state hazard: every workgroup of a step reads all of h_{t-1} while others write h_t.  The steps of an advance
//     therefore write h_t (and c_t) into the WORKSPACE, one [B][Hp] plane per (layer, frame) — a plane is also the
//     layer above's x_t — and read the state itself only at t = 0; one commit launch copies the last planes back and
//     counts the frames.  The state holds one copy of h / c, so its bytes do not depend on the number of advances.
//   * layers x chunk_T step launches, at most one head launch, one commit launch, all on the caller's stream; no
//     workgroup waits for another, no atomics, every store a plain vector store.
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
constexpr int32_t kMagic = 0x4c525353;
constexpr int kHdrWords = 8;    // magic, B, H, layers, cell, frames, status, 0
enum { HD_MAGIC = 0, HD_B, HD_H, HD_LAYERS, HD_CELL, HD_FRAMES, HD_STATUS };

__host__ __device__ inline int gates_of(int cell) { return cell == LR_RNN_GRU ? 3 : cell == LR_RNN_LSTM ? 4 : 1; }

struct StateLayout {
  size_t Hp, h_off, c_off, plane_bytes, total;   // byte offsets; plane = [layers][B][Hp] floats
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
  size_t w_off[kMaxLayers];   // float offsets of a layer's fragments [unit tile][chunk][gate][64][4]
  size_t bias_off;            // [layers][4][HT * 16]
  size_t total;               // bytes
};
bool pack_layout(int mode, int I, int H, int layers, PackLayout* p) {
  if (mode < 0 || mode > LR_RNN_TANH || I < 1 || H < 1 || layers < 1 || layers > kMaxLayers) return false;
  if (I > (1 << 20) || H > (1 << 20)) return false;
  const size_t G = gates_of(mode), HT = ((size_t)H + 15) / 16;
  size_t off = 0;
  for (int l = 0; l < layers; ++l) {
    const size_t nchunk = ((size_t)(l == 0 ? I : H) + 15) / 16 + HT;
    p->w_off[l] = off;
    off += lr_align_up(HT * nchunk * G * FRAG * sizeof(float), 256) / sizeof(float);
  }
  p->bias_off = off;
  off += lr_align_up((size_t)layers * 4 * HT * 16 * sizeof(float), 256) / sizeof(float);
  p->total = off * sizeof(float);
  return true;
}

struct WsLayout {
  size_t Hp, hs_off, cs_off, total;   // hs [layers][chunk_T][B][Hp], cs [layers][B][Hp] (LSTM); byte offsets
};
bool ws_layout(int mode, int B, int chunk_T, int I, int H, int layers, int C, WsLayout* w) {
  StateLayout s;
  if (!state_layout(mode, B, H, layers, &s) || I < 1 || chunk_T < 0 || chunk_T > kMaxChunk || C < 0 || C > kMaxClasses)
    return false;
  w->Hp = s.Hp;
  w->hs_off = 0;
  w->cs_off = lr_align_up((size_t)layers * (chunk_T > 0 ? chunk_T : 1) * B * s.Hp * sizeof(float), 256);
  w->total = w->cs_off + (mode == LR_RNN_LSTM ? s.plane_bytes : 0);
  return true;
}

// the slot carries this call's configuration
__device__ __forceinline__ bool slot_ok(const int32_t* __restrict__ hdr, int b, int B, int H, int layers, int cell) {
  const int32_t* h = hdr + (int64_t)b * kHdrWords;
  return h[HD_MAGIC] == kMagic && h[HD_B] == B && h[HD_H] == H && h[HD_LAYERS] == layers && h[HD_CELL] == cell;
}
__device__ __forceinline__ int frames_of(const int32_t* __restrict__ sizes, int b, int chunk_T) {
  if (!sizes) return chunk_T;
  const int n = sizes[b];
  return n < 0 ? 0 : n > chunk_T ? chunk_T : n;
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
  const float* x;         // frame t of the layer's input: row b at x + b * x_sb, I floats
  int64_t x_sb;
  int x_vec;              // rows are 16-byte aligned
  const float* hprev;     // [B][Hp] h_{t-1} (the state at t = 0, else the workspace plane of t - 1)
  const float* cprev;     // LSTM: c_{t-1} likewise
  float* hout;            // [B][Hp] workspace plane of t
  float* cout;            // LSTM: [B][Hp]
  float* y;               // last layer, or NULL: row b at y + b * y_sb
  int64_t y_sb;
  const float* w;         // the layer's fragments
  const float* bias;      // [4][HT * 16]
  const int32_t* hdr;     // the state's headers
  const int32_t* sizes;
  int cell, layers, B, I, H, Hp, t, chunk_T;
};

template <int G>
__global__ __launch_bounds__(NW * 64) void stream_step_kernel(StepArgs p) {
  constexpr int NA = G == 3 ? 4 : G;   // accumulators: GRU r, z, n_x, n_h
  __shared__ float red[NW * NA * TILE * RED_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * TILE, b0 = blockIdx.y * TILE;
  const int H = p.H, Hp = p.Hp, I = p.I, B = p.B;
  const int HTp = gridDim.x * 16;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // ---- epilogue operands first (threads 0..255 own one (slot, hidden unit) each) ------------------------------------
  const int bl = (tid >> 4) & 15, jl = tid & 15;
  const int b = b0 + bl, j = j0 + jl;
  const bool epi = tid < 256 && b < B && j < H;
  float prev_h = 0.f, prev_c = 0.f, bs[4] = {0.f, 0.f, 0.f, 0.f};
  bool active = false;
  if (epi) {
    active = slot_ok(p.hdr, b, B, H, p.layers, p.cell) && p.t < frames_of(p.sizes, b, p.chunk_T);
    prev_h = p.hprev[(int64_t)b * Hp + j];
    if (G == 4) prev_c = p.cprev[(int64_t)b * Hp + j];
#pragma unroll
    for (int g = 0; g < (G == 3 ? 4 : G); ++g) bs[g] = p.bias[g * HTp + j];
  }

  // ---- acc[g] (16 slots x 16 units) += [x_t | h_{t-1}] (16 x K) . [W_ih | W_hh]_g^T (K x 16) ------------------------
  {
    f32x4 acc[NA];
#pragma unroll
    for (int g = 0; g < NA; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int rowi = lane & 15, kq = lane >> 4;
    const int nci = (I + 15) >> 4, nchunk = nci + ((H + 15) >> 4);
    const int ar = b0 + rowi;
    const bool row_in = ar < B;
    const float* xrow = p.x + (int64_t)(row_in ? ar : 0) * p.x_sb;
    const float* hrow = p.hprev + (int64_t)(row_in ? ar : 0) * Hp;
    const float* wsrc = p.w + ((int64_t)blockIdx.x * nchunk) * (G * FRAG) + lane * 4;
    for (int c0 = wave; c0 < nchunk; c0 += NW * UF) {
      float4 a[UF], w[UF][G];
#pragma unroll
      for (int u = 0; u < UF; ++u) {
        const int c = c0 + u * NW;
        const bool ok = c < nchunk;
        a[u] = zero4;
        if (ok && row_in) a[u] = c < nci ? lda(xrow, c * 16 + 4 * kq, I, p.x_vec != 0) : lda(hrow, (c - nci) * 16 + 4 * kq, H, true);
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
    const float n = tanhf((s[2] + bs[2]) + r * (s[NA - 1] + bs[3]));
    h = (1.f - z) * n + z * prev_h;
  } else {
    const float ig = lr_sigmoid(s[0] + bs[0]);
    const float fg = lr_sigmoid(s[1] + bs[1]);
    const float gg = tanhf(s[2] + bs[2]);
    const float og = lr_sigmoid(s[NA - 1] + bs[3]);
    c = fg * prev_c + ig * gg;
    h = og * tanhf(c);
  }
  // an idle slot, or one past its frames, carries its state through bit for bit
  p.hout[(int64_t)b * Hp + j] = active ? h : prev_h;
  if (G == 4) p.cout[(int64_t)b * Hp + j] = active ? c : prev_c;
  if (p.y) p.y[(int64_t)b * p.y_sb + j] = active ? h : 0.f;
}

// The head over 16-row blocks of the chunk (row r = b * chunk_T + t): log_softmax(y W^T + bias + log(mask + 1e-45)),
// wave w owning classes [16 w, 16 w + 16).  A row's arithmetic is one wave's walk over K in rising order, whatever the
// number of rows (lr_proj.hip's fused head has that property only at K % 16 == 0, its GEMM route at no K).  Rows past a
// slot's frames are the zero row.
__global__ __launch_bounds__(1024) void stream_head_kernel(const float* __restrict__ hs, const float* __restrict__ W,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ mask, float* __restrict__ log_probs,
                                                           const int32_t* __restrict__ hdr,
                                                           const int32_t* __restrict__ sizes, int cell, int layers, int B,
                                                           int chunk_T, int H, int Hp, int C, int w_vec) {
  __shared__ float logits[16][kMaxClasses + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int row = lane & 15, q = lane >> 4;
  const int64_t R = (int64_t)B * chunk_T;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int64_t ra = r0 + row;
  bool live = false;
  const float* arow = hs;
  if (ra < R) {
    const int b = (int)(ra / chunk_T), t = (int)(ra - (int64_t)b * chunk_T);
    live = slot_ok(hdr, b, B, H, layers, cell) && t < frames_of(sizes, b, chunk_T);
    arow = hs + ((int64_t)t * B + b) * Hp;
  }
  const int cls = min(16 * wave + row, C - 1);   // classes past C compute a copy of the last one (never stored)
  const float* wrow = W + (int64_t)cls * H;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int steps = (H + 15) >> 4;
  for (int s = 0; s < steps; ++s) {
    const int k = s * 16 + 4 * q;
    const float4 a = live ? lda(arow, k, H, true) : zero4;
    const float4 w = lda(wrow, k, H, w_vec != 0);
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

// The last planes of the chunk -> the state; frames counted (saturating); a slot with another configuration is left
// alone and flagged.  The fields that decide (magic, B, H, layers, cell) are written by a reset only.
__global__ void stream_commit_kernel(int32_t* hdr, float* sh, float* sc, const float* __restrict__ hs_last,
                                     const float* __restrict__ cs, const int32_t* __restrict__ sizes, int cell, int layers,
                                     int B, int chunk_T, int H, int Hp, int64_t layer_stride) {
  const int64_t total = (int64_t)layers * B * Hp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % Hp);
    const int b = (int)((i / Hp) % B);
    const int l = (int)(i / ((int64_t)Hp * B));
    const bool ok = slot_ok(hdr, b, B, H, layers, cell);
    if (ok && j < H) {
      sh[i] = hs_last[(int64_t)l * layer_stride + (int64_t)b * Hp + j];
      if (sc) sc[i] = cs[i];
    }
    if (l == 0 && j == 0) {
      int32_t* h = hdr + (int64_t)b * kHdrWords;
      if (ok) {
        const int64_t f = (int64_t)h[HD_FRAMES] + frames_of(sizes, b, chunk_T);
        h[HD_FRAMES] = f > 0x7fffffff ? 0x7fffffff : (int32_t)f;
      } else {
        h[HD_STATUS] |= LR_RNN_STREAM_MISMATCH;
      }
    }
  }
}

__global__ void stream_reset_kernel(int32_t* hdr, float* sh, float* sc, const int32_t* __restrict__ mask, int cell,
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

__global__ void stream_read_kernel(const int32_t* __restrict__ hdr, const float* __restrict__ sh,
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

// [W_ih | W_hh] of one layer -> fragment-major, zero past I and H:
//   out[(((jt * nchunk + c) * G + g) * 64 + l) * 4 + q] = W[g * H + jt * 16 + (l & 15)][kc * 16 + 4 * (l >> 4) + q]
// with W = W_ih, kc = c for c < nci and W = W_hh, kc = c - nci after.  Any I, H; no alignment asked of the sources.
__global__ void stream_pack_w_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                     float* __restrict__ out, int G, int I, int H) {
  const int HT = (H + 15) >> 4, nci = (I + 15) >> 4, nchunk = nci + HT;
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
        const int k = c * 16 + 4 * (l >> 4) + q;
        if (k < I) v = w_ih[((int64_t)g * H + unit) * I + k];
      } else {
        const int k = (c - nci) * 16 + 4 * (l >> 4) + q;
        if (k < H) v = w_hh[((int64_t)g * H + unit) * H + k];
      }
    }
    out[i] = v;
  }
}

// bias[slot][HT * 16]: b_ih + b_hh per gate; the GRU's n gate keeps b_in in slot 2 and b_hn in slot 3
__global__ void stream_pack_bias_kernel(const float* __restrict__ b_ih, const float* __restrict__ b_hh,
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

extern "C" size_t lr_rnn_stream_pack_bytes(int mode, int I, int H, int layers) {
  PackLayout p;
  return pack_layout(mode, I, H, layers, &p) ? p.total : 0;
}

extern "C" size_t lr_rnn_stream_state_bytes(int mode, int B, int H, int layers) {
  StateLayout s;
  return state_layout(mode, B, H, layers, &s) ? s.total : 0;
}

extern "C" size_t lr_rnn_stream_workspace_bytes(int mode, int B, int chunk_T, int I, int H, int layers, int C) {
  WsLayout w;
  return ws_layout(mode, B, chunk_T, I, H, layers, C, &w) ? w.total : 0;
}

extern "C" int lr_rnn_stream_pack(void* out, size_t out_bytes, int mode, const float* const* w_ih,
                                  const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, int I,
                                  int H, int layers, lr_stream_t stream) {
  LR_CHECK_ARG(out && w_ih && w_hh && b_ih && b_hh);
  LR_CHECK_ARG(I >= 1 && H >= 1 && layers >= 1 && mode >= 0);
  PackLayout p;
  if (!pack_layout(mode, I, H, layers, &p)) return LR_ERR_UNSUPPORTED;
  if (out_bytes < p.total) return LR_ERR_WORKSPACE;
  for (int l = 0; l < layers; ++l) LR_CHECK_ARG(w_ih[l] && w_hh[l] && b_ih[l] && b_hh[l]);
  const int G = gates_of(mode), HT = (H + 15) / 16;
  float* o = (float*)out;
  for (int l = 0; l < layers; ++l) {
    const int Il = l == 0 ? I : H;
    const int64_t total = (int64_t)HT * ((Il + 15) / 16 + HT) * G * FRAG;
    LR_LAUNCH(stream_pack_w_kernel, dim3(blocks_for(total, 256)), dim3(256), 0, stream, w_ih[l], w_hh[l], o + p.w_off[l],
              G, Il, H);
    int st = lr_launch_status();
    if (st != LR_OK) return st;
    LR_LAUNCH(stream_pack_bias_kernel, dim3((4 * HT * 16 + 255) / 256), dim3(256), 0, stream, b_ih[l], b_hh[l],
              o + p.bias_off + (size_t)l * 4 * HT * 16, G, H);
    st = lr_launch_status();
    if (st != LR_OK) return st;
  }
  return LR_OK;
}

extern "C" int lr_rnn_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int mode, int B, int H,
                                   int layers, lr_stream_t stream) {
  LR_CHECK_ARG(state);
  LR_CHECK_ARG(B >= 1 && H >= 1 && layers >= 1 && mode >= 0);
  StateLayout s;
  if (!state_layout(mode, B, H, layers, &s)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total) return LR_ERR_WORKSPACE;
  char* base = (char*)state;
  LR_LAUNCH(stream_reset_kernel, dim3(blocks_for((int64_t)layers * B * s.Hp, 256)), dim3(256), 0, stream, (int32_t*)base,
            (float*)(base + s.h_off), mode == LR_RNN_LSTM ? (float*)(base + s.c_off) : (float*)nullptr, mask, mode, layers, B,
            H, (int)s.Hp);
  return lr_launch_status();
}

extern "C" int lr_rnn_stream_advance(int mode, const float* x, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                     const void* pack, size_t pack_bytes, const float* head_w, const float* head_b,
                                     const float* head_mask, float* y, float* log_probs, void* state, size_t state_bytes,
                                     void* workspace, size_t workspace_bytes, int B, int chunk_T, int I, int H, int layers,
                                     int C, lr_stream_t stream) {
  LR_CHECK_ARG(x && pack && state && workspace);
  LR_CHECK_ARG(B >= 1 && chunk_T >= 0 && I >= 1 && H >= 1 && layers >= 1 && C >= 0 && mode >= 0);
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
      !ws_layout(mode, B, chunk_T, I, H, layers, head ? C : 0, &w))
    return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total || pack_bytes < pk.total || workspace_bytes < w.total) return LR_ERR_WORKSPACE;
  char* sb = (char*)state;
  int32_t* hdr = (int32_t*)sb;
  if (chunk_T == 0) return LR_OK;
  const int Hp = (int)s.Hp, HT = Hp / 16;
  float* sh = (float*)(sb + s.h_off);
  float* sc = mode == LR_RNN_LSTM ? (float*)(sb + s.c_off) : nullptr;
  float* hs = (float*)((char*)workspace + w.hs_off);
  float* cs = mode == LR_RNN_LSTM ? (float*)((char*)workspace + w.cs_off) : nullptr;
  const float* pf = (const float*)pack;
  const int64_t plane = (int64_t)B * Hp, layer_stride = plane * chunk_T;
  const dim3 grid(HT, (B + TILE - 1) / TILE), block(NW * 64);
  const bool x_al = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && stride_b % 4 == 0 && stride_t % 4 == 0;
  for (int l = 0; l < layers; ++l) {
    for (int t = 0; t < chunk_T; ++t) {
      StepArgs a;
      if (l == 0) {
        a.x = x + (int64_t)t * stride_t;
        a.x_sb = stride_b;
        a.x_vec = x_al ? 1 : 0;
        a.I = I;
      } else {
        a.x = hs + (int64_t)(l - 1) * layer_stride + (int64_t)t * plane;
        a.x_sb = Hp;
        a.x_vec = 1;
        a.I = H;
      }
      a.hprev = t == 0 ? sh + (int64_t)l * plane : hs + (int64_t)l * layer_stride + (int64_t)(t - 1) * plane;
      a.hout = hs + (int64_t)l * layer_stride + (int64_t)t * plane;
      a.cprev = cs ? (t == 0 ? sc + (int64_t)l * plane : cs + (int64_t)l * plane) : nullptr;
      a.cout = cs ? cs + (int64_t)l * plane : nullptr;
      a.y = (y && l == layers - 1) ? y + (int64_t)t * H : nullptr;
      a.y_sb = (int64_t)chunk_T * H;
      a.w = pf + pk.w_off[l];
      a.bias = pf + pk.bias_off + (size_t)l * 4 * Hp;
      a.hdr = hdr;
      a.sizes = sizes;
      a.cell = mode;
      a.layers = layers;
      a.B = B;
      a.H = H;
      a.Hp = Hp;
      a.t = t;
      a.chunk_T = chunk_T;
      if (mode == LR_RNN_GRU) LR_LAUNCH(stream_step_kernel<3>, grid, block, 0, stream, a);
      else if (mode == LR_RNN_LSTM) LR_LAUNCH(stream_step_kernel<4>, grid, block, 0, stream, a);
      else LR_LAUNCH(stream_step_kernel<1>, grid, block, 0, stream, a);
      const int st = lr_launch_status();
      if (st != LR_OK) return st;
    }
  }
  if (head) {
    const int64_t R = (int64_t)B * chunk_T;
    const int nw = (C + 15) / 16;
    const int w_vec = H % 4 == 0 && (reinterpret_cast<uintptr_t>(head_w) & 15) == 0;
    LR_LAUNCH(stream_head_kernel, dim3((unsigned)((R + 15) / 16)), dim3(64 * nw), 0, stream,
              (const float*)(hs + (int64_t)(layers - 1) * layer_stride), head_w, head_b, head_mask, log_probs,
              (const int32_t*)hdr, sizes, mode, layers, B, chunk_T, H, Hp, C, w_vec);
    const int st = lr_launch_status();
    if (st != LR_OK) return st;
  }
  LR_LAUNCH(stream_commit_kernel, dim3(blocks_for((int64_t)layers * plane, 256)), dim3(256), 0, stream, hdr, sh, sc,
            (const float*)(hs + (int64_t)(chunk_T - 1) * plane), (const float*)cs, sizes, mode, layers, B, chunk_T, H, Hp,
            layer_stride);
  return lr_launch_status();
}

extern "C" int lr_rnn_stream_read(const void* state, size_t state_bytes, float* h, float* c, int32_t* frames,
                                  int32_t* status, int B, int H, int layers, lr_stream_t stream) {
  LR_CHECK_ARG(state && (h || c || frames || status));
  LR_CHECK_ARG(B >= 1 && H >= 1 && layers >= 1);
  StateLayout s;
  const int mode = c ? LR_RNN_LSTM : LR_RNN_GRU;
  if (!state_layout(mode, B, H, layers, &s)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < s.total) return LR_ERR_WORKSPACE;
  const char* base = (const char*)state;
  LR_LAUNCH(stream_read_kernel, dim3(blocks_for((int64_t)layers * B * H, 256)), dim3(256), 0, stream,
            (const int32_t*)base, (const float*)(base + s.h_off), c ? (const float*)(base + s.c_off) : (const float*)nullptr,
            h, c, frames, status, layers, B, H, (int)s.Hp, c ? 1 : 0);
  return lr_launch_status();
}
