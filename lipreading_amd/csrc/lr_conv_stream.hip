// lr_conv_stream.hip — resumable conv frontend sessions: the three spatio-temporal convolutions (each followed by
// ReLU and a (1,2,2) max-pool) advanced chunk by chunk from a caller-owned state, on gfx950
// (include/lipreading_hip.h lr_conv_stream_*).
//
// Every layer has KT = 3, pt = 1: feature frame t depends on clip frames t-3 .. t+3.  A slot keeps the last TWO input
// frames of every layer (a ring per layer, bf16, zero after a reset — which is the zero padding before frame 0) and
// the counters; an advance computes the frames of every level that the new clip frames complete, once each.
//
//   * levels: level 0 is the clip, level l the pooled output of layer l; a slot with n clip frames has
//     p1 = n or max(0, n-1), p2 = p1 or max(0, p1-1), p3 likewise frames of them (the first value once the stream has
//     ended: the frame after the last one is the zero padding), and p3 feature frames have been emitted.
//   * a PLAN kernel reads the headers, `sizes` and `end` on the device and writes, per (layer, slot, output row), whether
//     the slot produces that frame and where its three input planes are: a ring plane, a plane of this call's new
//     frames in the workspace, or none (zero).  Nothing goes to the host.  It also writes each slot's counters before
//     and after the call, which is what the commit reads (the headers change only there).
//   * the conv kernel is an implicit GEMM on v_mfma_f32_32x32x16_bf16: a workgroup owns 32 GEMM rows x 32 output
//     channels of one (slot, output frame).  The four positions of a pooling window are four consecutive GEMM rows, so
//     that one lane of the C tile holds a window per four registers and relu_pool4 applies unchanged: the pooled frame
//     is all that is written, into the workspace plane the next layer reads (layer 3: the fp32 feature row).
//   * the session's shapes are 1-5 frames of 1-8 slots: latency bound.  So the tile is small (8 windows x 32 channels:
//     72 x 1, 18 x 2, 5 x 3 workgroups per frame at 96 x 96), a lane gathers its own operand fragments straight from
//     global memory (16 bytes = 8 k of one tap; layer 1: two taps of 4 channels) with LR_CS_UF chunks in flight, and the
//     workgroup's four waves split K.
//   * the order of a sum is fixed by the layer alone: k runs over (kt, kh, kw, c); chunk c (16 k) goes to wave c % 4, a
//     wave adds its chunks in rising order, the four partial tiles are added in wave order.  A tap outside the frame, or
//     of a plane that is not there, multiplies zeros.  Neither B, the slot's position, chunk_T nor the cut changes a bit.
//   * plan, ingest, three conv launches, commit, all on the caller's stream: a linear sequence.  No workgroup waits for
//     another, no atomics, every store a plain vector store.  The commit shifts the rings element by element (no
//     rotating index: the state's bytes after given frames do not depend on how they were cut).
#include "lr_common.h"
#include "lr_conv_dev.h"

namespace {

constexpr int32_t kMagic = 0x4c524353;
constexpr int kHdrWords = 8;   // magic, H, W, frames consumed, features emitted, ended, status, 0
enum { HD_MAGIC = 0, HD_H, HD_W, HD_N, HD_EMIT, HD_ENDED, HD_STATUS };
constexpr int kPlanWords = 12;  // before[4], after[4], status bits to set, active, ended after, 0
enum { PL_BEFORE = 0, PL_AFTER = 4, PL_BITS = 8, PL_ACTIVE = 9, PL_ENDED = 10 };
constexpr int kMaxDim = 1024;
constexpr int kMaxZ = 65535;
constexpr int LR_CS_UF = 4;     // chunks (16 k) a wave keeps in flight

struct Layout {
  int h[3], w[3], c[3];        // input of layer l + 1
  size_t plane[3];             // bytes of one input plane, a multiple of 256
  size_t ring_off[3];          // byte offset of a layer's two ring planes inside a slot
  size_t hdr_bytes, slot_bytes, state_total;
};
bool layout(int B, int H, int W, Layout* L) {
  if (B < 1 || B > kMaxZ || H < 16 || W < 16 || H > kMaxDim || W > kMaxDim || H % 16 || W % 16) return false;
  const int div[3] = {1, 4, 8}, ch[3] = {4, 32, 64};
  size_t off = 0;
  for (int l = 0; l < 3; ++l) {
    L->h[l] = H / div[l];
    L->w[l] = W / div[l];
    L->c[l] = ch[l];
    L->plane[l] = lr_align_up((size_t)L->h[l] * L->w[l] * ch[l] * sizeof(bf16_t), 256);
    L->ring_off[l] = off;
    off += 2 * L->plane[l];
  }
  L->slot_bytes = off;
  L->hdr_bytes = lr_align_up((size_t)B * kHdrWords * sizeof(int32_t), 256);
  L->state_total = L->hdr_bytes + (size_t)B * L->slot_bytes;
  return true;
}

struct WsLayout {
  int R;                       // rows of the plan table per slot: chunk_T + 3
  size_t plan_off, table_off, new_off[3], total;
};
bool ws_layout(const Layout& L, int B, int chunk_T, WsLayout* w) {
  if (chunk_T < 0 || (int64_t)B * ((int64_t)chunk_T + 3) > kMaxZ) return false;
  w->R = chunk_T + 3;
  size_t off = 0;
  w->plan_off = off;
  off += lr_align_up((size_t)B * kPlanWords * sizeof(int32_t), 256);
  w->table_off = off;
  off += lr_align_up((size_t)3 * B * w->R * 4 * sizeof(int32_t), 256);
  for (int l = 0; l < 3; ++l) {   // level l gets at most chunk_T + l new frames in one call
    w->new_off[l] = off;
    off += (size_t)B * (chunk_T + l) * L.plane[l];
  }
  w->total = off;
  return true;
}

__device__ __forceinline__ int level_up(int n, bool ended) { return ended ? n : (n > 0 ? n - 1 : 0); }

// One thread per slot writes the slot's plan and counts[b]; then every thread fills entries of the plane table.
__global__ void cs_plan_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ sizes,
                               const int32_t* __restrict__ end, int32_t* __restrict__ plan, int4* __restrict__ table,
                               int32_t* __restrict__ counts, int B, int chunk_T, int H, int W, int R) {
  const int total = 3 * B * R;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int j = i % R, b = (i / R) % B, l = i / (R * B);
    const int32_t* h = hdr + (int64_t)b * kHdrWords;
    const bool cfg = h[HD_MAGIC] == kMagic && h[HD_H] == H && h[HD_W] == W;
    int s = sizes ? sizes[b] : chunk_T;
    s = s < 0 ? 0 : s > chunk_T ? chunk_T : s;
    bool e = end && end[b] != 0;
    const bool was_ended = cfg && h[HD_ENDED] != 0;
    int bits = 0;
    if (!cfg && (s > 0 || e)) bits |= LR_CONV_STREAM_MISMATCH;
    if (was_ended && s > 0) bits |= LR_CONV_STREAM_AFTER_END;
    const bool active = cfg && !was_ended && (s > 0 || e);
    if (!active) {
      s = 0;
      e = false;
    }
    int before[4], after[4];
    before[0] = cfg ? h[HD_N] : 0;
    const int64_t na = (int64_t)before[0] + s;
    after[0] = na > 0x7fffffff ? 0x7fffffff : (int)na;
    const bool ended_after = was_ended || e;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      before[q] = level_up(before[q - 1], was_ended);
      after[q] = level_up(after[q - 1], ended_after);
    }
    if (l == 0 && j == 0) {
      int32_t* p = plan + (int64_t)b * kPlanWords;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        p[PL_BEFORE + q] = before[q];
        p[PL_AFTER + q] = after[q];
      }
      p[PL_BITS] = bits;
      p[PL_ACTIVE] = active ? 1 : 0;
      p[PL_ENDED] = ended_after ? 1 : 0;
      p[11] = 0;
      if (counts) counts[b] = after[3] - before[3];
    }
    // output frame t of layer l + 1 reads frames t - 1, t, t + 1 of level l
    const int t = before[l + 1] + j;
    int4 ent = make_int4(0, -1, -1, -1);
    if (active && t < after[l + 1]) {
      ent.x = 1;
      int src[3];
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) {
        const int g = t - 1 + kt;
        int code = -1;
        if (g >= 0 && g < after[l]) {
          if (g >= before[l]) {
            const int k = g - before[l];
            if (k < chunk_T + l) code = 2 + k;
          } else {
            const int r = g - (before[l] - 2);
            if (r == 0 || r == 1) code = r;
          }
        }
        src[kt] = code;
      }
      ent.y = src[0];
      ent.z = src[1];
      ent.w = src[2];
    }
    table[i] = ent;
  }
}

// x (B, chunk_T, 3, H, W) uint8 (scaled by 1/255) or fp32 -> workspace planes [B][chunk_T][H][W][4] bf16, 4th channel 0
__global__ void cs_ingest_kernel(const void* __restrict__ x, int is_f32, int64_t stride_b, int64_t stride_t,
                                 unsigned char* __restrict__ out, size_t plane_bytes, int B, int chunk_T, int H, int W) {
  const int64_t hw = (int64_t)H * W, total = (int64_t)B * chunk_T * hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = i / hw, p = i - f * hw;
    const int b = (int)(f / chunk_T), t = (int)(f - (int64_t)b * chunk_T);
    const int64_t src = (int64_t)b * stride_b + (int64_t)t * stride_t + p;
    float c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      c[ch] = is_f32 ? ((const float*)x)[src + ch * hw] : (float)((const unsigned char*)x)[src + ch * hw] * (1.f / 255.f);
    uint2 v;
    v.x = (unsigned)f2bf(c[0]) | ((unsigned)f2bf(c[1]) << 16);
    v.y = (unsigned)f2bf(c[2]);
    *reinterpret_cast<uint2*>(out + (size_t)f * plane_bytes + (size_t)p * 8) = v;
  }
}

struct ConvArgs {
  const int4* table;            // this layer's [B][R] entries
  const unsigned char* ring;    // state + header bytes + the layer's ring offset; slot b at + b * slot_bytes
  const unsigned char* newin;   // workspace planes of this call's new input frames: [B][nin]
  unsigned char* out;           // workspace planes of the next level [B][nout] (bf16), or feat [B][zr][F] fp32
  const bf16_t* wp;             // [COUT][taps][CIN]
  const float* bias;
  size_t slot_bytes, in_plane, out_plane;
  int Hin, Win, R, zr, nin, nout;
};

template <int CIN, int COUT, int KH, int KW, int STRIDE, int PAD, bool LAST>
__global__ __launch_bounds__(256) void cs_conv_kernel(ConvArgs p) {
  constexpr int KTOT = 3 * KH * KW * CIN;
  constexpr int NCHUNK = (KTOT + 15) / 16;
  constexpr int TAPS = 3 * KH * KW;
  __shared__ float red[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z / p.zr, j = blockIdx.z - b * p.zr;
  const int4 ent = p.table[(int64_t)b * p.R + j];
  const int Hp = p.Hin / (2 * STRIDE), Wp = p.Win / (2 * STRIDE), NP = Hp * Wp;
  // epilogue coordinates: one (window, channel) per thread
  const int ewin = blockIdx.x * 8 + (tid >> 5), en = blockIdx.y * 32 + (tid & 31);
  if (!ent.x) {   // the slot does not produce this frame
    if (LAST && ewin < NP)
      reinterpret_cast<float*>(p.out)[((int64_t)b * p.zr + j) * ((int64_t)NP * COUT) + (int64_t)ewin * COUT + en] = 0.f;
    return;
  }
  auto plane_of = [&](int c) -> const unsigned char* {
    return c < 0 ? nullptr
           : c < 2 ? p.ring + (size_t)b * p.slot_bytes + (size_t)c * p.in_plane
                   : p.newin + ((size_t)b * p.nin + (size_t)(c - 2)) * p.in_plane;
  };
  const unsigned char* const pl0 = plane_of(ent.y);
  const unsigned char* const pl1 = plane_of(ent.z);
  const unsigned char* const pl2 = plane_of(ent.w);
  // this lane's GEMM row: window (row >> 2), position (row & 3) in the window, row-major
  const int lr = lane & 31, lk = lane >> 5;
  const int row = blockIdx.x * 32 + lr, win = row >> 2, pos = row & 3;
  const bool rowok = win < NP;
  const int php = rowok ? win / Wp : 0, pwp = rowok ? win - php * Wp : 0;
  const int hi0 = (2 * php + (pos >> 1)) * STRIDE - PAD, wi0 = (2 * pwp + (pos & 1)) * STRIDE - PAD;
  const bf16_t* wrow = p.wp + (int64_t)(blockIdx.y * 32 + lr) * KTOT;

  auto gather = [&](int tap, int ch) -> const unsigned char* {   // address of (tap, ch) for this row, or null
    const int kw = tap % KW, kh = (tap / KW) % KH, kt = tap / (KW * KH);
    const unsigned char* base = kt == 0 ? pl0 : kt == 1 ? pl1 : pl2;
    const int hi = hi0 + kh, wi = wi0 + kw;
    if (!rowok || !base || hi < 0 || hi >= p.Hin || wi < 0 || wi >= p.Win) return nullptr;
    return base + (((size_t)hi * p.Win + wi) * CIN + ch) * sizeof(bf16_t);
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int c0 = wave; c0 < NCHUNK; c0 += 4 * LR_CS_UF) {
    uint4 a[LR_CS_UF], w[LR_CS_UF];
#pragma unroll
    for (int u = 0; u < LR_CS_UF; ++u) {
      const int c = c0 + 4 * u;
      const int k = c * 16 + lk * 8;
      a[u] = make_uint4(0u, 0u, 0u, 0u);
      w[u] = make_uint4(0u, 0u, 0u, 0u);
      if (c < NCHUNK) {   // wave-uniform
        if (CIN >= 8) {
          const unsigned char* src = gather(k / CIN, k % CIN);
          if (src) a[u] = *reinterpret_cast<const uint4*>(src);
          w[u] = *reinterpret_cast<const uint4*>(wrow + k);
        } else {          // two taps of four channels; the last chunk ends inside the row
          const int tap = k / 4;
          if (tap < TAPS) {
            const unsigned char* src = gather(tap, 0);
            const uint2 v = src ? *reinterpret_cast<const uint2*>(src) : make_uint2(0u, 0u);
            const uint2 ww = *reinterpret_cast<const uint2*>(wrow + k);
            a[u].x = v.x, a[u].y = v.y;
            w[u].x = ww.x, w[u].y = ww.y;
          }
          if (tap + 1 < TAPS) {
            const unsigned char* src = gather(tap + 1, 0);
            const uint2 v = src ? *reinterpret_cast<const uint2*>(src) : make_uint2(0u, 0u);
            const uint2 ww = *reinterpret_cast<const uint2*>(wrow + k + 4);
            a[u].z = v.x, a[u].w = v.y;
            w[u].z = ww.x, w[u].w = ww.y;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < LR_CS_UF; ++u)
      if (c0 + 4 * u < NCHUNK)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[u]), __builtin_bit_cast(bf16x8, w[u]),
                                                      acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
  __syncthreads();
  // C/D layout of 32x32x16: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5): window q of the tile is
  // registers 4 * (q >> 1) .. + 3 of lane (q & 1) * 32 + col
  const int q = tid >> 5, el = (q & 1) * 32 + (tid & 31), r0 = 4 * (q >> 1);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = ((red[0][r0 + i][el] + red[1][r0 + i][el]) + red[2][r0 + i][el]) + red[3][r0 + i][el];
  bf16_t best;
  int arg;
  relu_pool4(v[0], v[1], v[2], v[3], p.bias[en], best, arg);
  if (ewin >= NP) return;
  if (LAST)
    reinterpret_cast<float*>(p.out)[((int64_t)b * p.zr + j) * ((int64_t)NP * COUT) + (int64_t)ewin * COUT + en] = bf2f(best);
  else
    *reinterpret_cast<bf16_t*>(p.out + ((size_t)b * p.nout + j) * p.out_plane + ((size_t)ewin * COUT + en) * sizeof(bf16_t)) = best;
}

// Rings <- the last two frames of (ring, this call's new frames), element by element; then the counters.
struct CommitArgs {
  unsigned char* state;
  const unsigned char* ws;
  const int32_t* plan;
  size_t hdr_bytes, slot_bytes, plane[3], ring_off[3], new_off[3];
  int B, chunk_T;
};
__global__ void cs_commit_kernel(CommitArgs p) {
  const int64_t units = (int64_t)(p.plane[0] + p.plane[1] + p.plane[2]) / 16;
  const int64_t total = (int64_t)p.B * units;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / units);
    int64_t u = i - (int64_t)b * units;
    int l = 0;
    if (u >= (int64_t)p.plane[0] / 16) {
      u -= p.plane[0] / 16;
      l = 1;
      if (u >= (int64_t)p.plane[1] / 16) {
        u -= p.plane[1] / 16;
        l = 2;
      }
    }
    const int32_t* pb = p.plan + (int64_t)b * kPlanWords;
    if (!pb[PL_ACTIVE]) continue;
    const int c = pb[PL_AFTER + l] - pb[PL_BEFORE + l];   // new frames of level l: 0 .. chunk_T + l
    if (c <= 0) continue;
    uint4* r0 = reinterpret_cast<uint4*>(p.state + p.hdr_bytes + (size_t)b * p.slot_bytes + p.ring_off[l]) + u;
    uint4* r1 = reinterpret_cast<uint4*>(p.state + p.hdr_bytes + (size_t)b * p.slot_bytes + p.ring_off[l] + p.plane[l]) + u;
    const unsigned char* nb = p.ws + p.new_off[l] + (size_t)b * (p.chunk_T + l) * p.plane[l];
    const uint4 last = *(reinterpret_cast<const uint4*>(nb + (size_t)(c - 1) * p.plane[l]) + u);
    const uint4 prev = c >= 2 ? *(reinterpret_cast<const uint4*>(nb + (size_t)(c - 2) * p.plane[l]) + u) : *r1;
    *r0 = prev;
    *r1 = last;
  }
}
__global__ void cs_commit_hdr_kernel(int32_t* hdr, const int32_t* __restrict__ plan, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int32_t* pb = plan + (int64_t)b * kPlanWords;
  int32_t* h = hdr + (int64_t)b * kHdrWords;
  if (pb[PL_BITS]) h[HD_STATUS] |= pb[PL_BITS];
  if (pb[PL_ACTIVE]) {
    h[HD_N] = pb[PL_AFTER + 0];
    h[HD_EMIT] = pb[PL_AFTER + 3];
    h[HD_ENDED] = pb[PL_ENDED];
  }
}

__global__ void cs_reset_kernel(unsigned char* state, const int32_t* __restrict__ mask, size_t hdr_bytes,
                                size_t slot_bytes, int B, int H, int W) {
  const int64_t units = (int64_t)slot_bytes / 16;
  const int64_t total = (int64_t)B * units;
  int32_t* hdr = reinterpret_cast<int32_t*>(state);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / units);
    const int64_t u = i - (int64_t)b * units;
    if (mask && mask[b] == 0) continue;
    int32_t* h = hdr + (int64_t)b * kHdrWords;
    // (the fields that decide are written by an unmasked reset only, in the header launch that follows this one)
    const bool ok = !mask || (h[HD_MAGIC] == kMagic && h[HD_H] == H && h[HD_W] == W);
    if (ok) *(reinterpret_cast<uint4*>(state + hdr_bytes + (size_t)b * slot_bytes) + u) = make_uint4(0u, 0u, 0u, 0u);
  }
}
__global__ void cs_reset_hdr_kernel(int32_t* hdr, const int32_t* __restrict__ mask, int B, int H, int W) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || (mask && mask[b] == 0)) return;
  int32_t* h = hdr + (int64_t)b * kHdrWords;
  if (!mask) {
    h[HD_MAGIC] = kMagic;
    h[HD_H] = H;
    h[HD_W] = W;
    h[7] = 0;
  } else if (!(h[HD_MAGIC] == kMagic && h[HD_H] == H && h[HD_W] == W)) {
    h[HD_STATUS] |= LR_CONV_STREAM_MISMATCH;
    return;
  }
  h[HD_N] = 0;
  h[HD_EMIT] = 0;
  h[HD_ENDED] = 0;
  h[HD_STATUS] = 0;
}

__global__ void cs_read_kernel(const int32_t* __restrict__ hdr, int32_t* __restrict__ frames,
                               int32_t* __restrict__ emitted, int32_t* __restrict__ ended, int32_t* __restrict__ status,
                               int B, int H, int W) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int32_t* h = hdr + (int64_t)b * kHdrWords;
  const bool ok = h[HD_MAGIC] == kMagic && h[HD_H] == H && h[HD_W] == W;
  if (frames) frames[b] = ok ? h[HD_N] : 0;
  if (emitted) emitted[b] = ok ? h[HD_EMIT] : 0;
  if (ended) ended[b] = ok ? h[HD_ENDED] : 0;
  if (status) status[b] = ok ? h[HD_STATUS] : (h[HD_MAGIC] == kMagic ? h[HD_STATUS] : 0) | LR_CONV_STREAM_MISMATCH;
}

unsigned blocks_for(int64_t n, int threads) {
  int64_t b = (n + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : b > 65535 ? 65535 : b);
}

}  // namespace

extern "C" size_t lr_conv_stream_state_bytes(int B, int H, int W) {
  Layout L;
  return layout(B, H, W, &L) ? L.state_total : 0;
}

extern "C" size_t lr_conv_stream_workspace_bytes(int B, int chunk_T, int H, int W) {
  Layout L;
  WsLayout w;
  return layout(B, H, W, &L) && ws_layout(L, B, chunk_T, &w) ? w.total : 0;
}

extern "C" int lr_conv_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int B, int H, int W,
                                    lr_stream_t stream) {
  LR_CHECK_ARG(state);
  LR_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H % 16 == 0 && W % 16 == 0);
  LR_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 15) == 0);
  Layout L;
  if (!layout(B, H, W, &L)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < L.state_total) return LR_ERR_WORKSPACE;
  LR_LAUNCH(cs_reset_kernel, dim3(blocks_for((int64_t)B * (int64_t)(L.slot_bytes / 16), 256)), dim3(256), 0, stream,
            (unsigned char*)state, mask, L.hdr_bytes, L.slot_bytes, B, H, W);
  int st = lr_launch_status();
  if (st != LR_OK) return st;
  LR_LAUNCH(cs_reset_hdr_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, (int32_t*)state, mask, B, H, W);
  return lr_launch_status();
}

extern "C" int lr_conv_stream_advance(const void* x, int flags, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                      const int32_t* end, const void* w1, const void* w2, const void* w3,
                                      const float* bias1, const float* bias2, const float* bias3, float* feat,
                                      int32_t* counts, void* state, size_t state_bytes, void* workspace,
                                      size_t workspace_bytes, int B, int chunk_T, int H, int W, lr_stream_t stream) {
  LR_CHECK_ARG(state && workspace && w1 && w2 && w3 && bias1 && bias2 && bias3);
  LR_CHECK_ARG(B >= 1 && chunk_T >= 0 && H >= 1 && W >= 1 && H % 16 == 0 && W % 16 == 0);
  LR_CHECK_ARG((flags & ~LR_CONV_STREAM_F32) == 0 && stride_b >= 0 && stride_t >= 0);
  LR_CHECK_ARG(chunk_T == 0 || x);
  LR_CHECK_ARG(((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(workspace) |
                 reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(w3)) &
                15) == 0);
  if (flags & LR_CONV_STREAM_F32) LR_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3) == 0);
  const int rows = chunk_T + (end ? 3 : 0);
  LR_CHECK_ARG(rows == 0 || (feat && counts));
  Layout L;
  WsLayout ws;
  if (!layout(B, H, W, &L) || !ws_layout(L, B, chunk_T, &ws)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < L.state_total || workspace_bytes < ws.total) return LR_ERR_WORKSPACE;
  if (rows == 0) return LR_OK;
  unsigned char* sb = (unsigned char*)state;
  unsigned char* wb = (unsigned char*)workspace;
  int32_t* plan = (int32_t*)(wb + ws.plan_off);
  int4* table = (int4*)(wb + ws.table_off);
  int st;
  LR_LAUNCH(cs_plan_kernel, dim3(blocks_for((int64_t)3 * B * ws.R, 256)), dim3(256), 0, stream, (const int32_t*)sb, sizes,
            end, plan, table, counts, B, chunk_T, H, W, ws.R);
  if ((st = lr_launch_status()) != LR_OK) return st;
  if (chunk_T > 0) {
    LR_LAUNCH(cs_ingest_kernel, dim3(blocks_for((int64_t)B * chunk_T * H * W, 256)), dim3(256), 0, stream, x,
              (flags & LR_CONV_STREAM_F32) ? 1 : 0, stride_b, stride_t, wb + ws.new_off[0], L.plane[0], B, chunk_T, H, W);
    if ((st = lr_launch_status()) != LR_OK) return st;
  }
  const void* wp[3] = {w1, w2, w3};
  const float* bias[3] = {bias1, bias2, bias3};
  for (int l = 0; l < 3; ++l) {
    ConvArgs a;
    a.table = table + (size_t)l * B * ws.R;
    a.ring = sb + L.hdr_bytes + L.ring_off[l];
    a.newin = wb + ws.new_off[l];
    a.wp = (const bf16_t*)wp[l];
    a.bias = bias[l];
    a.slot_bytes = L.slot_bytes;
    a.in_plane = L.plane[l];
    a.Hin = L.h[l];
    a.Win = L.w[l];
    a.R = ws.R;
    a.nin = chunk_T + l;
    // a layer's new output frames: at most its new input frames, one more when the stream ends
    a.zr = l == 2 ? rows : chunk_T + (end ? l + 1 : 0);
    if (l < 2) {
      a.out = wb + ws.new_off[l + 1];
      a.out_plane = L.plane[l + 1];
      a.nout = chunk_T + l + 1;
    } else {
      a.out = (unsigned char*)feat;
      a.out_plane = 0;
      a.nout = 0;
    }
    if (a.zr == 0) continue;
    const int stride = l == 0 ? 2 : 1;
    const int np = (a.Hin / (2 * stride)) * (a.Win / (2 * stride));
    const dim3 grid((np + 7) / 8, l + 1, (unsigned)(B * a.zr));
    if (l == 0) LR_LAUNCH((cs_conv_kernel<4, 32, 5, 5, 2, 2, false>), grid, dim3(256), 0, stream, a);
    else if (l == 1) LR_LAUNCH((cs_conv_kernel<32, 64, 5, 5, 1, 2, false>), grid, dim3(256), 0, stream, a);
    else LR_LAUNCH((cs_conv_kernel<64, 96, 3, 3, 1, 1, true>), grid, dim3(256), 0, stream, a);
    if ((st = lr_launch_status()) != LR_OK) return st;
  }
  CommitArgs c;
  c.state = sb;
  c.ws = wb;
  c.plan = plan;
  c.hdr_bytes = L.hdr_bytes;
  c.slot_bytes = L.slot_bytes;
  for (int l = 0; l < 3; ++l) {
    c.plane[l] = L.plane[l];
    c.ring_off[l] = L.ring_off[l];
    c.new_off[l] = ws.new_off[l];
  }
  c.B = B;
  c.chunk_T = chunk_T;
  LR_LAUNCH(cs_commit_kernel, dim3(blocks_for((int64_t)B * (int64_t)(L.slot_bytes / 32), 256)), dim3(256), 0, stream, c);
  if ((st = lr_launch_status()) != LR_OK) return st;
  LR_LAUNCH(cs_commit_hdr_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, (int32_t*)sb, (const int32_t*)plan, B);
  return lr_launch_status();
}

extern "C" int lr_conv_stream_read(const void* state, size_t state_bytes, int32_t* frames, int32_t* emitted,
                                   int32_t* ended, int32_t* status, int B, int H, int W, lr_stream_t stream) {
  LR_CHECK_ARG(state && (frames || emitted || ended || status));
  LR_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && H % 16 == 0 && W % 16 == 0);
  Layout L;
  if (!layout(B, H, W, &L)) return LR_ERR_UNSUPPORTED;
  if (state_bytes < L.state_total) return LR_ERR_WORKSPACE;
  LR_LAUNCH(cs_read_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, (const int32_t*)state, frames, emitted, ended,
            status, B, H, W);
  return lr_launch_status();
}
