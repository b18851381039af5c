// Stabilised, roll-corrected mouth crops inside the collate launch (lr_lip_stable_collate_u8; the specification is the
// header's, DESIGN.md "Stabilised crop" has the measurements).
//
// Two launches.  stable_pose_kernel: one workgroup per sample; a thread takes the raw pose of a row (mouth mean, eye
// vector: float64 sums in ascending index) into the workspace, and after the workgroup's barrier the same thread
// averages the raw poses of the row's neighbours, again in float64 and in ascending order, into the second half of the
// workspace (and into `pose`).  stable_window_kernel: lip_augment_collate_kernel's structure (lr_misc.hip) — 256
// threads, a capped grid striding over the B * t_max (sample, frame) pairs, V = 16 / 4 / 1 pixels per store, the next
// pair's prologue loads issued before this pair's pixels, the flip as a mirrored store — with two differences.  The
// prologue is one 16-byte load of the smoothed pose where the box rule reduces twenty landmarks, and every address in
// it is uniform, so each lane takes the window for itself: no LDS slot, no barrier.  And a rolled window's four taps
// do not sit on two source rows per output row, so both source coordinates are made per pixel.
//
// The bilinear tail is lip_crop_pixel's (lr_misc.hip), restated here: that file's kernels and their resources are
// pinned by tests and stay as they are.
#include "lr_common.h"

namespace {
struct StablePose { float mx, my, ax, ay; };

// mean of x and y over landmarks [lo, hi) of one row: float64 sums in ascending index, one rounding to fp32
__device__ __forceinline__ void stable_mean(const float* __restrict__ L, int lo, int hi, float& x, float& y) {
  double sx = 0.0, sy = 0.0;
  for (int p = lo; p < hi; ++p) {
    sx += (double)L[p * 3];
    sy += (double)L[p * 3 + 1];
  }
  const double n = (double)(hi - lo);
  x = (float)(sx / n);
  y = (float)(sy / n);
}

// raw [rows][4] and smooth [rows][4] are the two halves of the workspace.  The rows of sample b are this workgroup's
// alone: what one thread writes to raw before the barrier, another reads after it.
__global__ __launch_bounds__(256) void stable_pose_kernel(const float* __restrict__ lmk,
                                                          const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ lens, float4* raw, float4* smooth,
                                                          float* pose, int64_t rows, int npts, int lo, int hi, int ea_lo,
                                                          int ea_hi, int eb_lo, int eb_hi, int radius) {
  const int b = blockIdx.x;
  const int64_t first = offsets[b];
  int len = lens[b];
  if (first < 0 || first >= rows || len <= 0) return;      // uniform; never outside the workspace
  len = (int)min((int64_t)len, rows - first);
  for (int i = threadIdx.x; i < len; i += blockDim.x) {
    const float* L = lmk + (first + i) * npts * 3;
    float mx, my, ax0, ay0, ax1, ay1;
    stable_mean(L, lo, hi, mx, my);
    stable_mean(L, ea_lo, ea_hi, ax0, ay0);
    stable_mean(L, eb_lo, eb_hi, ax1, ay1);
    raw[first + i] = make_float4(mx, my, ax1 - ax0, ay1 - ay0);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < len; i += blockDim.x) {
    const int j0 = max(0, i - radius), j1 = min(len - 1, i + radius);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int j = j0; j <= j1; ++j) {
      const float4 r = raw[first + j];
      s0 += (double)r.x; s1 += (double)r.y; s2 += (double)r.z; s3 += (double)r.w;
    }
    const double n = (double)(j1 - j0 + 1);
    const float4 s = make_float4((float)(s0 / n), (float)(s1 / n), (float)(s2 / n), (float)(s3 / n));
    smooth[first + i] = s;
    if (pose) {
      float* P = pose + (first + i) * 4;
      P[0] = s.x; P[1] = s.y; P[2] = s.z; P[3] = s.w;
    }
  }
}

template <int V> struct StableVec;
template <> struct StableVec<1> { typedef unsigned char T; };
template <> struct StableVec<4> { typedef uint32_t T; };
template <> struct StableVec<16> { typedef uint4 T; };

// the bytes of a group in reverse order when flip is set (sel: v_perm's byte selector, identity or reversed)
__device__ __forceinline__ unsigned char stable_vec_mirror(unsigned char v, bool, uint32_t) { return v; }
__device__ __forceinline__ uint32_t stable_vec_mirror(uint32_t v, bool, uint32_t sel) {
  return __builtin_amdgcn_perm(v, v, sel);
}
__device__ __forceinline__ uint4 stable_vec_mirror(uint4 v, bool flip, uint32_t sel) {
  const uint32_t a = __builtin_amdgcn_perm(v.x, v.x, sel), b = __builtin_amdgcn_perm(v.y, v.y, sel);
  const uint32_t c = __builtin_amdgcn_perm(v.z, v.z, sel), d = __builtin_amdgcn_perm(v.w, v.w, sel);
  return make_uint4(flip ? d : a, flip ? c : b, flip ? b : c, flip ? a : d);
}

// the sample at (sx, sy) of the plane P [H][W]: lip_crop_pixel's arithmetic from its clamp onwards
__device__ __forceinline__ unsigned char stable_tap(const unsigned char* __restrict__ P, int H, int W, float sx, float sy) {
  sx = fminf(fmaxf(sx, 0.f), (float)(W - 1));
  sy = fminf(fmaxf(sy, 0.f), (float)(H - 1));
  const int ix = (int)floorf(sx), iy = (int)floorf(sy);
  const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
  const float fx = sx - (float)ix, fy = sy - (float)iy;
  const float a = (float)P[iy * W + ix], b = (float)P[iy * W + ix1];
  const float d = (float)P[iy1 * W + ix], e = (float)P[iy1 * W + ix1];
  const float top_v = fmaf(b - a, fx, a), bot_v = fmaf(e - d, fx, d);
  const float v = fmaf(bot_v - top_v, fy, top_v);
  return (unsigned char)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
}

// The 16- and 1-pixel variants take 42 and 34 VGPRs.  The 4-pixel one, its four pixels unrolled, takes 76 (six waves per
// SIMD): it makes them one after the other, which holds it at 60.  (Asking for eight waves in the launch bounds
// spills SGPRs in all three instead.)
template <int V>
__global__ __launch_bounds__(256) void stable_window_kernel(
    const unsigned char* __restrict__ frames, const float4* __restrict__ smooth, const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ lens, const float* __restrict__ clip_aug, const int32_t* __restrict__ tmap,
    unsigned char* __restrict__ out, int B, int64_t rows, int t_max, int H, int W, int S, float extent) {
  typedef typename StableVec<V>::T vec_t;
  const int per_row = S / V;                 // S % V == 0 (the launcher picks V)
  const int items = 3 * S * per_row;         // V-pixel groups of one frame
  const int pairs = B * t_max;
  const float half = 0.5f * (float)S;
  int p = blockIdx.x;                        // (sample, frame) pairs p, p + gridDim.x, ...: uniform per workgroup
  if (p >= pairs) return;
  // the pair whose prologue loads are in flight: its map value (< 0: a frame of zeros), source row, record and pose
  int m;
  int64_t n;
  float dx = 0.f, dy = 0.f, zoom = 1.f, flipf = 0.f;
  float4 ps;
  auto fetch = [&](int q) {
    const int b = q / t_max, t = q - b * t_max;
    const int rows_b = lens[b];
    const int len = min(rows_b, t_max);      // lens[b] > t_max is the caller's error; never write outside out
    const int64_t first = offsets[b];
    if (clip_aug) {                          // (and tmap: both or neither)
      const float* A = clip_aug + (int64_t)b * 4;
      dx = A[0]; dy = A[1]; zoom = A[2]; flipf = A[3];
      m = t < len ? tmap[first + t] : -1;
    } else {
      m = t < len ? t : -1;
    }
    n = first + min(max(m, 0), rows_b - 1);  // whatever the map holds, the row is one of sample b's
    n = min(max(n, (int64_t)0), rows - 1);   // and whatever offsets and lens hold, one of the workspace's
    ps = smooth[n];
  };
  fetch(p);
  for (;;) {
    const int m_now = m;
    const bool flip = flipf != 0.f;
    const unsigned char* F = frames + n * 3 * H * W;
    vec_t* O = reinterpret_cast<vec_t*>(out + (int64_t)p * 3 * S * S);
    // the window (every lane for itself: all of it is uniform)
    float ax = ps.z, ay = ps.w;
    const float d = sqrtf(fmaf(ay, ay, ax * ax));
    if (!(extent * d * zoom >= 2.f)) {       // the 2-pixel minimum side; coincident eye points; NaN
      ax = 2.f / (extent * zoom);
      ay = 0.f;
    }
    const float ex = extent * ax, ey = extent * ay;
    const float cx = fmaf(-dy, ey, fmaf(dx, ex, ps.x));
    const float cy = fmaf(dy, ex, fmaf(dx, ey, ps.y));
    const float ux = (ex * zoom) / (float)S, uy = (ey * zoom) / (float)S;
    const int p_next = p + gridDim.x;
    if (p_next < pairs) fetch(p_next);       // in flight while this frame's pixels are made
    if (m_now < 0) {                         // padding or a masked frame
      vec_t zero;
      __builtin_memset(&zero, 0, sizeof(zero));
      for (int i = threadIdx.x; i < items; i += blockDim.x) O[i] = zero;
    } else {
      // mirrored, output column S - 1 - x shows source column x: group g is stored at group per_row - 1 - g with its
      // bytes reversed
      const int mirror = flip ? 1 : 0;
      const uint32_t sel = flip ? 0x00010203u : 0x03020100u;
      for (int i = threadIdx.x; i < items; i += blockDim.x) {
        const int c = i / (S * per_row), r = i - c * S * per_row;
        const int oy = r / per_row, g = r - oy * per_row, ox = g * V;
        const unsigned char* P = F + (int64_t)c * H * W;
        const float py = ((float)oy + 0.5f) - half;
        // (the specification adds the row's share LAST, so it cannot be hoisted out of the group)
        auto pixel = [&](int k) {
          const float px = ((float)(ox + k) + 0.5f) - half;
          const float sx = fmaf(-py, uy, fmaf(px, ux, cx)) - 0.5f;
          const float sy = fmaf(py, ux, fmaf(px, uy, cy)) - 0.5f;
          return stable_tap(P, H, W, sx, sy);
        };
        vec_t v;
        if constexpr (V == 4) {              // one pixel after the other (see above)
          uint32_t w = 0;
#pragma unroll 1
          for (int k = 0; k < 4; ++k) w |= (uint32_t)pixel(k) << (8 * k);
          v = w;
        } else {
          union { vec_t v; unsigned char px[V]; } u;
#pragma unroll
          for (int k = 0; k < V; ++k) u.px[k] = pixel(k);
          v = u.v;
        }
        O[i + mirror * (per_row - 1 - 2 * g)] = stable_vec_mirror(v, flip, sel);
      }
    }
    if (p_next >= pairs) break;
    p = p_next;
  }
}
}  // namespace

extern "C" size_t lr_lip_stable_workspace_bytes(int64_t rows, int radius) {
  if (rows <= 0 || rows > ((int64_t)1 << 40) || radius < 0 || radius > LR_LIP_STABLE_MAX_RADIUS) return 0;
  return lr_align_up((size_t)rows * 2 * sizeof(float4), 256);   // raw and smoothed poses
}

extern "C" int lr_lip_stable_collate_u8(const void* frames, const float* lmk, const int64_t* offsets, const int32_t* lens,
                                        const float* clip_aug, const int32_t* tmap, void* out, float* pose,
                                        void* workspace, size_t workspace_bytes, int B, int64_t rows, int t_max, int H,
                                        int W, int S, int npts, int lo, int hi, int ea_lo, int ea_hi, int eb_lo, int eb_hi,
                                        float extent, int radius, lr_stream_t stream) {
  LR_CHECK_ARG(frames && lmk && offsets && lens && out && workspace);
  LR_CHECK_ARG((clip_aug == nullptr) == (tmap == nullptr));
  LR_CHECK_ARG(B > 0 && rows > 0 && t_max > 0 && H > 0 && W > 0 && S > 0);
  LR_CHECK_ARG(npts > 0 && lo >= 0 && hi > lo && hi <= npts);
  LR_CHECK_ARG(ea_lo >= 0 && ea_hi > ea_lo && ea_hi <= npts && eb_lo >= 0 && eb_hi > eb_lo && eb_hi <= npts);
  LR_CHECK_ARG(extent > 0.f && isfinite(extent));
  LR_CHECK_ARG(radius >= 0 && radius <= LR_LIP_STABLE_MAX_RADIUS);
  LR_CHECK_ARG((int64_t)B * t_max <= INT32_MAX && (int64_t)S * S <= INT32_MAX / 3);   // as lr_lip_crop_collate_aug_u8
  LR_CHECK_ARG((int64_t)H * W <= INT32_MAX / 3);                                     // a tap's index is an int
  const size_t need = lr_lip_stable_workspace_bytes(rows, radius);
  LR_CHECK_ARG(need > 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  if (workspace_bytes < need) return LR_ERR_WORKSPACE;
  float4* raw = (float4*)workspace;
  float4* smooth = raw + rows;
  LR_LAUNCH(stable_pose_kernel, dim3(B), dim3(256), 0, stream, lmk, offsets, lens, raw, smooth, pose, rows, npts, lo, hi,
            ea_lo, ea_hi, eb_lo, eb_hi, radius);
  const int st = lr_launch_status();
  if (st != LR_OK) return st;
  const int pairs = B * t_max;
  const dim3 grid(pairs < 2048 ? pairs : 2048);   // 256 CUs x 8 workgroups; the rest by the grid stride
  const unsigned char* f = (const unsigned char*)frames;
  unsigned char* o = (unsigned char*)out;
  // a frame of out starts at a multiple of 3 * S * S bytes: vector stores need S % V == 0 and an aligned base
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (aligned && S % 16 == 0) {
    LR_LAUNCH(stable_window_kernel<16>, grid, dim3(256), 0, stream, f, smooth, offsets, lens, clip_aug, tmap, o, B, rows,
              t_max, H, W, S, extent);
  } else if (aligned && S % 4 == 0) {
    LR_LAUNCH(stable_window_kernel<4>, grid, dim3(256), 0, stream, f, smooth, offsets, lens, clip_aug, tmap, o, B, rows,
              t_max, H, W, S, extent);
  } else {
    LR_LAUNCH(stable_window_kernel<1>, grid, dim3(256), 0, stream, f, smooth, offsets, lens, clip_aug, tmap, o, B, rows,
              t_max, H, W, S, extent);
  }
  return lr_launch_status();
}
