// lr_misc.hip — library entry points plus the bandwidth-trivial kernels either side of the
// encoder: batch collation (A1), the landmark step (A7), and the optimiser tail of the
// reference step (A5).
//
// Reference arithmetic replaced here:
//   src/data/data_loader.py:130-142   _pad (zero-pad ragged sequences to the batch max)
//   src/utils/data/face.py:76-90      _applyPadding (integer rectangle padding)
//   src/utils/data/face.py:164-175    getFace (translate x,y by the padded rect origin)
//   src/train/train_better_model.py:78-80  clip_grad_norm_ + Adam.step
#include "lr_common.h"
#include <hip/hip_ext.h>

extern "C" int lr_version(void) { return 100; /* 0.1.0 */ }

extern "C" const char* lr_status_string(int status) {
  switch (status) {
    case LR_OK: return "ok";
    case LR_ERR_INVALID_ARG: return "invalid argument";
    case LR_ERR_WORKSPACE: return "workspace too small";
    case LR_ERR_LAUNCH: return "kernel launch failed";
    case LR_ERR_UNSUPPORTED: return "unsupported configuration";
    case LR_ERR_NO_DEVICE: return "no gfx950 device";
    default: return "unknown status";
  }
}

extern "C" int lr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

namespace {

// One workgroup-row per (b,t): feat floats copied or zeroed; lanes along feat.
__global__ void collate_pad_kernel(const float* __restrict__ packed,
                                   const int64_t* __restrict__ offsets,
                                   const int32_t* __restrict__ lens, float* __restrict__ out,
                                   int B, int t_max, int feat) {
  const int64_t total = (int64_t)B * t_max * feat;
  const int64_t row_elems = (int64_t)t_max * feat;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / row_elems);
    const int64_t r = i - (int64_t)b * row_elems;
    const int t = (int)(r / feat);
    const int f = (int)(r - (int64_t)t * feat);
    float v = 0.f;
    if (t < lens[b]) v = packed[(offsets[b] + t) * feat + f];
    out[i] = v;
  }
}

__global__ void lmk_apply_padding_kernel(const int32_t* __restrict__ rin,
                                         const int32_t* __restrict__ dims,
                                         int32_t* __restrict__ rout, int n, float padding) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int img_h = dims[2 * i], img_w = dims[2 * i + 1];
  int left = rin[4 * i], right = rin[4 * i + 1], top = rin[4 * i + 2], bottom = rin[4 * i + 3];
  const int box_h = bottom - top, box_w = right - left;
  // Python: int(padding * box_w) — a double product truncated toward zero.
  const int pw = (int)((double)padding * (double)box_w);
  const int ph = (int)((double)padding * (double)box_h);
  left = max(0, left - pw);
  right = min(img_w, right + pw);
  top = max(0, top - ph);
  bottom = min(img_h, bottom + ph);
  rout[4 * i] = left;
  rout[4 * i + 1] = right;
  rout[4 * i + 2] = top;
  rout[4 * i + 3] = bottom;
}

__global__ void lmk_translate_kernel(const float* __restrict__ in, const int32_t* __restrict__ rects,
                                     float* __restrict__ out, int64_t total, int per_frame) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t frame = i / per_frame;
    const int comp = (int)((i - frame * per_frame) % 3);
    float v = in[i];
    if (comp == 0) v -= (float)rects[4 * frame];          // left
    else if (comp == 1) v -= (float)rects[4 * frame + 2];  // top
    out[i] = v;
  }
}

// ---- PRNet crop / restore / landmark gather (src/models/face/prnet.py:112-119,136-156,162-170) --------
// Crop geometry of one face rect (left, right, top, bottom): old = (r-l+b-t)/2, centre = (r-(r-l)/2,
// b-(b-t)/2), size = int(old*1.6); the reference then asks skimage for the similarity transform that
// maps the crop square's corners (c-size/2, c-size/2), (c-size/2, c+size/2), (c+size/2, c-size/2) onto
// (0,0), (0,res-1), (res-1,0).  Those three source points ARE a similarity image of the destination
// points (axis-aligned right isosceles triangles), so the least-squares (Umeyama) solution is the exact
// one: scale s = (res-1)/size, no rotation, t = -s * (c - size/2).  size == 0 gives inf/nan as the
// reference's division does.
struct CropT { double s, tx, ty; };
__device__ __forceinline__ CropT crop_transform_of(const int32_t* r, int res, int* size_out) {
  const int left = r[0], right = r[1], top = r[2], bottom = r[3];
  const double old_size = (double)(right - left + bottom - top) / 2.0;
  const double cx = (double)right - (double)(right - left) / 2.0, cy = (double)bottom - (double)(bottom - top) / 2.0;
  const int size = (int)(old_size * 1.6);
  CropT t;
  t.s = (double)(res - 1) / (double)size;
  t.tx = -t.s * (cx - (double)size / 2.0);
  t.ty = -t.s * (cy - (double)size / 2.0);
  if (size_out) *size_out = size;
  return t;
}

__global__ void lmk_crop_transform_kernel(const int32_t* __restrict__ rects, double* __restrict__ tform,
                                          int32_t* __restrict__ sizes, int n, int res) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int size;
  const CropT t = crop_transform_of(rects + 4 * i, res, &size);
  double* o = tform + 9 * (int64_t)i;
  o[0] = t.s; o[1] = 0.0; o[2] = t.tx;
  o[3] = 0.0; o[4] = t.s; o[5] = t.ty;
  o[6] = 0.0; o[7] = 0.0; o[8] = 1.0;
  if (sizes) sizes[i] = size;
}

// restore (prnet.py:150-156): z /= tform[0][0]; [x y]' = (tform^-1 [x y 1]')[0:2], for a general affine
// tform (row-major 3x3, last row 0 0 1).  float32 position map in, float64 out (np.dot's result type).
__device__ __forceinline__ void restore_point(const double* m, double x, double y, double z, double* o) {
  const double det = m[0] * m[4] - m[1] * m[3];
  const double i00 = m[4] / det, i01 = -m[1] / det, i10 = -m[3] / det, i11 = m[0] / det;
  const double i02 = -(i00 * m[2] + i01 * m[5]), i12 = -(i10 * m[2] + i11 * m[5]);
  o[0] = i00 * x + i01 * y + i02;
  o[1] = i10 * x + i11 * y + i12;
  o[2] = z / m[0];
}
__global__ void lmk_restore_kernel(const float* __restrict__ cp, const double* __restrict__ tform,
                                   double* __restrict__ pos, int64_t npix) {
  const int frame = blockIdx.y;
  const double* m = tform + 9 * (int64_t)frame;
  const float* src = cp + (int64_t)frame * npix * 3;
  double* dst = pos + (int64_t)frame * npix * 3;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x)
    restore_point(m, (double)src[3 * p], (double)src[3 * p + 1], (double)src[3 * p + 2], dst + 3 * p);
}

// get_landmarks (prnet.py:162-170): kpt[k] = pos[uv[1][k]][uv[0][k]][:], optionally translated by a rect's
// (left, top) as getFace does (face.py:164-175).  grid n frames, K threads.
__global__ void lmk_gather_kernel(const double* __restrict__ pos, const int32_t* __restrict__ uv,
                                  const int32_t* __restrict__ rects, double* __restrict__ kpt, int res, int K) {
  const int frame = blockIdx.x, k = threadIdx.x;
  if (k >= K) return;
  const int u = uv[k], v = uv[K + k];
  const double* p = pos + (((int64_t)frame * res + v) * res + u) * 3;
  double* o = kpt + ((int64_t)frame * K + k) * 3;
  o[0] = p[0] - (rects ? (double)rects[4 * frame] : 0.0);
  o[1] = p[1] - (rects ? (double)rects[4 * frame + 2] : 0.0);
  o[2] = p[2];
}

// generate_dataview.py:58-64 minus the two networks, fused: padded rect (extractFace, padding) ->
// crop transform of the UNPADDED rect -> restore only the K gathered points -> translate by the
// PADDED rect.  Reads K*12 bytes of each frame's 786 KB position map.
__global__ void lmk_landmarks_kernel(const float* __restrict__ cp, const int32_t* __restrict__ rects,
                                     const int32_t* __restrict__ dims, double padding,
                                     const int32_t* __restrict__ uv, double* __restrict__ out64,
                                     float* __restrict__ out32, int32_t* __restrict__ rects_padded, int res, int K) {
  const int frame = blockIdx.x, k = threadIdx.x;
  const int32_t* r = rects + 4 * frame;
  const int img_h = dims[2 * frame], img_w = dims[2 * frame + 1];
  const int box_h = r[3] - r[2], box_w = r[1] - r[0];
  const int pw = (int)(padding * (double)box_w), ph = (int)(padding * (double)box_h);
  const int left = max(0, r[0] - pw), right = min(img_w, r[1] + pw);
  const int top = max(0, r[2] - ph), bottom = min(img_h, r[3] + ph);
  if (k == 0 && rects_padded) {
    rects_padded[4 * frame] = left;
    rects_padded[4 * frame + 1] = right;
    rects_padded[4 * frame + 2] = top;
    rects_padded[4 * frame + 3] = bottom;
  }
  if (k >= K) return;
  const CropT t = crop_transform_of(r, res, nullptr);
  const double m[9] = {t.s, 0.0, t.tx, 0.0, t.s, t.ty, 0.0, 0.0, 1.0};
  const int u = uv[k], v = uv[K + k];
  const float* p = cp + (((int64_t)frame * res + v) * res + u) * 3;
  double o[3];
  restore_point(m, (double)p[0], (double)p[1], (double)p[2], o);
  o[0] -= (double)left;
  o[1] -= (double)top;
  const int64_t base = ((int64_t)frame * K + k) * 3;
  if (out64) { out64[base] = o[0]; out64[base + 1] = o[1]; out64[base + 2] = o[2]; }
  if (out32) { out32[base] = (float)o[0]; out32[base + 1] = (float)o[1]; out32[base + 2] = (float)o[2]; }
}

__global__ void sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
  float acc = 0.f;
  const int64_t n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x4[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) acc += x[i] * x[i];
  acc = lr_wave_sum(acc);
  __shared__ float part[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += part[w];
    atomicAdd(out, s);
  }
}

// One thread: advance the device-side step counter (unless the batch is skipped), derive the
// bias corrections and the clip coefficient.  Keeping the counter on the device makes the
// whole optimiser step replayable from a hipGraph (host-computed corrections would be frozen).
//   st[0] = active (0/1), st[1] = lr / (1 - beta1^t), st[2] = 1 / sqrt(1 - beta2^t),
//   st[3] = gradient scale (grad_scale x clip coefficient)
__device__ __forceinline__ void adam_prepare_body(int32_t* __restrict__ step_count, int32_t* __restrict__ skip,
                                                  int32_t* __restrict__ fault, bool has_sumsq, float sumsq_value,
                                                  float max_norm, float grad_scale, float lr, float beta1, float beta2,
                                                  float* __restrict__ st, const float* __restrict__ dist_words,
                                                  float world) {
  // fault[0] != 0: a one-launch recurrence of THIS step gave up waiting for a partner workgroup (its outputs
  // and gradients are garbage): the step is skipped like a batch the reference skips (train_better_model.py:49-50).
  // dist_words (data parallel): {number of ranks whose batch was skipped, number of ranks whose recurrence timed out},
  // summed over the ranks by the gradient all-reduce itself (lr_fault_export_f32): the batch counts as skipped only if
  // EVERY rank skipped it, and nobody updates if ANY rank's gradient is garbage — it is in everybody's sum.
  // With dist_words the verdict comes from the SUMMED words ALONE — every rank reads the same two numbers, so the ranks
  // cannot disagree about whether this update happens (round 5 also OR-ed the local fault word read here, at Adam time:
  // a recurrence that timed out after the words had left would then have skipped the update on ONE rank and let the
  // weights drift apart).  lipreading_amd.distributed guarantees the words are exported behind the step's last
  // recurrence — it falls back to the exchange after backward when their bucket was not the last to leave.  The
  // verdict is written back into the local words, so that every rank's status / fault word (the per-epoch loss, the
  // `keep` masks of eval) says the same as the ranks' sum.
  bool skipped = skip && skip[0] != 0, faulted = fault && fault[0] != 0;
  if (dist_words) {
    skipped = dist_words[0] > world - 0.5f;
    faulted = dist_words[1] > 0.5f;
    if (skip) skip[0] = skipped ? 1 : 0;     // the caller's status becomes the ranks' verdict (rounds 1-4: a MIN all-reduce)
    if (fault && faulted) fault[0] |= 1;     // ... and so does the fault word of a rank whose own recurrence was fine
  }
  const bool active = !skipped && !faulted;
  int t = step_count[0];
  if (active) step_count[0] = ++t;
  else step_count[1] += 1;      // steps skipped (a batch the reference `continue`s past, or a recurrence fault)
  if (t < 1) t = 1;
  const float bc1 = 1.f - powf(beta1, (float)t);
  const float bc2 = 1.f - powf(beta2, (float)t);
  float scale = grad_scale;
  if (max_norm > 0.f && has_sumsq) {
    // clip_grad_norm_: coef = max_norm / (total_norm + 1e-6), clamped to 1
    const float norm = sqrtf(sumsq_value) * fabsf(grad_scale);
    const float coef = max_norm / (norm + 1e-6f);
    if (coef < 1.f) scale *= coef;
  }
  st[0] = active ? 1.f : 0.f;
  st[1] = lr / bc1;
  st[2] = 1.f / sqrtf(bc2);
  st[3] = scale;
}
__global__ void adam_prepare_kernel(int32_t* __restrict__ step_count, int32_t* __restrict__ skip,
                                    int32_t* __restrict__ fault, const float* __restrict__ sumsq, float max_norm,
                                    float grad_scale, float lr, float beta1, float beta2, float* __restrict__ st,
                                    const float* __restrict__ dist_words, float world) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  adam_prepare_body(step_count, skip, fault, sumsq != nullptr, sumsq ? sumsq[0] : 0.f, max_norm, grad_scale, lr, beta1, beta2,
                    st, dist_words, world);
}
// sumsq_kernel AND adam_prepare_kernel in one launch (lr_clip_adam_step): every workgroup adds its partial sum of squares
// to out[0] and takes a ticket (out[1], an unsigned); the one that draws the last ticket — every other partial sum is in
// out[0] by then — derives the step's coefficients, leaves the sum in st[5] (FusedAdam.total_norm) and puts BOTH words
// back to 0: the accumulator is clean for the next step whoever launches it (an eager optimiser step behind a replayed
// graph used to pay an ATen fill for that), and lr_step_begin clears both words as well, so a launch that was torn down
// half-way cannot leave a ticket behind that no later launch would ever complete.
__global__ void sumsq_prepare_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out,
                                     int32_t* __restrict__ step_count, int32_t* __restrict__ skip,
                                     int32_t* __restrict__ fault, float max_norm, float grad_scale, float lr,
                                     float beta1, float beta2, float* __restrict__ st,
                                     const float* __restrict__ dist_words, float world) {
  float acc = 0.f;
  const int64_t n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = x4[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) acc += x[i] * x[i];
  acc = lr_wave_sum(acc);
  __shared__ float part[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  float s = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += part[w];
  atomicAdd(out, s);
  __threadfence();
  unsigned* ticket = reinterpret_cast<unsigned*>(out + 1);
  if (atomicAdd(ticket, 1u) != gridDim.x - 1) return;
  *ticket = 0u;
  __threadfence();
  const float total = atomicExch(out, 0.f);   // (an atomic read, served where the other workgroups' adds were, and the reset)
  st[5] = total;
  adam_prepare_body(step_count, skip, fault, true, total, max_norm, grad_scale, lr, beta1, beta2, st, dist_words, world);
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v, int64_t n,
                            const float* __restrict__ st, float beta1, float beta2, float eps) {
  if (st[0] == 0.f) return;  // skipped batch: parameters and moments untouched
  const float step = st[1], inv_sqrt_bc2 = st[2], scale = st[3];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * scale;
    const float mi = beta1 * m[i] + (1.f - beta1) * gi;
    const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] -= step * (mi / denom);
  }
}

// 256 threads = 4 row lanes x 64 columns; blockIdx.y = row slice.
__global__ void colsum_partial_kernel(const float* __restrict__ x, int ld, int rows, int ncol,
                                      float* __restrict__ partial) {
  lr_colsum_partial_body(x, ld, rows, ncol, partial, blockIdx.x, blockIdx.y);
}

inline int grid_for(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CUs x 8 blocks, grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int lr_collate_pad_f32(const float* packed, const int64_t* offsets,
                                  const int32_t* lens, float* out, int B, int t_max, int feat,
                                  lr_stream_t stream) {
  LR_CHECK_ARG(packed && offsets && lens && out);
  LR_CHECK_ARG(B > 0 && t_max > 0 && feat > 0);
  const int64_t total = (int64_t)B * t_max * feat;
  LR_LAUNCH(collate_pad_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, packed, offsets, lens, out, B, t_max, feat);
  return lr_launch_status();
}

extern "C" int lr_lmk_apply_padding(const int32_t* rects_in, const int32_t* dims,
                                    int32_t* rects_out, int n, float padding,
                                    lr_stream_t stream) {
  LR_CHECK_ARG(rects_in && dims && rects_out && n > 0);
  LR_LAUNCH(lmk_apply_padding_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, rects_in, dims, rects_out, n, padding);
  return lr_launch_status();
}

extern "C" int lr_lmk_translate(const float* lmk_in, const int32_t* rects, float* lmk_out, int n,
                                int npts, lr_stream_t stream) {
  LR_CHECK_ARG(lmk_in && rects && lmk_out && n > 0 && npts > 0);
  const int64_t total = (int64_t)n * npts * 3;
  LR_LAUNCH(lmk_translate_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, lmk_in, rects, lmk_out, total, npts * 3);
  return lr_launch_status();
}

extern "C" int lr_lmk_crop_transform(const int32_t* rects, double* tform, int32_t* sizes, int n, int resolution,
                                     lr_stream_t stream) {
  LR_CHECK_ARG(rects && tform && n > 0 && resolution > 1);
  LR_LAUNCH(lmk_crop_transform_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, rects, tform, sizes, n, resolution);
  return lr_launch_status();
}

extern "C" int lr_lmk_restore(const float* cropped_pos, const double* tform, double* pos, int n, int64_t npix,
                              lr_stream_t stream) {
  LR_CHECK_ARG(cropped_pos && tform && pos && n > 0 && npix > 0);
  int gx = (int)((npix + 255) / 256);
  if (gx > 256) gx = 256;
  LR_LAUNCH(lmk_restore_kernel, dim3(gx, n), dim3(256), 0, stream, cropped_pos, tform, pos, npix);
  return lr_launch_status();
}

extern "C" int lr_lmk_gather(const double* pos, const int32_t* uv_kpt_ind, const int32_t* rects, double* kpt, int n,
                             int resolution, int K, lr_stream_t stream) {
  LR_CHECK_ARG(pos && uv_kpt_ind && kpt && n > 0 && resolution > 0 && K > 0 && K <= 1024);
  LR_LAUNCH(lmk_gather_kernel, dim3(n), dim3((K + 63) / 64 * 64), 0, stream, pos, uv_kpt_ind, rects, kpt, resolution, K);
  return lr_launch_status();
}

extern "C" int lr_lmk_landmarks(const float* cropped_pos, const int32_t* rects, const int32_t* dims, double padding,
                                const int32_t* uv_kpt_ind, double* lmk_f64, float* lmk_f32, int32_t* rects_padded,
                                int n, int resolution, int K, lr_stream_t stream) {
  LR_CHECK_ARG(cropped_pos && rects && dims && uv_kpt_ind && (lmk_f64 || lmk_f32));
  LR_CHECK_ARG(n > 0 && resolution > 1 && K > 0 && K <= 1024);
  LR_LAUNCH(lmk_landmarks_kernel, dim3(n), dim3((K + 63) / 64 * 64), 0, stream, cropped_pos, rects, dims, padding,
            uv_kpt_ind, lmk_f64, lmk_f32, rects_padded, resolution, K);
  return lr_launch_status();
}

// ---- decoder loss (train_better_model.py:62,65): sum over (sample, step) rows of nll_loss(ignore_index = PAD,
// reduction = 'sum') divided by the number of non-PAD labels, and its gradient -----------------------------------
namespace {
// one workgroup, fixed summation order: out[0] = -sum_r lp[r][label_r] / count, out[1] = count (rows whose label != ignore)
__global__ __launch_bounds__(1024) void nll_mean_fwd_kernel(const float* __restrict__ lp, const int64_t* __restrict__ labels,
                                                           int64_t label_stride, int L, int ignore, float* __restrict__ out,
                                                           int R, int V, int out3) {
  __shared__ float s_sum[1024];
  __shared__ int s_cnt[1024];
  float acc = 0.f;
  int cnt = 0;
  for (int r = threadIdx.x; r < R; r += 1024) {
    const int64_t lab = labels[(int64_t)(r / L) * label_stride + (r % L)];
    if (lab != ignore && lab >= 0 && lab < V) {
      acc -= lp[(int64_t)r * V + lab];
      ++cnt;
    }
  }
  s_sum[threadIdx.x] = acc;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = s_sum[0] / (float)s_cnt[0];
    out[1] = (float)s_cnt[0];
    if (out3) out[2] = s_sum[0];
  }
}
// the same gradient for any V (one element per thread): V % 4 != 0
__global__ void nll_mean_bwd_scalar_kernel(const int64_t* __restrict__ labels, int64_t label_stride, int L, int ignore,
                                           const float* __restrict__ fwd_out, const float* __restrict__ g,
                                           float* __restrict__ d_lp, int R, int V) {
  const float w = -g[0] / fwd_out[1];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)R * V; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / V), v = (int)(i - (int64_t)r * V);
    const int64_t lab = labels[(int64_t)(r / L) * label_stride + (r % L)];
    d_lp[i] = (lab != ignore && lab == v) ? w : 0.f;
  }
}
// d_lp[r][v] = (v == label_r != ignore) ? -g / count : 0, 4 columns per thread
__global__ void nll_mean_bwd_kernel(const int64_t* __restrict__ labels, int64_t label_stride, int L, int ignore,
                                    const float* __restrict__ fwd_out, const float* __restrict__ g,
                                    float* __restrict__ d_lp, int R, int V) {
  const int vq = V >> 2;
  const float w = -g[0] / fwd_out[1];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)R * vq; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / vq), v = 4 * (int)(i - (int64_t)r * vq);
    const int64_t lab = labels[(int64_t)(r / L) * label_stride + (r % L)];
    const bool on = lab != ignore;
    float4 o;
    o.x = on && lab == v ? w : 0.f;
    o.y = on && lab == v + 1 ? w : 0.f;
    o.z = on && lab == v + 2 ? w : 0.f;
    o.w = on && lab == v + 3 ? w : 0.f;
    reinterpret_cast<float4*>(d_lp)[i] = o;
  }
}
}  // namespace

extern "C" int lr_nll_mean_forward(const float* log_probs, const int64_t* labels, int64_t label_stride, int L,
                                   int ignore_index, float* out2, int R, int V, lr_stream_t stream) {
  LR_CHECK_ARG(log_probs && labels && out2 && R > 0 && V > 0 && L > 0 && R % L == 0);
  LR_LAUNCH(nll_mean_fwd_kernel, dim3(1), dim3(1024), 0, stream, log_probs, labels, label_stride, L, ignore_index, out2,
            R, V, 0);
  return lr_launch_status();
}

extern "C" int lr_nll_forward3(const float* log_probs, const int64_t* labels, int64_t label_stride, int L, int ignore_index,
                               float* out3, int R, int V, lr_stream_t stream) {
  LR_CHECK_ARG(log_probs && labels && out3 && R > 0 && V > 0 && L > 0 && R % L == 0);
  LR_LAUNCH(nll_mean_fwd_kernel, dim3(1), dim3(1024), 0, stream, log_probs, labels, label_stride, L, ignore_index, out3,
            R, V, 1);
  return lr_launch_status();
}

extern "C" int lr_nll_mean_backward(const int64_t* labels, int64_t label_stride, int L, int ignore_index,
                                    const float* fwd_out2, const float* grad_out, float* d_log_probs, int R, int V,
                                    lr_stream_t stream) {
  LR_CHECK_ARG(labels && fwd_out2 && grad_out && d_log_probs && R > 0 && V > 0 && L > 0 && R % L == 0);
  if (V % 4 != 0 || (reinterpret_cast<uintptr_t>(d_log_probs) & 15) != 0) {
    int blocks = (int)(((int64_t)R * V + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    LR_LAUNCH(nll_mean_bwd_scalar_kernel, dim3(blocks), dim3(256), 0, stream, labels, label_stride, L, ignore_index,
              fwd_out2, grad_out, d_log_probs, R, V);
    return lr_launch_status();
  }
  int blocks = (int)(((int64_t)R * (V / 4) + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  LR_LAUNCH(nll_mean_bwd_kernel, dim3(blocks), dim3(256), 0, stream, labels, label_stride, L, ignore_index, fwd_out2,
            grad_out, d_log_probs, R, V);
  return lr_launch_status();
}

// ---- inter-layer dropout of nn.GRU / nn.LSTM(dropout = p) in training mode (better_model.py:47-49 passes rnn_dropout
// through; every shipped config sets 0) ------------------------------------------------------------------------
// mask[i] = 0 with probability p, 1 / (1 - p) otherwise — Philox4x32-10 keyed by (seed), counter = the element's group of
// four, so the mask of a (seed, n) is the same whatever the launch geometry; y = x * mask.  The backward is the same
// multiply (lr_mul_f32).  torch draws its mask from its own generator stream: like the decoder loop's samples
// (better_model.py:63), the mask is a random variable, not a value to match — it is tested as a mask.
namespace {
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__global__ void dropout_fwd_kernel(const float* x, float* y, float* __restrict__ mask, int64_t n,
                                   float p, unsigned long long seed) {
  const float scale = 1.f / (1.f - p);
  const int64_t groups = (n + 3) >> 2;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * blockDim.x) {
    unsigned r[4];
    philox4x32_10((unsigned)gi, (unsigned)(gi >> 32), 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = 4 * gi + e;
      if (i < n) {
        // uniform in [0, 1) from the top 24 bits: keep with probability 1 - p
        const float u = (float)(r[e] >> 8) * (1.f / 16777216.f);
        const float m = u < p ? 0.f : scale;
        mask[i] = m;
        if (y) y[i] = x[i] * m;      // x == y == NULL: the mask alone
      }
    }
  }
}
__global__ void mul_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = a[i] * b[i];
}
// (D, B, H) -> (B, D * H), forward direction first (better_model.py:98-112 _cat_directions), or back; nt tensors at once
struct CatPtrs {
  const float* in[2];
  float* out[2];
};
__global__ void cat_directions_kernel(CatPtrs p, int nt, int B, int H, int D, int inverse) {
  const int64_t total = (int64_t)nt * D * B * H;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / ((int64_t)D * B * H));
    const int64_t r = i - (int64_t)k * D * B * H;
    const int j = (int)(r % H), b = (int)((r / H) % B), d = (int)(r / ((int64_t)H * B));
    const int64_t dbh = ((int64_t)d * B + b) * H + j, bdh = ((int64_t)b * D + d) * H + j;
    if (inverse) p.out[k][dbh] = p.in[k][bdh];
    else p.out[k][bdh] = p.in[k][dbh];
  }
}
}  // namespace

extern "C" int lr_dropout_forward(const float* x, float* y, float* mask, int64_t n, float p, uint64_t seed,
                                  lr_stream_t stream) {
  LR_CHECK_ARG(mask && ((x && y) || (!x && !y)) && n > 0 && p >= 0.f && p < 1.f);
  LR_LAUNCH(dropout_fwd_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, stream, x, y, mask, n, p,
            (unsigned long long)seed);
  return lr_launch_status();
}
extern "C" int lr_mul_f32(const float* a, const float* b, float* out, int64_t n, lr_stream_t stream) {
  LR_CHECK_ARG(a && b && out && n > 0);
  LR_LAUNCH(mul_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, a, b, out, n);
  return lr_launch_status();
}
extern "C" int lr_cat_directions(const float* in0, float* out0, const float* in1, float* out1, int B, int H, int D,
                                 int inverse, lr_stream_t stream) {
  LR_CHECK_ARG(in0 && out0 && B > 0 && H > 0 && (D == 1 || D == 2) && ((in1 == nullptr) == (out1 == nullptr)));
  CatPtrs p;
  p.in[0] = in0; p.out[0] = out0; p.in[1] = in1; p.out[1] = out1;
  const int nt = in1 ? 2 : 1;
  LR_LAUNCH(cat_directions_kernel, dim3(grid_for((int64_t)nt * D * B * H, 256)), dim3(256), 0, stream, p, nt, B, H, D, inverse);
  return lr_launch_status();
}

// labels = chars[:, 1:] + 1 as int32, frame_lens / (char_lens - 1) as int32 (include/lipreading_hip.h)
__global__ void ctc_prepare_i64_kernel(const int64_t* __restrict__ chars, int64_t chars_stride,
                                       const int64_t* __restrict__ frame_lens, const int64_t* __restrict__ char_lens,
                                       int32_t* __restrict__ labels_p1, int32_t* __restrict__ frame_lens32,
                                       int32_t* __restrict__ label_lens32, int B, int L) {
  const int total = B * L;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / L, l = i - b * L;
    labels_p1[i] = (int32_t)chars[(int64_t)b * chars_stride + 1 + l] + 1;
  }
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    frame_lens32[b] = (int32_t)frame_lens[b];
    label_lens32[b] = (int32_t)char_lens[b] - 1;
  }
}

extern "C" int lr_ctc_prepare_i64(const int64_t* chars, int64_t chars_stride, const int64_t* frame_lens,
                                  const int64_t* char_lens, int32_t* labels_p1, int32_t* frame_lens32,
                                  int32_t* label_lens32, int B, int L, lr_stream_t stream) {
  LR_CHECK_ARG(chars && frame_lens && char_lens && labels_p1 && frame_lens32 && label_lens32 && B > 0 && L > 0);
  int blocks = (B * L + 255) / 256;
  if (blocks > 256) blocks = 256;
  LR_LAUNCH(ctc_prepare_i64_kernel, dim3(blocks), dim3(256), 0, stream, chars, chars_stride, frame_lens, char_lens,
            labels_p1, frame_lens32, label_lens32, B, L);
  return lr_launch_status();
}

// ---- device-side fault words (see include/lipreading_hip.h: lr_fault_words) ---------------------------------
// One int32[2] per device, {pending, total}.  The one-launch recurrences OR 1 into `pending` when a member gives
// up waiting; lr_ctc_reduce and lr_adam_step read `pending` (skip the batch / the update); lr_step_begin moves
// `pending` into `total` at the top of the next step.  Allocated on first use (never under stream capture: the
// product runs its first steps eagerly, and _C.lib() calls lr_fault_words() when it loads the library).
namespace {
constexpr int kMaxDevices = 64;
int32_t* g_fault_words[kMaxDevices];
int g_drop_member = -1;
int g_cluster_off = 0;   // lr_rnn_debug_disable_cluster; bit 0 (the only one read): no cluster recurrence
__global__ void step_begin_kernel(float4* __restrict__ g, int64_t n4, float* __restrict__ tail, int ntail,
                                  int32_t* __restrict__ fault, float* __restrict__ also_zero) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0 && fault) {
    fault[1] += fault[0];
    fault[0] = 0;
    fault[2] = 0;   // lr_ctc.hip's completion count of the alpha/beta launch (a torn-down launch must not poison the next step)
  }
  if (i0 == 0 && also_zero) also_zero[0] = also_zero[1] = 0.f;   // (sum-of-squares accumulator, its ticket)
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = i0; i < n4; i += (int64_t)gridDim.x * blockDim.x) g[i] = z;
  if (i0 < ntail) tail[i0] = 0.f;
}
// lr_step_begin + lr_ctc_prepare_i64 in one launch (lr_step_begin_ctc): the step's first two launches depend on nothing
// and on each other not at all; the last workgroups of the grid do the label plumbing
__global__ void step_begin_ctc_kernel(float4* __restrict__ g, int64_t n4, float* __restrict__ tail, int ntail,
                                      int32_t* __restrict__ fault, float* __restrict__ also_zero, int zero_blocks,
                                      const int64_t* __restrict__ chars, int64_t chars_stride,
                                      const int64_t* __restrict__ frame_lens, const int64_t* __restrict__ char_lens,
                                      int32_t* __restrict__ labels_p1, int32_t* __restrict__ frame_lens32,
                                      int32_t* __restrict__ label_lens32, int B, int L) {
  if ((int)blockIdx.x >= zero_blocks) {
    const int pb = blockIdx.x - zero_blocks, np = gridDim.x - zero_blocks;
    const int total = B * L;
    for (int i = pb * blockDim.x + threadIdx.x; i < total; i += np * blockDim.x) {
      const int b = i / L, l = i - b * L;
      labels_p1[i] = (int32_t)chars[(int64_t)b * chars_stride + 1 + l] + 1;
    }
    for (int b = pb * blockDim.x + threadIdx.x; b < B; b += np * blockDim.x) {
      frame_lens32[b] = (int32_t)frame_lens[b];
      label_lens32[b] = (int32_t)char_lens[b] - 1;
    }
    return;
  }
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 == 0 && fault) {
    fault[1] += fault[0];
    fault[0] = 0;
    fault[2] = 0;   // lr_ctc.hip's completion count of the alpha/beta launch (a torn-down launch must not poison the next step)
  }
  if (i0 == 0 && also_zero) also_zero[0] = also_zero[1] = 0.f;   // (sum-of-squares accumulator, its ticket)
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = i0; i < n4; i += (int64_t)zero_blocks * blockDim.x) g[i] = z;
  if (i0 < ntail) tail[i0] = 0.f;
}
__global__ void fault_export_kernel(const int32_t* __restrict__ status, const int32_t* __restrict__ fault,
                                    int32_t* __restrict__ out2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  out2[0] = status ? status[0] : 0;
  out2[1] = (fault && fault[0] != 0) ? -1 : 0;
}
// the same two facts as floats the gradient all-reduce can SUM: {1 if this rank's batch was skipped, 1 if its recurrence
// timed out} (lipreading_amd.distributed writes them into the spare words at the front of the flat gradient buffer)
__global__ void fault_export_f32_kernel(const int32_t* __restrict__ status, const int32_t* __restrict__ fault,
                                        float* __restrict__ out2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  out2[0] = (status && status[0] != 0) ? 1.f : 0.f;
  out2[1] = (fault && fault[0] != 0) ? 1.f : 0.f;
}
__global__ void fault_import_kernel(const int32_t* __restrict__ in2, int32_t* __restrict__ status,
                                    int32_t* __restrict__ fault) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (status) status[0] = in2[0];
  if (fault && in2[1] < 0) fault[0] |= 1;
}
}  // namespace

int32_t* lr_fault_words() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
  if (!g_fault_words[dev]) {
    int32_t* p = nullptr;
    if (hipMalloc((void**)&p, 4 * sizeof(int32_t)) != hipSuccess) {
      lr_clear_error();
      return nullptr;
    }
    if (hipMemset(p, 0, 4 * sizeof(int32_t)) != hipSuccess) {
      lr_clear_error();
      (void)hipFree(p);
      return nullptr;
    }
    g_fault_words[dev] = p;
  }
  return g_fault_words[dev];
}
int lr_debug_drop_member_value() { return g_drop_member; }
// compute units of the current device (0 without a device): the one-launch recurrences need their partner
// workgroups resident together, one per CU
int lr_device_cus() {
  static int cus[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
    lr_clear_error();
    return 0;
  }
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
      lr_clear_error();
      return 0;
    }
    cus[dev] = n;
  }
  return cus[dev];
}

extern "C" void* lr_fault_words_ptr(void) { return lr_fault_words(); }
extern "C" void lr_rnn_debug_drop_member(int member) { g_drop_member = member; }
extern "C" void lr_rnn_debug_disable_cluster(int off) { g_cluster_off = off; }
// lr_rnn_one_launch_enable(0): the product's switch (lipreading_amd.train after repeated recurrence time-outs) — no
// pair / cluster recurrence, encoder layers and decoder loop alike, until it is switched on again
namespace { int g_one_launch_off = 0; }
extern "C" void lr_rnn_one_launch_enable(int on) { g_one_launch_off = on ? 0 : 1; }
extern "C" int lr_rnn_one_launch_enabled(void) { return g_one_launch_off ? 0 : 1; }
int lr_debug_cluster_disabled() { return (g_cluster_off & 1) | g_one_launch_off; }

// TEST HOOK (lr_debug_busy): `workgroups` workgroups that each take a whole compute unit's LDS (lds_bytes) and spin for
// `microseconds` of wall clock — a stand-in for a foreign kernel (an RCCL ring kernel on another stream) that holds CUs
// while a cluster recurrence, whose members must all be resident, is launched.
namespace {
__global__ __launch_bounds__(256) void busy_kernel(long long ticks, int* sink) {
  extern __shared__ int hog[];
  const long long t0 = wall_clock64();
  int v = 0;
  while (wall_clock64() - t0 < ticks) {
    hog[threadIdx.x] = v++;
    __builtin_amdgcn_s_sleep(32);
  }
  if (sink && v == -1) sink[0] = hog[0];
}
}  // namespace
extern "C" int lr_debug_busy(int workgroups, int lds_bytes, int microseconds, lr_stream_t stream) {
  LR_CHECK_ARG(workgroups > 0 && lds_bytes >= 1024 && lds_bytes <= 160 * 1024 && microseconds >= 0);
  lr_clear_error();
  if (hipFuncSetAttribute((const void*)busy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
    return LR_ERR_LAUNCH;
  // wall_clock64 ticks at 100 MHz on gfx9
  hipLaunchKernelGGL(busy_kernel, dim3(workgroups), dim3(256), (size_t)lds_bytes, (hipStream_t)stream,
                     (long long)microseconds * 100, (int*)nullptr);
  return lr_launch_status();
}
// tuning knobs of the cluster recurrence's exchange (lr_rnn_debug_tune): [0] forward, [1] backward; bits 0-7 = 64-clock
// sleeps before the first poll, bits 8-15 = sleeps between poll rounds
// which = 2 .. 5: the grid recurrence's four gathers (lr_rnn_grid.hip): forward h, forward partial sums, backward partial dh,
// backward dG
namespace { int g_tune[6] = {1 << 8, 1 << 8, 1 << 8, 1 << 8, 1 << 8, 1 << 8}; }   // (swept on the MI355X: one sleep between rounds, no first-poll delay)
int lr_debug_tune_value(int which) { return g_tune[which >= 0 && which < 6 ? which : 0]; }
extern "C" void lr_rnn_debug_tune(int which, int first_poll_delay, int round_sleep) {
  if (which < 0 || which >= 6) return;
  g_tune[which] = (first_poll_delay & 0xff) | ((round_sleep & 0xff) << 8);
}

extern "C" int lr_rnn_pair_errors(void) {
  int32_t* w = lr_fault_words();
  if (!w) return -1;
  int32_t v[2] = {0, 0}, zero[2] = {0, 0};
  lr_clear_error();
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(v, w, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if ((v[0] || v[1]) && hipMemcpy(w, zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess) return -1;
  return v[0] + v[1];
}

// data parallel: {status, -(pending != 0)} for ONE MIN all-reduce — the batch is skipped when every rank skipped it
// (status), the update is skipped everywhere when ANY rank's recurrence timed out (its garbage gradient is in the sum)
extern "C" int lr_fault_export(const int32_t* status, int32_t* out2, lr_stream_t stream) {
  LR_CHECK_ARG(out2);
  LR_LAUNCH(fault_export_kernel, dim3(1), dim3(64), 0, stream, status, (const int32_t*)lr_fault_words(), out2);
  return lr_launch_status();
}
extern "C" int lr_fault_export_f32(const int32_t* status, float* out2, lr_stream_t stream) {
  LR_CHECK_ARG(out2);
  LR_LAUNCH(fault_export_f32_kernel, dim3(1), dim3(64), 0, stream, status, (const int32_t*)lr_fault_words(), out2);
  return lr_launch_status();
}
extern "C" int lr_fault_import(const int32_t* in2, int32_t* status, lr_stream_t stream) {
  LR_CHECK_ARG(in2);
  LR_LAUNCH(fault_import_kernel, dim3(1), dim3(64), 0, stream, in2, status, lr_fault_words());
  return lr_launch_status();
}

extern "C" int lr_step_begin(float* grad, int64_t n, float* also_zero, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && (grad || n == 0));
  LR_CHECK_ARG((reinterpret_cast<uintptr_t>(grad) & 15) == 0);
  const int64_t n4 = n / 4;
  LR_LAUNCH(step_begin_kernel, dim3(grid_for(n4 > 0 ? n4 : 1, 256)), dim3(256), 0, stream, (float4*)grad, n4,
            grad + n4 * 4, (int)(n - n4 * 4), lr_fault_words(), also_zero);
  return lr_launch_status();
}

extern "C" int lr_step_begin_ctc(float* grad, int64_t n, float* also_zero, const int64_t* chars, int64_t chars_stride,
                                 const int64_t* frame_lens, const int64_t* char_lens, int32_t* labels_p1,
                                 int32_t* frame_lens32, int32_t* label_lens32, int B, int L, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && (grad || n == 0));
  LR_CHECK_ARG((reinterpret_cast<uintptr_t>(grad) & 15) == 0);
  LR_CHECK_ARG(chars && frame_lens && char_lens && labels_p1 && frame_lens32 && label_lens32 && B > 0 && L > 0);
  const int64_t n4 = n / 4;
  const int zero_blocks = grid_for(n4 > 0 ? n4 : 1, 256);
  int prep_blocks = (B * L + 255) / 256;
  if (prep_blocks > 16) prep_blocks = 16;
  LR_LAUNCH(step_begin_ctc_kernel, dim3(zero_blocks + prep_blocks), dim3(256), 0, stream, (float4*)grad, n4, grad + n4 * 4,
            (int)(n - n4 * 4), lr_fault_words(), also_zero, zero_blocks, chars, chars_stride, frame_lens, char_lens, labels_p1,
            frame_lens32, label_lens32, B, L);
  return lr_launch_status();
}

extern "C" int lr_sumsq(const float* x, int64_t n, float* out, lr_stream_t stream) {
  LR_CHECK_ARG(x && out && n >= 0);
  if (n == 0) return LR_OK;
  LR_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  int g = grid_for((n + 3) / 4, 256);
  if (g > 256) g = 256;  // one atomic per workgroup
  LR_LAUNCH(sumsq_kernel, dim3(g), dim3(256), 0, stream, x, n, out);
  return lr_launch_status();
}

extern "C" int lr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                            int64_t n, const float* sumsq, float max_norm, float grad_scale,
                            float lr, float beta1, float beta2, float eps, int32_t* step_count,
                            int32_t* skip, float* scratch, const float* dist_words, float world,
                            lr_stream_t stream) {
  LR_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && step_count && scratch && n >= 0);
  LR_LAUNCH(adam_prepare_kernel, dim3(1), dim3(64), 0, stream, step_count, skip, lr_fault_words(),
            sumsq, max_norm, grad_scale, lr, beta1, beta2, scratch, dist_words, world);
  int st = lr_launch_status();
  if (st != LR_OK || n == 0) return st;
  LR_LAUNCH(adam_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, param, grad, exp_avg,
            exp_avg_sq, n, (const float*)scratch, beta1, beta2, eps);
  return lr_launch_status();
}

extern "C" int lr_clip_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 float* sumsq, float max_norm, float grad_scale, float lr, float beta1, float beta2,
                                 float eps, int32_t* step_count, int32_t* skip, float* scratch8,
                                 const float* dist_words, float world, int64_t n_sumsq, lr_stream_t stream) {
  LR_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && step_count && scratch8 && sumsq && n > 0 && max_norm > 0.f);
  LR_CHECK_ARG((reinterpret_cast<uintptr_t>(grad) & 15) == 0 && n_sumsq >= 0 && n_sumsq <= n);
  int g = grid_for((n_sumsq + 3) / 4, 256);
  if (g > 256) g = 256;  // one atomic per workgroup
  // (n_sumsq < n: the rest of the buffer's sum of squares is in sumsq[0] already — lr_sumsq calls of this step)
  LR_LAUNCH(sumsq_prepare_kernel, dim3(g), dim3(256), 0, stream, grad, n_sumsq, sumsq, step_count, skip,
            lr_fault_words(), max_norm, grad_scale, lr, beta1, beta2, scratch8, dist_words, world);
  int st = lr_launch_status();
  if (st != LR_OK) return st;
  LR_LAUNCH(adam_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, param, grad, exp_avg, exp_avg_sq, n,
            (const float*)scratch8, beta1, beta2, eps);
  return lr_launch_status();
}

int lr_colsum_partial(const float* x, int ld, int rows, int ncol, float* partial, hipStream_t stream) {
  LR_LAUNCH(colsum_partial_kernel, dim3((ncol + 63) / 64, LR_COLSUM_SPLITS), dim3(256), 0, stream, x,
            ld, rows, ncol, partial);
  return lr_launch_status();
}

// ---- A9 (BUILD-DEFINED): mouth crop + bilinear resize ------------------------------------------------
// The reference defines `_mouth = slice(48, 68)` (src/utils/data/face.py:21) and never uses it; it
// has no pixel lip crop.  Specification of this build: per frame, the bounding box
// of landmarks [lo,hi) in image coordinates -> centre (cx,cy), side = max(w,h)*(1+2*margin), at least
// 2 px -> square window resampled to S x S with bilinear interpolation, half-pixel centres, source
// coordinates clamped to the image (edge replication), result rounded to nearest uint8.
// lip_crop_box / lip_crop_pixel are the ONE statement of that arithmetic: the per-sample kernel (lr_lip_crop_u8) and the
// whole-batch kernel (lr_lip_crop_collate_u8) both inline them, so the compiler contracts the same multiplies and
// adds in both and their bytes agree.  The multiply-adds whose rounding matters are spelled fmaf (what the compiler
// made of `a + b * c` here all along); the other products are by 0.5 or 2 and exact either way.
namespace {
// box[0] = left, box[1] = top, box[2] = source pixels per output pixel
__device__ __forceinline__ void lip_crop_box(const float* __restrict__ L, int lo, int hi, float margin, int S,
                                             float* box) {
  float x0 = L[lo * 3], x1 = x0, y0 = L[lo * 3 + 1], y1 = y0;
  for (int p = lo + 1; p < hi; ++p) {
    const float x = L[p * 3], y = L[p * 3 + 1];
    x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
  }
  float side = fmaxf(x1 - x0, y1 - y0) * (1.f + 2.f * margin);
  side = fmaxf(side, 2.f);
  box[0] = 0.5f * (x0 + x1) - 0.5f * side;   // left
  box[1] = 0.5f * (y0 + y1) - 0.5f * side;   // top
  box[2] = side / (float)S;                  // source pixels per output pixel
}

// output pixel (oy, ox) of the plane P [H][W]
__device__ __forceinline__ unsigned char lip_crop_pixel(const unsigned char* __restrict__ P, int H, int W, int oy, int ox,
                                                        float left, float top, float scale) {
  float sx = fmaf((float)ox + 0.5f, scale, left) - 0.5f;
  float sy = fmaf((float)oy + 0.5f, scale, top) - 0.5f;
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
}  // namespace

__global__ void lip_crop_kernel(const unsigned char* __restrict__ frames, const float* __restrict__ lmk,
                                unsigned char* __restrict__ out, int H, int W, int S, int npts, int lo,
                                int hi, float margin) {
  __shared__ float box[4];
  const int n = blockIdx.x;
  if (threadIdx.x == 0) lip_crop_box(lmk + (int64_t)n * npts * 3, lo, hi, margin, S, box);
  __syncthreads();
  const float left = box[0], top = box[1], scale = box[2];
  const unsigned char* F = frames + (int64_t)n * 3 * H * W;
  unsigned char* O = out + (int64_t)n * 3 * S * S;
  for (int i = threadIdx.x; i < 3 * S * S; i += blockDim.x) {
    const int c = i / (S * S), r = i - c * S * S;
    const int oy = r / S, ox = r - oy * S;
    O[i] = lip_crop_pixel(F + (int64_t)c * H * W, H, W, oy, ox, left, top, scale);
  }
}

extern "C" int lr_lip_crop_u8(const void* frames, const float* lmk, void* out, int n, int H, int W, int S,
                              int npts, int lo, int hi, float margin, lr_stream_t stream) {
  LR_CHECK_ARG(frames && lmk && out && n > 0 && H > 0 && W > 0 && S > 0);
  LR_CHECK_ARG(npts > 0 && lo >= 0 && hi > lo && hi <= npts && margin >= 0.f);
  LR_LAUNCH(lip_crop_kernel, dim3(n), dim3(256), 0, stream, (const unsigned char*)frames, lmk,
            (unsigned char*)out, H, W, S, npts, lo, hi, margin);
  return lr_launch_status();
}

// A9 for a whole ragged batch in one launch (lr_lip_crop_collate_u8): a capped grid strides over the B * t_max
// (sample, frame) pairs of the padded batch.  A real frame is cropped exactly as lip_crop_kernel crops it, V
// horizontally adjacent pixels per thread stored as one V-byte vector; a padding frame is filled with zeros V bytes at
// a time.  Every byte of out is written.  The box of a frame is computed by one lane into one of two LDS slots, so
// that one barrier per frame is enough: the slot written for frame i + 2 is the one whose readers all passed the
// barrier of frame i + 1.
namespace {
template <int V> struct CropVec;
template <> struct CropVec<1> { typedef unsigned char T; };
template <> struct CropVec<4> { typedef uint32_t T; };
template <> struct CropVec<16> { typedef uint4 T; };

template <int V>
__global__ __launch_bounds__(256) void lip_crop_collate_kernel(
    const unsigned char* __restrict__ frames, const float* __restrict__ lmk, const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ lens, unsigned char* __restrict__ out, int B, int t_max, int H, int W, int S, int npts,
    int lo, int hi, float margin) {
  typedef typename CropVec<V>::T vec_t;
  __shared__ float box[2][4];
  const int per_row = S / V;                 // S % V == 0 (the launcher picks V)
  const int items = 3 * S * per_row;         // V-pixel groups of one frame
  const int pairs = B * t_max;
  int parity = 0;
  for (int p = blockIdx.x; p < pairs; p += gridDim.x) {   // uniform per workgroup: the barrier below is safe
    const int b = p / t_max, t = p - b * t_max;
    const int len = min(lens[b], t_max);     // lens[b] > t_max is the caller's error; never write outside out
    vec_t* O = reinterpret_cast<vec_t*>(out + (int64_t)p * 3 * S * S);
    if (t >= len) {
      vec_t zero;
      __builtin_memset(&zero, 0, sizeof(zero));
      for (int i = threadIdx.x; i < items; i += blockDim.x) O[i] = zero;
      continue;
    }
    const int64_t n = offsets[b] + t;
    float* bx = box[parity];
    parity ^= 1;
    if (threadIdx.x == 0) lip_crop_box(lmk + n * npts * 3, lo, hi, margin, S, bx);
    __syncthreads();
    const float left = bx[0], top = bx[1], scale = bx[2];
    const unsigned char* F = frames + n * 3 * H * W;
    for (int i = threadIdx.x; i < items; i += blockDim.x) {
      const int c = i / (S * per_row), r = i - c * S * per_row;
      const int oy = r / per_row, ox = (r - oy * per_row) * V;
      const unsigned char* P = F + (int64_t)c * H * W;
      union { vec_t v; unsigned char px[V]; } u;
#pragma unroll
      for (int k = 0; k < V; ++k) u.px[k] = lip_crop_pixel(P, H, W, oy, ox + k, left, top, scale);
      O[i] = u.v;
    }
  }
}
}  // namespace

extern "C" int lr_lip_crop_collate_u8(const void* frames, const float* lmk, const int64_t* offsets,
                                      const int32_t* lens, void* out, int B, int t_max, int H, int W, int S, int npts,
                                      int lo, int hi, float margin, lr_stream_t stream) {
  LR_CHECK_ARG(frames && lmk && offsets && lens && out && B > 0 && t_max > 0 && H > 0 && W > 0 && S > 0);
  LR_CHECK_ARG(npts > 0 && lo >= 0 && hi > lo && hi <= npts && margin >= 0.f);
  LR_CHECK_ARG((int64_t)B * t_max <= INT32_MAX && (int64_t)S * S <= INT32_MAX / 3);
  const int pairs = B * t_max;
  const dim3 grid(pairs < 2048 ? pairs : 2048);   // 256 CUs x 8 workgroups; the rest by the grid stride
  const unsigned char* f = (const unsigned char*)frames;
  unsigned char* o = (unsigned char*)out;
  // a frame of out starts at a multiple of 3 * S * S bytes: vector stores need S % V == 0 and an aligned base
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (aligned && S % 16 == 0) {
    LR_LAUNCH(lip_crop_collate_kernel<16>, grid, dim3(256), 0, stream, f, lmk, offsets, lens, o, B, t_max, H, W, S,
              npts, lo, hi, margin);
  } else if (aligned && S % 4 == 0) {
    LR_LAUNCH(lip_crop_collate_kernel<4>, grid, dim3(256), 0, stream, f, lmk, offsets, lens, o, B, t_max, H, W, S,
              npts, lo, hi, margin);
  } else {
    LR_LAUNCH(lip_crop_collate_kernel<1>, grid, dim3(256), 0, stream, f, lmk, offsets, lens, o, B, t_max, H, W, S,
              npts, lo, hi, margin);
  }
  return lr_launch_status();
}

// Training-time clip augmentation inside the collate launch (lr_lip_crop_collate_aug_u8).  The host draws, the kernel
// applies: clip_aug[b] = (dx, dy, zoom, flip) moves, scales and mirrors the crop window of every frame of sample b, and
// tmap[offsets[b] + t] names the source frame (within sample b) of output frame t, or < 0 for a masked (all-zero) frame.
// The window starts from lip_crop_box's centre and side of the SOURCE row: the shift is in units of the un-zoomed
// side, the zoom scales the side about the shifted centre, the flip mirrors output columns.  With the identity record
// (0, 0, 1, 0) every expression rounds to lip_crop_box's: fmaf(0, side, c) = c and max(side * 1, 2) = side.  Grid, LDS
// slots, barrier and stores are lip_crop_collate_kernel's.  Three things differ, each measured:
//  * A mirrored frame is computed group by group exactly as the plain one — the same source columns per lane,
//    ascending across the wave (gathering them in descending order was 40 % slower) — and each group of V pixels is
//    stored at its mirrored place with its bytes reversed (v_perm with a uniform selector: one loop for both).
//  * The extent is taken by the first wave together, one landmark per lane, instead of by one lane point after point:
//    min and max do not depend on the order.
//  * A workgroup has one or two frames to do, so a frame's prologue (lens, offsets -> map -> landmarks: three dependent
//    loads) is on the critical path.  The NEXT frame's prologue loads are issued before the pixels of this one, and
//    only their reduction is left for afterwards (one landmark per lane is held meanwhile; with more than 64
//    landmarks in [lo, hi) they are loaded when the frame is started).
// The 4-pixel variant (S % 16 != 0, off the bench shape) sits at the 64 VGPRs of 8 waves per SIMD already: it keeps the
// one-lane extent (taken when the frame is started) and mirrors by reversing the source columns, which holds it there.
namespace {
// The landmarks' bounding box in two steps, by threads 0 .. LANES-1 together (LANES = 64: the first wave, every lane
// of it; or 1).  lip_crop_partial: each lane's share of the points (the loads); lip_crop_finish: the reduction over the
// lanes, then twice the centre (sx2 = x0 + x1, sy2 = y0 + y1) and the window's side (lip_crop_box's), in every lane.
template <int LANES>
__device__ __forceinline__ void lip_crop_partial(const float* __restrict__ L, int lo, int hi, float& x0, float& x1,
                                                 float& y0, float& y1) {
  x0 = x1 = L[lo * 3];
  y0 = y1 = L[lo * 3 + 1];
  for (int p = lo + (LANES > 1 ? (int)threadIdx.x : 1); p < hi; p += LANES) {
    const float x = L[p * 3], y = L[p * 3 + 1];
    x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
  }
}

template <int LANES>
__device__ __forceinline__ void lip_crop_finish(float x0, float x1, float y0, float y1, float margin, float& sx2,
                                                float& sy2, float& side) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1) {
    x0 = fminf(x0, __shfl_xor(x0, off, 64)); x1 = fmaxf(x1, __shfl_xor(x1, off, 64));
    y0 = fminf(y0, __shfl_xor(y0, off, 64)); y1 = fmaxf(y1, __shfl_xor(y1, off, 64));
  }
  side = fmaxf(x1 - x0, y1 - y0) * (1.f + 2.f * margin);
  side = fmaxf(side, 2.f);
  sx2 = x0 + x1;
  sy2 = y0 + y1;
}

// the bytes of a group in reverse order when flip is set (sel: v_perm's byte selector, identity or reversed)
__device__ __forceinline__ unsigned char crop_vec_mirror(unsigned char v, bool, uint32_t) { return v; }
__device__ __forceinline__ uint32_t crop_vec_mirror(uint32_t v, bool, uint32_t sel) {
  return __builtin_amdgcn_perm(v, v, sel);
}
__device__ __forceinline__ uint4 crop_vec_mirror(uint4 v, bool flip, uint32_t sel) {
  const uint32_t a = __builtin_amdgcn_perm(v.x, v.x, sel), b = __builtin_amdgcn_perm(v.y, v.y, sel);
  const uint32_t c = __builtin_amdgcn_perm(v.z, v.z, sel), d = __builtin_amdgcn_perm(v.w, v.w, sel);
  return make_uint4(flip ? d : a, flip ? c : b, flip ? b : c, flip ? a : d);
}
template <int V>
__global__ __launch_bounds__(256) void lip_augment_collate_kernel(
    const unsigned char* __restrict__ frames, const float* __restrict__ lmk, const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ lens, const float* __restrict__ clip_aug, const int32_t* __restrict__ tmap,
    unsigned char* __restrict__ out, int B, int t_max, int H, int W, int S, int npts, int lo, int hi, float margin) {
  typedef typename CropVec<V>::T vec_t;
  constexpr bool kWide = V != 4;             // (see above)
  constexpr int kLanes = kWide ? 64 : 1;
  __shared__ float box[2][4];
  const int per_row = S / V;                 // S % V == 0 (the launcher picks V)
  const int items = 3 * S * per_row;         // V-pixel groups of one frame
  const int pairs = B * t_max;
  int p = blockIdx.x;                        // (sample, frame) pairs p, p + gridDim.x, ...: uniform per workgroup
  if (p >= pairs) return;
  // the pair whose prologue loads are in flight: its map value (< 0: a frame of zeros), source row and record, and in
  // the first wave each lane's landmark (x0, y0)
  int m;
  int64_t n;
  float dx, dy, zoom, flipf;
  float x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
  auto fetch = [&](int q) {
    const int b = q / t_max, t = q - b * t_max;
    const int rows_b = lens[b];
    const int len = min(rows_b, t_max);      // lens[b] > t_max is the caller's error; never write outside out
    const int64_t first = offsets[b];
    const float* A = clip_aug + (int64_t)b * 4;
    dx = A[0]; dy = A[1]; zoom = A[2]; flipf = A[3];
    m = t < len ? tmap[first + t] : -1;
    n = first + min(max(m, 0), rows_b - 1);  // whatever the map holds, the row is one of sample b's
    if (kWide && hi - lo <= kLanes && m >= 0 && threadIdx.x < kLanes) {   // one point per lane (spare lanes: the last)
      const float* Lq = lmk + n * npts * 3 + (lo + min((int)threadIdx.x, hi - lo - 1)) * 3;
      x0 = Lq[0];
      y0 = Lq[1];
    }
  };
  fetch(p);
  int parity = 0;
  for (;;) {
    const int m_now = m;
    const bool flip = flipf != 0.f;
    const unsigned char* F = frames + n * 3 * H * W;
    vec_t* O = reinterpret_cast<vec_t*>(out + (int64_t)p * 3 * S * S);
    float left = 0.f, top = 0.f, scale = 0.f;
    if (m_now >= 0) {                        // uniform: the barrier is safe
      float* bx = box[parity];
      parity ^= 1;
      if (threadIdx.x < kLanes) {
        if (kWide && hi - lo <= kLanes) {    // prefetched
          x1 = x0;
          y1 = y0;
        } else {
          lip_crop_partial<kLanes>(lmk + n * npts * 3, lo, hi, x0, x1, y0, y1);
        }
        float sx2, sy2, side;
        lip_crop_finish<kLanes>(x0, x1, y0, y1, margin, sx2, sy2, side);
        if (threadIdx.x == 0) {
          const float side_z = fmaxf(side * zoom, 2.f);
          bx[0] = fmaf(dx, side, 0.5f * sx2) - 0.5f * side_z;   // left
          bx[1] = fmaf(dy, side, 0.5f * sy2) - 0.5f * side_z;   // top
          bx[2] = side_z / (float)S;                            // source pixels per output pixel
        }
      }
      __syncthreads();
      left = bx[0]; top = bx[1]; scale = bx[2];
    }
    const int p_next = p + gridDim.x;
    if (p_next < pairs) fetch(p_next);       // in flight while this frame's pixels are made
    if (m_now < 0) {                         // padding or a masked frame
      vec_t zero;
      __builtin_memset(&zero, 0, sizeof(zero));
      for (int i = threadIdx.x; i < items; i += blockDim.x) O[i] = zero;
    } else {
      // mirrored, output column S - 1 - x shows source column x: group g is stored at group per_row - 1 - g with its
      // bytes reversed (4-pixel variant: the group at S - V - ox is computed in place of the one at ox)
      const int mirror = flip ? 1 : 0, src0 = flip && !kWide ? S - V : 0, dir = flip && !kWide ? -1 : 1;
      const uint32_t sel = flip ? 0x00010203u : 0x03020100u;
      for (int i = threadIdx.x; i < items; i += blockDim.x) {
        const int c = i / (S * per_row), r = i - c * S * per_row;
        const int oy = r / per_row, g = r - oy * per_row, ox = g * V;
        const unsigned char* P = F + (int64_t)c * H * W;
        union { vec_t v; unsigned char px[V]; } u;
        const int src = kWide ? ox : src0 + dir * ox;
#pragma unroll
        for (int k = 0; k < V; ++k) u.px[k] = lip_crop_pixel(P, H, W, oy, src + k, left, top, scale);
        O[kWide ? i + mirror * (per_row - 1 - 2 * g) : i] = crop_vec_mirror(u.v, flip, sel);
      }
    }
    if (p_next >= pairs) break;
    p = p_next;
  }
}

// collate_pad_kernel with the source row of every frame taken from tmap (< 0: a masked, all-zero row)
__global__ void collate_pad_aug_kernel(const float* __restrict__ packed, const int64_t* __restrict__ offsets,
                                       const int32_t* __restrict__ lens, const int32_t* __restrict__ tmap,
                                       float* __restrict__ out, int B, int t_max, int feat) {
  const int64_t total = (int64_t)B * t_max * feat;
  const int64_t row_elems = (int64_t)t_max * feat;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / row_elems);
    const int64_t r = i - (int64_t)b * row_elems;
    const int t = (int)(r / feat);
    const int f = (int)(r - (int64_t)t * feat);
    const int len = lens[b];
    float v = 0.f;
    if (t < len) {
      const int m = tmap[offsets[b] + t];
      if (m >= 0) v = packed[(offsets[b] + min(m, len - 1)) * feat + f];
    }
    out[i] = v;
  }
}
}  // namespace

extern "C" int lr_lip_crop_collate_aug_u8(const void* frames, const float* lmk, const int64_t* offsets,
                                          const int32_t* lens, const float* clip_aug, const int32_t* tmap, void* out,
                                          int B, int t_max, int H, int W, int S, int npts, int lo, int hi, float margin,
                                          lr_stream_t stream) {
  LR_CHECK_ARG(frames && lmk && offsets && lens && clip_aug && tmap && out);
  LR_CHECK_ARG(B > 0 && t_max > 0 && H > 0 && W > 0 && S > 0);
  LR_CHECK_ARG(npts > 0 && lo >= 0 && hi > lo && hi <= npts && margin >= 0.f);
  LR_CHECK_ARG((int64_t)B * t_max <= INT32_MAX && (int64_t)S * S <= INT32_MAX / 3);
  const int pairs = B * t_max;
  const dim3 grid(pairs < 2048 ? pairs : 2048);   // 256 CUs x 8 workgroups; the rest by the grid stride
  const unsigned char* f = (const unsigned char*)frames;
  unsigned char* o = (unsigned char*)out;
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;   // as lr_lip_crop_collate_u8
  if (aligned && S % 16 == 0) {
    LR_LAUNCH(lip_augment_collate_kernel<16>, grid, dim3(256), 0, stream, f, lmk, offsets, lens, clip_aug, tmap, o, B,
              t_max, H, W, S, npts, lo, hi, margin);
  } else if (aligned && S % 4 == 0) {
    LR_LAUNCH(lip_augment_collate_kernel<4>, grid, dim3(256), 0, stream, f, lmk, offsets, lens, clip_aug, tmap, o, B,
              t_max, H, W, S, npts, lo, hi, margin);
  } else {
    LR_LAUNCH(lip_augment_collate_kernel<1>, grid, dim3(256), 0, stream, f, lmk, offsets, lens, clip_aug, tmap, o, B,
              t_max, H, W, S, npts, lo, hi, margin);
  }
  return lr_launch_status();
}

extern "C" int lr_collate_pad_aug_f32(const float* packed, const int64_t* offsets, const int32_t* lens,
                                      const int32_t* tmap, float* out, int B, int t_max, int feat, lr_stream_t stream) {
  LR_CHECK_ARG(packed && offsets && lens && tmap && out);
  LR_CHECK_ARG(B > 0 && t_max > 0 && feat > 0);
  const int64_t total = (int64_t)B * t_max * feat;
  LR_LAUNCH(collate_pad_aug_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, packed, offsets, lens, tmap, out, B,
            t_max, feat);
  return lr_launch_status();
}

// ---- instrumentation ----------------------------------------------------------------------------
namespace {
constexpr int kProfRing = 1024;
struct ProfSlot {
  hipEvent_t start[kProfRing], stop[kProfRing];
  int count;
  bool ready;
};
ProfSlot g_prof[LR_PROF_SLOTS];
bool g_prof_on = false;
}  // namespace

bool lr_prof_next(int slot, hipEvent_t* start, hipEvent_t* stop) {
  if (!g_prof_on || slot < 0 || slot >= LR_PROF_SLOTS) return false;
  ProfSlot& p = g_prof[slot];
  if (!p.ready || p.count >= kProfRing) return false;
  *start = p.start[p.count];
  *stop = p.stop[p.count];
  ++p.count;
  return true;
}

extern "C" int lr_profile_enable(int on) {
  if (on && !g_prof_on) {
    for (int w = 0; w < LR_PROF_SLOTS; ++w) {
      ProfSlot& p = g_prof[w];
      if (!p.ready) {
        for (int i = 0; i < kProfRing; ++i) {
          if (hipEventCreate(&p.start[i]) != hipSuccess || hipEventCreate(&p.stop[i]) != hipSuccess) {
            (void)hipGetLastError();
            return LR_ERR_NO_DEVICE;
          }
        }
        p.ready = true;
      }
      p.count = 0;
    }
  }
  g_prof_on = on != 0;
  return LR_OK;
}

extern "C" int lr_profile_read(int which, float* total_ms_host, int* samples_host) {
  LR_CHECK_ARG(which >= 0 && which < LR_PROF_SLOTS && total_ms_host && samples_host);
  ProfSlot& p = g_prof[which];
  float total = 0.f;
  int n = 0;
  for (int i = 0; i < p.count; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(p.stop[i]) == hipSuccess &&
        hipEventElapsedTime(&ms, p.start[i], p.stop[i]) == hipSuccess) {
      total += ms;
      ++n;
    }
  }
  (void)hipGetLastError();
  p.count = 0;
  *total_ms_host = total;
  *samples_host = n;
  return LR_OK;
}
