/*
 * lipreading_hip.h — C ABI of the MI355X (gfx950) hot path of joseph-zhong/LipReading:
 * landmark step -> recurrent sequence encoder -> CTC loss / greedy decode.
 *
 * The reference has no FFI of its own (it is pure Python over stock torch ops), so this
 * ABI is the build's design; every entry point names the reference symbol (file:line under
 * the reference root) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - every function only ENQUEUES work on `stream` (a hipStream_t passed as void*); it never
 *     allocates, frees, synchronises or copies to the host, so a whole training step can be
 *     captured in one hipGraph.  TWO exceptions, both outside any captured region:
 *       (1) the per-device fault words (16 bytes: {recurrence timed out, 3 spare}) are
 *           hipMalloc'ed + hipMemset the FIRST time any entry point needs them on a device;
 *           call lr_fault_words_ptr() once per device before capturing (lipreading_amd.train's
 *           StepGraphs does: its first steps of a shape run eagerly) — afterwards nothing
 *           allocates again for the life of the process;
 *       (2) the host-side readers lr_rnn_pair_errors / lr_profile_read
 *           synchronise the device and copy a few words back: diagnostics, never on a step;
 *   - scratch comes from the caller: ask `*_workspace_bytes`, pass the buffer back in;
 *   - return value: LR_OK (0) or a negative lr_status; no C++ exception crosses the boundary;
 *   - all floating point is IEEE fp32 (subnormals kept), all indices int32 unless noted.
 */
#ifndef LIPREADING_HIP_H
#define LIPREADING_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lr_stream_t; /* hipStream_t */

typedef enum lr_status {
  LR_OK = 0,
  LR_ERR_INVALID_ARG = -1, /* null pointer, negative size, unsupported shape            */
  LR_ERR_WORKSPACE = -2,   /* caller workspace smaller than *_workspace_bytes()          */
  LR_ERR_LAUNCH = -3,      /* hipLaunchKernel / hipGetLastError reported a failure       */
  LR_ERR_UNSUPPORTED = -4, /* valid request outside what the kernels implement           */
  LR_ERR_NO_DEVICE = -5    /* no gfx950 device visible                                   */
} lr_status;

typedef enum lr_rnn_mode {
  LR_RNN_GRU = 0, /* torch.nn.GRU  gate order r,z,n   (3 gates) */
  LR_RNN_LSTM = 1, /* torch.nn.LSTM gate order i,f,g,o (4 gates) */
  LR_RNN_TANH = 2, /* torch.nn.RNN (nonlinearity='tanh'): h' = tanh(W_ih x + b_ih + W_hh h + b_hh) (1 "gate");
                      better_model.py:9 allows rnn_type='RNN' */
  LR_RNN_CELL_MASK = 0xff,
  /* Optional flags OR-ed into `mode` of lr_rnn_layer_* / lr_rnn_*_bytes (build-defined, used by
   * the pixel regime only; the reference-faithful path passes none and stays on exact fp32 MFMA):
   * contract the layer's INPUT projection (x W_ih^T, and its two gradients) on the bf16 matrix
   * cores with every fp32 operand split into bf16 hi + lo terms (~1e-5 relative, lr_xgemm). */
  LR_RNN_PROJ_BF16X3 = 0x100,
  /* with LR_RNN_PROJ_BF16X3: the layer input is the bf16 conv frontend's output — every element
   * of x is already a bf16 value, so x needs no lo term, and dx goes to a bf16 consumer (the
   * frontend's backward), so dx is contracted from the hi terms only. */
  LR_RNN_INPUT_BF16_EXACT = 0x200,
  /* (0x400: rounds 1-4's single-plane bf16 recurrence, LR_RNN_RECUR_BF16 — removed in round 5: no shipped
   * configuration ran it once the fp32-faithful one-launch kernels below covered every size) */
  /* with LR_RNN_PROJ_BF16X3 | LR_RNN_INPUT_BF16_EXACT and I % 8 == 0: x (and dx) are STORED as bf16
   * matrices [B*T][I] — the conv frontend's features as they are; x is then the hi plane of the
   * projection's operand and is never converted or packed. */
  LR_RNN_INPUT_STORED_BF16 = 0x800,
  /* The recurrence of a supported layer (lr_rnn_pair_supported != 0: GRU or LSTM, H % 4 == 0, H up to the largest
   * cluster — the reference's config/defaults.txt:19-21, config/train/attn/attention_type:16-19, config/train/micro:6-8
   * and the decoders behind them, better_model.py:134-148) as ONE launch per pass and fp32-FAITHFUL: W_hh and the
   * carried state are split into bf16 hi + lo planes, all four cross terms accumulate in fp32 on the bf16 matrix cores
   * (~1e-6 of the exact fp32 product).  W_hh stays in the registers + LDS of a cluster of ceil(H / 32) (past 864 /
   * 768 units: ceil(H / 16)) compute units per (direction, 8 samples), which exchange their slices of the state
   * (forward) / their partial state gradients (backward) once per step (lr_rnn_cluster.hip).  What the
   * reference-faithful regime runs by default where it is supported; the decoder loop (lr_decoder_forward /
   * _backward) takes the same cluster kernels, started from the encoder's final state, when every step is
   * teacher forced. */
  LR_RNN_RECUR_SPLIT = 0x1000,
  /* with LR_RNN_PROJ_BF16X3: keep only the bf16 hi plane of both operands of the input projection — one product
   * instead of two or three (~2^-9 relative).  A FORWARD-ONLY experiment of the build-defined pixel regime
   * (encoder.input_projection = 'bf16x1'), compared with the default in bench.py's parity block; the backward
   * answers LR_ERR_UNSUPPORTED. */
  LR_RNN_PROJ_BF16X1 = 0x2000
} lr_rnn_mode;

typedef enum lr_ctc_reduction {
  LR_CTC_SUM = 0, /* reference reduction='sum'  (src/train/ctc_loss.py:114) */
  LR_CTC_MEAN = 1 /* reference reduction='mean' incl. its run-weighting quirk (:74,:103-105) */
} lr_ctc_reduction;

/* ---- library ------------------------------------------------------------------------- */

/* ABI version: major*10000 + minor*100 + patch. */
int lr_version(void);
/* Static string for a status code (never NULL). */
const char* lr_status_string(int status);
/* Number of visible HIP devices (0 when none); does not create a context. */
int lr_device_count(void);

/* ---- A1: batch collation — src/data/data_loader.py:117-152 (_collate_fn, _pad) --------- */

/* Zero-pad ragged rows to the batch maximum on the device.
 *   packed   [sum(lens), feat]   rows of all samples back to back (sample b starts at
 *                                row offsets[b])
 *   offsets  [B] int64, lens [B] int32
 *   out      [B, t_max, feat]    out[b,t,:] = t < lens[b] ? packed[offsets[b]+t,:] : 0
 * Replaces the per-sample torch.Tensor(seq) copy loop of _pad (:139-141). */
int lr_collate_pad_f32(const float* packed, const int64_t* offsets, const int32_t* lens,
                       float* out, int B, int t_max, int feat, lr_stream_t stream);

/* ---- A7: landmark step — src/utils/data/face.py:76-90,164-175 -------------------------- */

/* _applyPadding (face.py:76-90) for n rectangles, integer arithmetic identical to the
 * reference: left = max(0, left - int(padding*box_w)) ... ; rect layout (left,right,top,bottom).
 *   rects_in/out [n,4] int32, dims [n,2] int32 = (img_h, img_w). */
int lr_lmk_apply_padding(const int32_t* rects_in, const int32_t* dims, int32_t* rects_out,
                         int n, float padding, lr_stream_t stream);

/* getFace (face.py:164-175): out[i,p,0] = in[i,p,0]-left_i; out[i,p,1] = in[i,p,1]-top_i;
 * z untouched.  lmk [n, npts, 3] f32, rects [n,4] int32 (left,right,top,bottom).  in==out ok. */
int lr_lmk_translate(const float* lmk_in, const int32_t* rects, float* lmk_out, int n,
                     int npts, lr_stream_t stream);

/* PRNet crop geometry (src/models/face/prnet.py:112-119,136-140, image_info = the UNPADDED face rect
 * as generate_dataview.py:62 passes it): old = (r-l+b-t)/2, centre of the box, size = int(old*1.6),
 * similarity transform of the crop square onto resolution x resolution (what the reference obtains
 * from skimage.transform.estimate_transform('similarity', ...)).
 *   rects [n,4] int32 (left,right,top,bottom) -> tform [n,3,3] float64 row-major, sizes [n] int32 (NULL ok) */
int lr_lmk_crop_transform(const int32_t* rects, double* tform, int32_t* sizes, int n, int resolution,
                          lr_stream_t stream);

/* Restore (prnet.py:150-156): the network's position map of the crop -> image coordinates:
 * z /= tform[0][0]; [x y] = (tform^-1 [x y 1])[0:2].
 *   cropped_pos [n, npix, 3] f32 (PosPrediction.predict's output, prnet.py:304-309), tform [n,3,3] f64
 *   -> pos [n, npix, 3] f64 (np.dot's result type). */
int lr_lmk_restore(const float* cropped_pos, const double* tform, double* pos, int n, int64_t npix,
                   lr_stream_t stream);

/* get_landmarks (prnet.py:162-170): kpt[i,k,:] = pos[i, uv[1][k], uv[0][k], :]; with `rects` non-NULL
 * also getFace's translation by (left, top) of rects[i] (face.py:164-175).
 *   pos [n,res,res,3] f64, uv_kpt_ind [2,K] int32, rects [n,4] int32 or NULL -> kpt [n,K,3] f64 */
int lr_lmk_gather(const double* pos, const int32_t* uv_kpt_ind, const int32_t* rects, double* kpt, int n,
                  int resolution, int K, lr_stream_t stream);

/* The arithmetic of _gen_data (src/scripts/generate_dataview.py:58-64) around the two networks, in one
 * launch: padded rect = _applyPadding(dims, rect, padding) (extractFace, :61); the UNPADDED rect
 * defines the PRNet crop (:62); the K landmark points are gathered from the position map, restored
 * to image coordinates and translated by the PADDED rect (:64).
 *   cropped_pos [n,res,res,3] f32, rects [n,4], dims [n,2] = (img_h, img_w), uv_kpt_ind [2,K]
 *   -> lmk_f64 [n,K,3] and/or lmk_f32 [n,K,3] (either may be NULL), rects_padded [n,4] (NULL ok) */
int lr_lmk_landmarks(const float* cropped_pos, const int32_t* rects, const int32_t* dims, double padding,
                     const int32_t* uv_kpt_ind, double* lmk_f64, float* lmk_f32, int32_t* rects_padded,
                     int n, int resolution, int K, lr_stream_t stream);

/* A9 (BUILD-DEFINED, no reference symbol: face.py:21 defines `_mouth = slice(48,68)` and never uses
 * it): crop the mouth region and resample it to S x S.  Per frame: bounding box of landmarks
 * [lo,hi) (x = lmk[..,0], y = lmk[..,1], image pixels) -> centre, side = max(w,h)*(1+2*margin)
 * (>= 2 px) -> bilinear resize with half-pixel centres and edge clamping, rounded to uint8.
 *   frames uint8 [n][3][H][W], lmk f32 [n][npts][3], out uint8 [n][3][S][S]. */
int lr_lip_crop_u8(const void* frames, const float* lmk, void* out, int n, int H, int W, int S, int npts,
                   int lo, int hi, float margin, lr_stream_t stream);

/* A9 for a whole ragged batch, written straight into the zero-padded batch in ONE launch (the loader's hot path).
 *   frames  uint8 [sum(lens)][3][H][W]   samples back to back
 *   lmk     f32   [sum(lens)][npts][3]
 *   offsets [B] int64  index of sample b's first frame;  lens [B] int32, 1 <= lens[b] <= t_max
 *   out     uint8 [B][t_max][3][S][S]:
 *           out[b,t] = t < lens[b] ? crop(frames[offsets[b]+t], lmk[offsets[b]+t]) : 0
 * crop() is lr_lip_crop_u8's arithmetic (one shared device function): the bytes are identical to B per-sample calls
 * into a zeroed batch.  EVERY byte of out is written, so the caller allocates it uninitialised.  lens[b] > t_max is
 * the caller's error and is clamped (nothing is written outside out). */
int lr_lip_crop_collate_u8(const void* frames, const float* lmk, const int64_t* offsets, const int32_t* lens,
                           void* out, int B, int t_max, int H, int W, int S, int npts, int lo, int hi, float margin,
                           lr_stream_t stream);

/* lr_lip_crop_collate_u8 with training-time clip augmentation applied inside the same launch.  The host draws
 * (lipreading_amd/augment.py), the kernel applies: no random number is made on the device.
 *   clip_aug f32 [B][4] = (dx, dy, zoom, flip) per CLIP;  tmap int32 [sum(lens)], indexed like the frames:
 *   tmap[offsets[b]+t] = source frame of output frame t within sample b, or < 0 for a masked frame.
 *   out[b,t] = 0                                   for t >= min(lens[b], t_max) or tmap[offsets[b]+t] < 0
 *            = crop'(row n = offsets[b] + min(tmap[offsets[b]+t], lens[b]-1))   otherwise
 * (a map value past the sample is clamped: no row of another sample is ever read).  crop' starts from the centre
 * (cx, cy) and side of lr_lip_crop_u8's window of row n:  side' = max(side*zoom, 2),
 * left = fmaf(dx, side, cx) - side'/2, top likewise with dy, scale = side'/S, and output pixel (oy, ox) is
 * lr_lip_crop_u8's pixel (oy, flip != 0 ? S-1-ox : ox) of that window: the shift is in units of the un-zoomed side,
 * the flip mirrors output columns.  The identity record (0,0,1,0) with tmap[t] = t gives lr_lip_crop_collate_u8's
 * bytes.  Source coordinates are clamped to the frame, so no value of the record reads outside it; keeping the
 * values in range is the host's job.  EVERY byte of out is written. */
int lr_lip_crop_collate_aug_u8(const void* frames, const float* lmk, const int64_t* offsets, const int32_t* lens,
                               const float* clip_aug, const int32_t* tmap, void* out, int B, int t_max, int H, int W,
                               int S, int npts, int lo, int hi, float margin, lr_stream_t stream);

/* lr_collate_pad_f32 with the same frame map (landmark regime: temporal jitter and time masks only):
 *   out[b,t,:] = t < lens[b] ? (m < 0 ? 0 : packed[offsets[b] + min(m, lens[b]-1), :]) : 0,  m = tmap[offsets[b]+t] */
int lr_collate_pad_aug_f32(const float* packed, const int64_t* offsets, const int32_t* lens, const int32_t* tmap,
                           float* out, int B, int t_max, int feat, lr_stream_t stream);

/* ---- A9, stabilised: mouth crops of fixed scale, roll-corrected, smoothed over time (BUILD-DEFINED) ---------- */

/* lr_lip_crop_collate_aug_u8's batch with another window rule.  The box rule cuts the bounding box of the mouth points
 * of one frame: its scale follows the mouth's opening, it shakes with the landmark noise and it keeps the head's roll.
 * Here scale and roll come from the EYES, which do not move with speech, the centre is the mouth points' MEAN, and all
 * of it is averaged over 2*radius+1 neighbouring frames of the same sample.
 *   pose of row n (four fp32):  mx, my = mean of x, y over landmarks [lo,hi);  (ax, ay) = mean over [eb_lo,eb_hi)
 *     minus mean over [ea_lo,ea_hi) (one fp32 subtraction each).  Every mean is a float64 sum in ascending index,
 *     divided in float64 by the count, rounded once to fp32.
 *   smoothed pose of row n = row i of a sample of len rows: each component's float64 sum over rows
 *     max(0,i-radius) .. min(len-1,i+radius) in ascending order / count, rounded once to fp32 (radius 0: the raw pose).
 *     The window never leaves the sample, whatever t_max is.
 *   window, all fp32, every a + b*c one fmaf, (dx,dy,zoom,flip) = clip_aug[b] or (0,0,1,0) when clip_aug is NULL:
 *     d = sqrtf(fmaf(ay,ay,ax*ax));  if !(extent*d*zoom >= 2) { ax = 2/(extent*zoom); ay = 0; }   (the 2-pixel minimum)
 *     ex = extent*ax, ey = extent*ay;  cx = fmaf(-dy,ey,fmaf(dx,ex,mx));  cy = fmaf(dy,ex,fmaf(dx,ey,my));
 *     ux = (ex*zoom)/S, uy = (ey*zoom)/S     — the side is `extent` eye distances, the shift is in units of the
 *     un-zoomed side along the window's own axes.
 *   output pixel (oy,ox): px = (ox+0.5f) - 0.5f*S, py likewise;  sx = fmaf(-py,uy,fmaf(px,ux,cx)) - 0.5f,
 *     sy = fmaf(py,ux,fmaf(px,uy,cy)) - 0.5f;  from there lr_lip_crop_u8's arithmetic (clamp to the frame, floor, three
 *     fmaf lerps, round to nearest).  flip != 0: output column S-1-ox shows what column ox would.
 * Batch semantics are lr_lip_crop_collate_aug_u8's: tmap NULL means tmap[offsets[b]+t] = t; zeros for
 * t >= min(lens[b], t_max) and for a map value < 0; the source row is offsets[b] + min(map value, lens[b]-1) and the
 * pose is that SOURCE row's, smoothed over its source neighbours; EVERY byte of out is written; out need not be 16-byte
 * aligned.  clip_aug and tmap are both NULL or both given.  NaN landmarks give unspecified pixels, never a read
 * outside the frame.
 *   pose      f32 [rows][4] or NULL: the smoothed (mx, my, ax, ay) of every row of every sample
 *   workspace lr_lip_stable_workspace_bytes(rows, radius) bytes, 16-byte aligned (LR_ERR_WORKSPACE when too small)
 * Two launches: the poses of all rows (one workgroup per sample), then the pixels. */
#define LR_LIP_STABLE_MAX_RADIUS 32
size_t lr_lip_stable_workspace_bytes(int64_t rows, int radius); /* 0 for arguments it rejects */
int lr_lip_stable_collate_u8(const void* frames, const float* lmk, const int64_t* offsets, const int32_t* lens,
                             const float* clip_aug, const int32_t* tmap, void* out, float* pose, void* workspace,
                             size_t workspace_bytes, int B, int64_t rows, int t_max, int H, int W, int S, int npts,
                             int lo, int hi, int ea_lo, int ea_hi, int eb_lo, int eb_hi, float extent, int radius,
                             lr_stream_t stream);

/* ---- Landmark pose: every frame's landmarks aligned to a canonical face inside the collate launch (BUILD-DEFINED) - */

/* lr_collate_pad_aug_f32's batch with the head's translation, rotation and (optionally) scale taken out of every
 * frame: a rigid or similarity alignment to the template `tmpl`, estimated from points that do not move with speech
 * (`rigid`: nose bridge, eye corners) and applied to all npts points.
 *   lmk     f32 [rows][npts][3]  samples back to back;  offsets, lens, tmap, t_max as in lr_collate_pad_aug_f32
 *           (tmap may be NULL: the identity)
 *   tmpl    f32 [npts][3]        the canonical face, on the device
 *   rigid_host                   HOST array of n_rigid distinct point indices (handed to the kernel by value)
 *   radius                       half-width of the smoothing window;  flags & LR_POSE_SCALE: similarity, else s = 1
 * All arithmetic is float64, inputs widened from fp32, every output value rounded to fp32 once.
 *   per source row n, p_i = lmk[n][rigid[i]], q_i = tmpl[rigid[i]]:  pbar_n, qbar = the means over i;
 *     M_n = sum_i (q_i - qbar)(p_i - pbar_n)^T  (3x3);  v_n = sum_i |p_i - pbar_n|^2;
 *     a row with a non-finite value among its npts*3 coordinates is BAD.
 *   window, row n = row i of a sample of len rows: M~_n, v~_n = the sums of M_m, v_m over the non-BAD rows m in
 *     max(0,i-radius) .. min(len-1,i+radius) of the same sample, ascending.  The window never leaves the sample.
 *     The translation is not smoothed: it is row n's own pbar_n.
 *   solve: R~_n = the proper rotation (det = +1) that maximises tr(R M~_n^T) — for M~ = U S V^T,
 *     R = U diag(1, 1, det(U V^T)) V^T;  s~_n = tr(R~_n M~_n^T) / v~_n with LR_POSE_SCALE, else 1.  (Here: the
 *     eigenvector of Horn's 4x4 symmetric matrix with the largest eigenvalue, by a fixed number of cyclic Jacobi
 *     sweeps.)  Where the maximiser is not unique (collinear rigid points) any maximiser may come out; it is finite.
 *   out[b][t][j][:] = fp32( s~_n R~_n (lmk[n][j] - pbar_n) + qbar ), n = offsets[b] + min(m, lens[b]-1),
 *     m = tmap[offsets[b]+t];  zeros for t >= min(lens[b], t_max), for m < 0 and for a BAD source row.  EVERY element
 *     of out is written.
 *   status int32 [rows]: LR_POSE_OK the row was normalised; LR_POSE_DEGENERATE the window has no usable row or
 *     v~_n == 0, then R = I and s = 1; LR_POSE_BAD_ROW the row has a non-finite coordinate.
 *   pose   f32 [rows][13] or NULL: R~ row-major, s~, pbar (a BAD row: I, 1, 0).  pose and status cover every row of
 *     every sample, whatever tmap says (as lr_lip_stable_collate_u8's pose).
 *   workspace lr_lmk_pose_workspace_bytes(rows, n_rigid, radius) bytes, 16-byte aligned.
 * Every sum has a fixed order and there are no atomics: two launches give the same bits, and a batch gives the bits of
 * B one-sample calls.  Errors, all before any launch: 3 <= n_rigid <= LR_POSE_MAX_RIGID, 1 <= npts <=
 * LR_POSE_MAX_POINTS, 0 <= radius <= LR_POSE_MAX_RADIUS or an unknown flag bit -> LR_ERR_UNSUPPORTED; a rigid index
 * outside [0, npts) or a repeated one, a NULL required pointer, rows > 2^31-1 -> LR_ERR_INVALID_ARG; LR_ERR_WORKSPACE.
 * Two launches: the rows' statistics (one wave per row), then one wave per (sample, frame). */
#define LR_POSE_MAX_RADIUS 32
#define LR_POSE_MAX_RIGID 64
#define LR_POSE_MAX_POINTS 256
#define LR_POSE_SCALE 1
#define LR_POSE_OK 0
#define LR_POSE_DEGENERATE 1
#define LR_POSE_BAD_ROW 2
size_t lr_lmk_pose_workspace_bytes(int64_t rows, int n_rigid, int radius); /* 0 for arguments it rejects */
int lr_lmk_pose_collate_f32(const float* lmk, const int64_t* offsets, const int32_t* lens, const int32_t* tmap,
                            const float* tmpl, const int32_t* rigid_host, int n_rigid, float* out, float* pose,
                            int32_t* status, void* workspace, size_t workspace_bytes, int B, int64_t rows, int t_max,
                            int npts, int radius, int flags, lr_stream_t stream);

/* ---- Landmark augmentation: one 3x3 matrix, a shift and noise per clip, on a collated batch (BUILD-DEFINED) -------- */

/* Training-time augmentation of a COLLATED landmark batch: it runs behind lr_collate_pad_f32, lr_collate_pad_aug_f32 or
 * lr_lmk_pose_collate_f32, so frame maps, masked frames, padding and pose are settled and neither tmap nor the pose
 * status is needed.  The host draws (lipreading_amd/augment.py, LandmarkAugmentSpec), the kernel applies.
 *   x, y        f32 [B][t_max][npts][3]; they may be the same buffer (in place), otherwise they must not overlap
 *   lens        int32 [B] on the device, clamped into [0, t_max]
 *   mirror_perm int32 [npts] on the device: the left/right partner of every point
 *   clip_stats  f64 [B][4] = (c_x, c_y, c_z, r), or NULL
 *   workspace   lr_lmk_augment_workspace_bytes(B) bytes, 16-byte aligned
 *   rec         16 eight-byte words per clip: words 0-8 A row-major f64; 9-11 shift f64; 12 jitter f64; 13 mirror f64
 *               (0 or 1); 14 key, read as uint64; 15 zero.  The host folds everything linear into A (rotation, scale,
 *               stretch, the mirror's sign flip): the device never evaluates a sine.
 * All arithmetic is float64, inputs widened from fp32, every output value rounded to fp32 once.
 *   EMPTY rows: row (b, t) is EMPTY when t >= min(lens[b], t_max), when all npts*3 of its values are zero of either
 *     sign, or when any of its values is not finite.  Padding, masked frames and the pose entry's BAD rows are exactly
 *     the all-zero rows, which is why nothing else is needed to recognise them.  The other rows are LIVE.
 *   clip statistics, over the LIVE rows of clip b, n = LIVE rows * npts:  c_b = sum x / n;
 *     r_b = sqrt(max(sum |x|^2 / n - |c_b|^2, 0));  a clip without a LIVE row has c = 0, r = 0.  The sums have a fixed
 *     order that does not depend on B, on the other clips or on the launch.
 *   noise (no transcendental function, so it is exact on host and device): mix = the splitmix64 finaliser
 *     (augment._mix), GOLDEN = 0x9E3779B97F4A7C15;  z = mix(key_b + GOLDEN + uint64((t*npts + j)*3 + k)), wrapping,
 *     with t, j, k the OUTPUT frame, point and coordinate;  S = the sum of the four 16-bit fields of z;
 *     g = double(S - 131070) * 2.6428997921303014e-05 (1 over the standard deviation of the sum of four uniform 16-bit
 *     integers: g has unit variance).  The noise is evaluated only where jitter != 0.
 *   LIVE rows:  y[b][t][j][k] = fp32( sum_l A[k][l] * (x[b][t][j'][l] - c_l) + c_k + r_b * (shift_k + jitter * g) ),
 *     j' = mirror_perm[j] when mirror != 0, else j;  j' is clamped into [0, npts) inside the kernel: no value of
 *     mirror_perm can read outside the row.
 *   EMPTY rows: all zeros.  EVERY element of y is written.
 * Two launches give the same bits, a batch gives the bits of B one-clip calls, in place gives the bits of out of place.
 * Errors, all before any launch: npts outside [1, LR_LMK_AUG_MAX_POINTS], B < 1, t_max < 1 or B*t_max >= 2^31 ->
 * LR_ERR_UNSUPPORTED; a NULL required pointer, or x and y overlapping without being equal -> LR_ERR_INVALID_ARG; a
 * workspace that is too small -> LR_ERR_WORKSPACE.
 * Two launches: the clips' statistics (one workgroup per clip), then one wave per row. */
#define LR_LMK_AUG_MAX_POINTS 256
#define LR_LMK_AUG_REC_WORDS 16
size_t lr_lmk_augment_workspace_bytes(int B); /* 0 for arguments it rejects */
int lr_lmk_augment_f32(const float* x, const int32_t* lens, const void* rec, const int32_t* mirror_perm, float* y,
                       double* clip_stats, void* workspace, size_t workspace_bytes, int B, int t_max, int npts,
                       lr_stream_t stream);

/* ---- dense fp32 contraction (MFMA f32 16x16x4 / 32x32x2), used by A3 ------------------- */

/* C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] + beta * C + bias[N]   (row-major, fp32)
 *   transA=0: A is [M,K] lda>=K ; transA=1: A is [K,M] lda>=M   (same for B with N)
 *   bias may be NULL.  beta==0 never reads C.
 *   row_shift/period: when period>0, row k of the K dimension of op(B) (transB=0 storage
 *   [K,N]) is taken from row k+row_shift if 0 <= (k % period)+row_shift < period, else it
 *   is zero — the "previous hidden state" view of a [B*T, H] matrix without a copy.
 *   workspace: lr_sgemm_workspace_bytes(M,N,K) bytes enable a deterministic split along K
 *   when M*N alone cannot fill the chip (weight gradients: K = B*T); NULL/0 = no split. */
size_t lr_sgemm_workspace_bytes(int M, int N, int K);
int lr_sgemm(int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
             const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
             int row_shift, int period, void* workspace, size_t workspace_bytes,
             lr_stream_t stream);

/* ---- A3: recurrent layer — src/models/lipreader/better_model.py:47-49,64-89 ------------ */

/* One (bi)directional GRU/LSTM layer with torch packed-sequence semantics
 * (pack_padded_sequence -> nn.GRU/LSTM -> pad_packed_sequence, better_model.py:68-78),
 * WITHOUT the length sort: every sample stops at its own length, the reverse direction
 * starts at each sample's last valid frame, positions past a length are zero in y and the
 * final state is the state at each sample's last valid step.
 *
 *   x      [B,T,I]        layer input, batch-first, contiguous
 *   lens   [B] int32      1 <= lens[b] <= T
 *   w_ih   D pointers -> [G*H, I]   (torch weight_ih_l{k}[_reverse])
 *   w_hh   D pointers -> [G*H, H]
 *   b_ih, b_hh  D pointers -> [G*H]
 *   y      [B,T,D*H]      outputs (direction d in columns [d*H,(d+1)*H))
 *   h_n    [D,B,H]        final hidden state; c_n [D,B,H] (LSTM; may be NULL for GRU)
 *                         h_n may be NULL: the final states are not extracted (one launch less; c_n is then ignored
 *                         and may be NULL for an LSTM too) — y and every gradient are the same bits either way
 *   I is any positive size and the W_ih pointers need no alignment: a layer whose I is no multiple of 4, or whose
 *   W_ih is not 16-byte aligned, takes element loads in its input projection (tests/test_gpu_rnn_fp64.py)
 *   reserve               saved activations for the backward pass (lr_rnn_reserve_bytes)
 * Pointer arrays (w_ih ...) are HOST arrays of D device pointers. */
int lr_rnn_pair_supported(int mode, int B, int T, int I, int H, int D);         /* see LR_RNN_RECUR_SPLIT: 2 or 0 */
/* ... and why not: 0 = the layer has a one-launch recurrence on this device now; 1 = no kernel for the shape; 2 =
 * switched off by lr_rnn_one_launch_enable(0); 3 = switched off by the test hook lr_rnn_debug_disable_cluster; 4 = the
 * device has too few compute units for a launch's clusters.  (What a caller says when it falls back.) */
int lr_rnn_one_launch_status(int mode, int B, int T, int I, int H, int D);
/* Recurrence launches ONE pass (forward or backward) of the layer takes on this device: 1 where every (direction,
 * 8 samples) cluster of the batch fits one launch — up to 8 * floor(32 / members) clusters, members = ceil(H / 32):
 * BiGRU-256 up to B = 128, BiLSTM-512 up to B = 64 (BASELINE configs[3]'s whole batch on one GPU); clusters of 17 .. 24
 * members (one per XCD: BiLSTM-700 / 768) take SIXTEEN samples each once the batch needs more than eight of them:
 * BiLSTM-768 one launch up to B = 64, two at the ecd files' B = 128 —, more where the batch is cut into several
 * launches, T where the layer runs one launch per time step; LSTM past 1152 units: one launch per direction and 64
 * samples. */
int lr_rnn_pass_launches(int mode, int B, int T, int I, int H, int D);
/* LR_RNN_RECUR_SPLIT's workgroups of a pair / cluster must be resident together (lr_rnn_pair_supported checks the
 * device's compute-unit count); their waits are bounded, and a member that gave up leaves garbage and raises the
 * device-side FAULT WORD.  The reference's contract for a batch it cannot use is assert / `None` => skip
 * (src/train/train_better_model.py:46-50); here, with no host round trip:
 *   fault words  int32[2] on the device, {pending, total}.  A recurrence that timed out ORs 1 into `pending`;
 *                lr_ctc_reduce then reports the batch as skipped (loss 0, status 2, zero gradient weights) and
 *                lr_adam_step leaves parameters, moments and step count untouched, exactly as for skip != 0;
 *                lr_step_begin (the top of the next step) moves `pending` into `total`.
 * lr_fault_words_ptr   device pointer to the two words (allocated on the first call — never call it first under
 *                      stream capture), NULL if that failed.
 * lr_rnn_pair_errors   pending + total since the last call, and clears both; synchronises the device (once per
 *                      epoch in train(), tests, bench).
 * lr_step_begin        zeroes the flat gradient buffer grad[0..n) (16-byte aligned; what opt.zero_grad() does,
 *                      train_better_model.py:67) and rolls the fault words; also_zero (may be NULL): TWO more words
 *                      to clear (lr_clip_adam_step's `sumsq`: the accumulator and its ticket); one launch.
 * lr_rnn_debug_drop_member   TEST HOOK: member `m` (>= 0) of every pair / cluster returns at once, so its partners
 *                      time out (a few tenths of a second) and raise the fault; -1 (default) = off.
 * lr_rnn_debug_disable_cluster   TEST HOOK: bit 0 makes lr_rnn_pair_supported answer 0 for the cluster shapes
 *                      (and the decoder loop take its step kernels), so the one-launch and the per-step recurrences
 *                      can be compared on one model; the other bits have no effect.  Size queries depend on it: set
 *                      it BEFORE the forward whose backward it should cover.
 * lr_fault_export / lr_fault_import   data parallel (lipreading_amd/distributed.py): out2 = {status[0] (0 when
 *                      status is NULL), -(pending != 0)} for ONE MIN all-reduce over the ranks; import writes
 *                      in2[0] back to status[0] (skip the batch only if every rank skipped it) and raises the local
 *                      fault when in2[1] < 0 (ANY rank timed out: its garbage gradient is in the sum, so every rank
 *                      skips the update and the ranks stay identical). */
/* lr_rnn_one_launch_enable   PRODUCT switch: 0 = every recurrence (encoder layers and the decoder loop) takes the
 *                      per-step kernels from the next forward on, 1 (default) = the one-launch kernels where supported.
 *                      lipreading_amd.train switches it off — once, with a warning — after three consecutive steps
 *                      whose one-launch recurrence timed out (e.g. a device whose compute units are held by another
 *                      process): a slow run instead of one that skips every batch (the reference's contract is skip a
 *                      bad batch and keep training, src/train/train_better_model.py:49-50).  Size queries depend on it:
 *                      switch between steps.
 * lr_debug_busy        TEST HOOK: `workgroups` workgroups that each hold lds_bytes of LDS (up to a whole CU's 160 KB)
 *                      and spin for `microseconds` — a stand-in for a foreign kernel (an RCCL ring kernel on another
 *                      stream) that occupies compute units across the launch of a cluster recurrence. */
void lr_rnn_one_launch_enable(int on);
int lr_rnn_one_launch_enabled(void);
int lr_debug_busy(int workgroups, int lds_bytes, int microseconds, lr_stream_t stream);
int lr_rnn_pair_errors(void);
int lr_fault_export(const int32_t* status, int32_t* out2, lr_stream_t stream);
int lr_fault_import(const int32_t* in2, int32_t* status, lr_stream_t stream);
/* The same two facts as FLOATS that the gradient all-reduce itself can sum (round 5: no second collective): out2 = {1 if
 * status[0] != 0 else 0, 1 if a recurrence of this step timed out else 0}.  lipreading_amd.distributed writes them
 * into the two spare words at the front of the flat gradient buffer; lr_adam_step / lr_clip_adam_step take the summed
 * words as `dist_words` with the number of ranks: the batch is skipped if every rank skipped it (words[0] > world - 0.5),
 * nobody updates if any rank timed out (words[1] > 0.5). */
int lr_fault_export_f32(const int32_t* status, float* out2, lr_stream_t stream);
void* lr_fault_words_ptr(void);
int lr_step_begin(float* grad, int64_t n, float* also_zero, lr_stream_t stream);
/* lr_step_begin and lr_ctc_prepare_i64 (below) in ONE launch: the two first launches of a training step
 * (train_better_model.py:31-32 and :67) depend on nothing and not on each other. */
int lr_step_begin_ctc(float* grad, int64_t n, float* also_zero, const int64_t* chars, int64_t chars_stride,
                      const int64_t* frame_lens, const int64_t* char_lens, int32_t* labels_p1, int32_t* frame_lens32,
                      int32_t* label_lens32, int B, int L, lr_stream_t stream);
void lr_rnn_debug_drop_member(int member);
void lr_rnn_debug_disable_cluster(int off);   /* bit 0: no one-launch recurrence (the only bit read) */
/* TUNING HOOK of the one-launch recurrences' exchange polling: which = 0 forward / 1 backward cluster kernels; 2 .. 5 the
 * four gathers of the grid recurrence (LSTM past 1152 units): forward h, forward partial sums, backward partial dh,
 * backward dG; first_poll_delay = 64-clock sleeps between a member's publish and its first poll of the others (default 0),
 * round_sleep = sleeps between two poll rounds (default 1). */
void lr_rnn_debug_tune(int which, int first_poll_delay, int round_sleep);
size_t lr_rnn_reserve_bytes(int mode, int B, int T, int I, int H, int D);
size_t lr_rnn_workspace_bytes(int mode, int B, int T, int I, int H, int D);

int lr_rnn_layer_forward(int mode, const float* x, const int32_t* lens,
                         const float* const* w_ih_host, const float* const* w_hh_host,
                         const float* const* b_ih_host, const float* const* b_hh_host, float* y,
                         float* h_n, float* c_n, void* reserve, size_t reserve_bytes, int B,
                         int T, int I, int H, int D, lr_stream_t stream);

/* Backward of the layer above.
 *   dy [B,T,D*H]; dh_n, dc_n [D,B,H] (may be NULL = zero)
 *   dx [B,T,I] (may be NULL when the input needs no gradient: layer 0)
 *   dw_ih/dw_hh/db_ih/db_hh: HOST arrays of D device pointers; overwritten with the grads, or
 *   (accumulate != 0) added to — the reference step runs two backward passes over the same
 *   encoder graph and lets the gradients accumulate (train_better_model.py:69,74).
 *   workspace: lr_rnn_workspace_bytes.
 *   reserve: the forward's, at the SAME address (const for the caller's purposes: the gates are only read).  On the
 *   one-launch recurrence the forward's prologue launch also left the backward's W_hh fragments and cleared exchange
 *   words in it (round 5); the first backward over a forward's reserve uses them (and dirties the exchange words), a
 *   second one over the same forward re-packs with a launch of its own — the library keeps track by the address. */
int lr_rnn_layer_backward(int mode, const float* x, const int32_t* lens,
                          const float* const* w_ih_host, const float* const* w_hh_host,
                          const float* const* b_ih_host, const float* const* b_hh_host,
                          const float* y, const float* dy, const float* dh_n, const float* dc_n,
                          float* dx, float* const* dw_ih_host, float* const* dw_hh_host,
                          float* const* db_ih_host, float* const* db_hh_host,
                          const void* reserve, size_t reserve_bytes, void* workspace,
                          size_t workspace_bytes, int accumulate, int B, int T, int I, int H, int D,
                          lr_stream_t stream);

/* The same backward in two calls that may sit on two streams (build-defined, LR_RNN_PROJ_BF16X3
 * layers only; LR_ERR_UNSUPPORTED otherwise unless parts == 3):
 *   parts & 1: the recurrence and the data gradient dx (what the layer below waits for);
 *   parts & 2: the weight and bias gradients, from the gate gradients the parts & 1 call left in
 *              `workspace` — the caller orders it after that call (an event) and keeps the workspace
 *              alive; it can then overlap the layer below's latency-bound recurrence.
 * parts == 3 is lr_rnn_layer_backward. */
int lr_rnn_layer_backward_parts(int mode, const float* x, const int32_t* lens,
                                const float* const* w_ih_host, const float* const* w_hh_host,
                                const float* const* b_ih_host, const float* const* b_hh_host,
                                const float* y, const float* dy, const float* dh_n, const float* dc_n,
                                float* dx, float* const* dw_ih_host, float* const* dw_hh_host,
                                float* const* db_ih_host, float* const* db_hh_host,
                                const void* reserve, size_t reserve_bytes, void* workspace,
                                size_t workspace_bytes, int accumulate, int B, int T, int I, int H, int D,
                                int parts, lr_stream_t stream);

/* Instrumentation for the roofline leg of bench.py (the only entry points that touch the host
 * clock).  While enabled, every lr_rnn_layer_forward / _backward call issues ONE of its step
 * launches (the middle one) with a hipEvent pair that stamps that dispatch's begin and end on
 * the stream the kernel runs on.
 * The conv entry points do the same for every call.  lr_profile_read(which) WAITS for the recorded
 * events, returns the summed elapsed milliseconds and the number of samples in HOST memory, and
 * clears the ring (1024 samples per slot; later samples are dropped).  Slots: 0/1 recurrent
 * forward/backward step kernel; 2,3,4 conv1..3 forward; 5,6 conv2/conv3 data gradient; 7,8,9
 * conv1..3 weight gradient; 10 CTC alpha/beta kernel (lr_ctc_nll); 11 CTC gradient rows kernel
 * (lr_ctc_grad). */
int lr_profile_enable(int on);
int lr_profile_read(int which, float* total_ms_host, int* samples_host);

/* fp32 GEMM on the bf16 matrix cores by operand splitting (hi = bf16(x), lo = bf16(x - hi);
 * a_hi b_hi + a_hi b_lo + a_lo b_hi, fp32 accumulate): same conventions as lr_sgemm; a_exact /
 * b_exact declare an operand whose elements are bf16 values already (no lo term).  Build-defined
 * (no reference counterpart); ~1e-5 relative accuracy. */
size_t lr_xgemm_workspace_bytes(int transA, int transB, int M, int N, int K);
int lr_xgemm(int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
             const float* B, int ldb, float beta, float* C, int ldc, const float* bias, int a_exact,
             int b_exact, void* workspace, size_t workspace_bytes, lr_stream_t stream);

/* ---- A3 sessions (BUILD-DEFINED, no reference symbol): the uni-directional stack fed chunk by chunk ------------ */
/* An encoder session is one device buffer owned by the caller: for B independent slots the hidden state (LSTM: and
 * the cell state) of every layer of a stacked uni-directional GRU / LSTM / tanh RNN (lipreading_amd/csrc/
 * lr_rnn_stream.hip).  Fed the same frames in any chunks, in any slot of any batch, a session computes
 * the same bits.  mode is a plain cell (LR_RNN_GRU / LR_RNN_LSTM / LR_RNN_TANH): a flagged mode is rejected.
 * With G = 3 / 4 / 1 gates, HT = ceil(H / 16), Hp = 16 HT, a256(n) = n rounded up to a multiple of 256:
 *   pack      per layer l (I_l = I for l = 0, else H): a256(4 * HT * (ceil(I_l / 16) + HT) * G * 256) bytes of
 *             [W_ih | W_hh] fragments, then a256(4 * layers * 4 * Hp) bytes of biases (b_ih + b_hh per gate; the
 *             GRU's b_in and b_hn apart)
 *   state     a256(32 * B) bytes of slot headers (int32: magic, B, H, layers, cell, frames consumed — saturating —,
 *             status bits, 0), then h [layers][B][Hp] in a256(4 * layers * B * Hp) bytes, then (LSTM) c likewise
 *   workspace a256(4 * layers * max(chunk_T, 1) * B * Hp) bytes of per-frame planes, then (LSTM) a256(4 * layers * B * Hp)
 * Limits: layers <= 16, C <= 256, chunk_T <= 2^20, B <= 16 * 65535 (else 0 bytes / LR_ERR_UNSUPPORTED).  Buffers
 * smaller than their *_bytes answer LR_ERR_WORKSPACE, NULLs and negative sizes LR_ERR_INVALID_ARG, before any launch.
 * state, pack and workspace must be 16-byte aligned. */
#define LR_RNN_STREAM_MISMATCH 1 /* a call's B, H, layers or cell is not the slot's */

size_t lr_rnn_stream_pack_bytes(int mode, int I, int H, int layers);              /* 0 for arguments it rejects */
/* w_ih / w_hh / b_ih / b_hh: host arrays of `layers` device pointers, torch.nn layouts; any I >= 1, H >= 1, no
 * alignment asked of the tensors.  Made once per weight set. */
int lr_rnn_stream_pack(void* out, size_t out_bytes, int mode, const float* const* w_ih, const float* const* w_hh,
                       const float* const* b_ih, const float* const* b_hh, int I, int H, int layers,
                       lr_stream_t stream);
size_t lr_rnn_stream_state_bytes(int mode, int B, int H, int layers);             /* 0 for arguments it rejects */
size_t lr_rnn_stream_workspace_bytes(int mode, int B, int chunk_T, int I, int H, int layers,
                                     int C);                                      /* C = 0: no head; 0 if rejected */

/* Slots with mask[b] != 0 (mask [B] int32 on the device; NULL: all) go back to the zero state with 0 frames and no
 * status bit; the others keep every bit.  Under a mask the slot must already carry this configuration (else it is left
 * alone and gets LR_RNN_STREAM_MISMATCH); with NULL whatever the buffer held is overwritten. */
int lr_rnn_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int mode, int B, int H, int layers,
                        lr_stream_t stream);

/* Slot b consumes frames [0, clamp(sizes[b], 0, chunk_T)) of x[b] (x + b * stride_b + t * stride_t, I floats of unit
 * stride; sizes NULL = chunk_T): layers * chunk_T step launches, one head launch if head_w / head_b / head_mask are
 * given (all three or none; with them log_probs [B][chunk_T][C], without them log_probs NULL), one commit launch.
 * y [B][chunk_T][H] (may be NULL) is the last layer's output, zero at t >= sizes[b]; log_probs there is the head of the
 * zero row.  A slot with no frame keeps every bit of its state.  A slot whose header disagrees with B, H, layers or the
 * cell is left alone and gets LR_RNN_STREAM_MISMATCH, which stays until a reset.  chunk_T == 0 does nothing. */
int lr_rnn_stream_advance(int mode, const float* x, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                          const void* pack, size_t pack_bytes, const float* head_w, const float* head_b,
                          const float* head_mask, float* y, float* log_probs, void* state, size_t state_bytes,
                          void* workspace, size_t workspace_bytes, int B, int chunk_T, int I, int H, int layers, int C,
                          lr_stream_t stream);

/* h [layers][B][H], c likewise (NULL unless the state is an LSTM's), frames [B], status [B] (each may be NULL, not
 * all): what the slots hold, without changing a byte of the state.  A slot whose header is not (B, H, layers), or whose
 * cell does not go with c, reads as zeros with LR_RNN_STREAM_MISMATCH in status[b]. */
int lr_rnn_stream_read(const void* state, size_t state_bytes, float* h, float* c, int32_t* frames, int32_t* status,
                       int B, int H, int layers, lr_stream_t stream);

/* ---- A3 look-ahead sessions (BUILD-DEFINED, no reference symbol): the BIDIRECTIONAL stack fed chunk by chunk ----- */
/* A latency-controlled bidirectional GRU / LSTM / tanh RNN (lipreading_amd/csrc/lr_rnn_bistream.hip).
 * One advance hands slot b a window of window_T frames: it CONSUMES the first n_b = clamp(sizes[b], 0, chunk_T) and SEES
 * a_b = clamp(ahead[b], 0, window_T - n_b) more; e_b = n_b + a_b.  In every layer the forward direction starts from the
 * slot's carried state and runs over frames 0 .. e_b - 1, the state committed being the one after frame n_b - 1; the
 * backward direction starts from ZERO at frame e_b - 1, runs down to frame 0 and carries nothing to the next advance.
 * An upper layer's input is [fwd | bwd] of the same frame (torch's order).  Only consumed frames are returned.  With
 * ahead = all a slot has left at every advance, outputs and state are bit for bit the single advance over the whole
 * utterance, which is the one-shot bidirectional model.  mode is a plain cell; a flagged mode is rejected.
 * With G = 3 / 4 / 1 gates, HT = ceil(H / 16), Hp = 16 HT, a256(n) = n rounded up to a multiple of 256:
 *   pack      per layer l and direction (forward, then backward), with IC_l = ceil(I / 16) for l = 0 and 2 HT above
 *             (each direction's half padded on its own): a256(4 * HT * (IC_l + HT) * G * 256) bytes of [W_ih | W_hh]
 *             fragments, then a256(4 * layers * 2 * 4 * Hp) bytes of biases (b_ih + b_hh per gate; the GRU's b_in and
 *             b_hn apart)
 *   state     a256(32 * B) bytes of slot headers (int32: magic — not the causal session's —, B, H, layers, cell, frames
 *             consumed — saturating —, status bits, 0), then the FORWARD h [layers][B][Hp] in
 *             a256(4 * layers * B * Hp) bytes, then (LSTM) the forward c likewise
 *   workspace a256(4 * layers * 2 * max(window_T, 1) * B * Hp) bytes of per-frame planes, then (LSTM)
 *             a256(4 * layers * 2 * B * Hp) + a256(4 * layers * B * Hp)
 * Limits: layers <= 16, C <= 256, chunk_T <= window_T <= 2^20, B <= 16 * 65535 (else 0 bytes / LR_ERR_UNSUPPORTED).
 * Buffers smaller than their *_bytes answer LR_ERR_WORKSPACE, NULLs, negative sizes and window_T < chunk_T
 * LR_ERR_INVALID_ARG, before any launch.  state, pack and workspace must be 16-byte aligned.  A causal session's state
 * (lr_rnn_stream_*) handed to these entry points gets LR_RNN_STREAM_MISMATCH and keeps its bytes, and the other way
 * round. */
size_t lr_rnn_bistream_pack_bytes(int mode, int I, int H, int layers);            /* 0 for arguments it rejects */
/* w_ih / w_hh / b_ih / b_hh: host arrays of 2 * layers device pointers, [2 l] the forward (`*_l{l}`) and [2 l + 1] the
 * backward (`*_l{l}_reverse`) direction, torch.nn layouts (W_ih of an upper layer [G H][2 H]); any I >= 1, H >= 1, no
 * alignment asked of the tensors.  Made once per weight set. */
int lr_rnn_bistream_pack(void* out, size_t out_bytes, int mode, const float* const* w_ih, const float* const* w_hh,
                         const float* const* b_ih, const float* const* b_hh, int I, int H, int layers,
                         lr_stream_t stream);
size_t lr_rnn_bistream_state_bytes(int mode, int B, int H, int layers);           /* 0 for arguments it rejects */
size_t lr_rnn_bistream_workspace_bytes(int mode, int B, int chunk_T, int window_T, int I, int H, int layers,
                                       int C);                                    /* C = 0: no head; 0 if rejected */

/* As lr_rnn_stream_reset, on a look-ahead session's state. */
int lr_rnn_bistream_reset(void* state, size_t state_bytes, const int32_t* mask, int mode, int B, int H, int layers,
                          lr_stream_t stream);

/* One advance (above).  x[b] frame t at x + b * stride_b + t * stride_t, I floats of unit stride, readable for
 * t < e_b; sizes NULL = chunk_T, ahead NULL = 0 (both [B] int32 on the device).  layers * window_T step launches (both
 * directions in each), one head launch if head_w [C][2 H] / head_b / head_mask are given (all three or none; with them
 * log_probs [B][chunk_T][C], without them log_probs NULL), one commit launch.  y [B][chunk_T][2 H] (may be NULL) is the
 * last layer's [fwd | bwd], zero at t >= n_b; log_probs there is the head of the zero row.  A slot with n_b == 0 keeps
 * every bit of its state and its frame count, whatever ahead[b] is.  A slot whose header disagrees with B, H, layers or
 * the cell is left alone and gets LR_RNN_STREAM_MISMATCH, which stays until a reset.  chunk_T == 0 does nothing. */
int lr_rnn_bistream_advance(int mode, const float* x, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                            const int32_t* ahead, const void* pack, size_t pack_bytes, const float* head_w,
                            const float* head_b, const float* head_mask, float* y, float* log_probs, void* state,
                            size_t state_bytes, void* workspace, size_t workspace_bytes, int B, int chunk_T,
                            int window_T, int I, int H, int layers, int C, lr_stream_t stream);

/* As lr_rnn_stream_read: h / c [layers][B][H] are the FORWARD direction's (the backward direction carries no state). */
int lr_rnn_bistream_read(const void* state, size_t state_bytes, float* h, float* c, int32_t* frames, int32_t* status,
                         int B, int H, int layers, lr_stream_t stream);

/* ---- A3 tail: output_proj + masked_log_softmax — better_model.py:92-93 ------------------ */

/* log_probs[r,:] = log_softmax(hidden[r,:] @ W^T + bias + log(mask + 1e-45))
 *   hidden [R,K] (R = B*T rows, padded rows included exactly as the reference does),
 *   W [C,K], bias [C], mask [C] (0/1 floats; masked classes end ~103.28 below, finite),
 *   log_probs [R,C].  C <= 256.  workspace: lr_proj_workspace_bytes(R,K,C). */
size_t lr_proj_workspace_bytes(int R, int K, int C);
int lr_proj_logsoftmax_forward(const float* hidden, const float* W, const float* bias,
                               const float* mask, float* log_probs, void* workspace,
                               size_t workspace_bytes, int R, int K, int C, lr_stream_t stream);

/* dlogits[r,c] = g[r,c] - exp(log_probs[r,c]) * sum_c g[r,c]; then
 * dhidden = dlogits @ W, dW = dlogits^T @ hidden, dbias = colsum(dlogits).
 *   dlogits [R,C] is caller scratch (also an output).  dhidden may be NULL.
 *   accumulate != 0: dW and dbias are added to instead of overwritten. */
int lr_proj_logsoftmax_backward(const float* g, const float* log_probs, const float* hidden,
                                const float* W, float* dlogits, float* dhidden, float* dW,
                                float* dbias, void* workspace, size_t workspace_bytes, int accumulate,
                                int R, int K, int C, lr_stream_t stream);

/* ---- N1: attention character decoder — better_model.py:124-235, train_better_model.py:54-65 - */

typedef enum lr_attention_type {
  LR_ATT_NONE = 0,    /* output_proj(rnn state)                                   (:228)      */
  LR_ATT_DOT = 1,     /* logit[t] = h . enc[t]                                     (:206-208)  */
  LR_ATT_GENERAL = 2, /* logit[t] = (W_g h + b_g) . enc[t]                         (:191-205)  */
  LR_ATT_1LNN = 3,    /* logit[t] = w . [enc[t]; h] + b                            (:185-190)  */
  LR_ATT_CONCAT = 4   /* logit[t] = w2 . tanh(W1 [enc[t]; h] + b1) + b2            (:209-215)  */
} lr_attention_type;

/* Device pointers to the parameters of CharDecodingStep (torch layouts, fp32). */
typedef struct lr_decoder_params {
  const float* emb;     /* embedding.weight      [V][Cd]                                        */
  const float* w_ih;    /* rnn.weight_ih_l0      [G*Hd][Cd]                                     */
  const float* w_hh;    /* rnn.weight_hh_l0      [G*Hd][Hd]                                     */
  const float* b_ih;    /* rnn.bias_ih_l0        [G*Hd]                                         */
  const float* b_hh;    /* rnn.bias_hh_l0        [G*Hd]                                         */
  const float* attn_w1; /* general: W_g [Hd][Hd]; 1_layer_nn: w [1][2Hd]; concat: W1 [A][2Hd]   */
  const float* attn_b1; /* general: b_g [Hd];     1_layer_nn: b [1];      concat: b1 [A]        */
  const float* attn_w2; /* concat: attn_proj_layer2.weight [1][A]                               */
  const float* attn_b2; /* concat: attn_proj_layer2.bias   [1]                                  */
  const float* w_c;     /* concat_layer.weight   [Hd][2Hd]   (unused for LR_ATT_NONE)           */
  const float* b_c;     /* concat_layer.bias     [Hd]                                           */
  const float* w_o;     /* output_proj.weight    [V][Hd]                                        */
  const float* b_o;     /* output_proj.bias      [V]                                            */
  const float* out_mask;/* [V] 0/1 floats: PAD and BOS masked (better_model.py:142-144)         */
} lr_decoder_params;

/* Gradients, same layouts; overwritten, or added to when `accumulate` != 0. */
typedef struct lr_decoder_grads {
  float* emb; float* w_ih; float* w_hh; float* b_ih; float* b_hh;
  float* attn_w1; float* attn_b1; float* attn_w2; float* attn_b2;
  float* w_c; float* b_c; float* w_o; float* b_o;
  int emb_padding_idx;  /* nn.Embedding(padding_idx): that row receives no gradient; -1 = none    */
} lr_decoder_grads;

/* Layers 1 .. num_layers-1 of the decoder's RNN stack (better_model.py:136,147-148: the decoder takes
 * the encoder's num_layers; nn.GRU/LSTM/RNN(char_dim, Hd, num_layers) semantics: layer k's input is
 * layer k-1's output of the same step).  Entry k-1 holds layer k: rnn.weight_ih_l{k} [G*Hd][Hd],
 * rnn.weight_hh_l{k} [G*Hd][Hd], rnn.bias_ih_l{k}, rnn.bias_hh_l{k} [G*Hd].  drop_mask (NULL = none):
 * [num_layers-1][B][L][Hd] multipliers (0 or 1/(1-p)) applied to the outputs of every layer but the
 * last — the inter-layer dropout of nn.GRU(dropout=p) in training mode, drawn by the caller.
 * Passing NULL for the struct = a single-layer decoder (every shipped config). */
#define LR_DEC_MAX_LAYERS 8
typedef struct lr_decoder_upper {
  int num_layers;
  const float* w_ih[LR_DEC_MAX_LAYERS - 1];
  const float* w_hh[LR_DEC_MAX_LAYERS - 1];
  const float* b_ih[LR_DEC_MAX_LAYERS - 1];
  const float* b_hh[LR_DEC_MAX_LAYERS - 1];
  const float* drop_mask;
} lr_decoder_upper;
typedef struct lr_decoder_upper_grads {
  float* w_ih[LR_DEC_MAX_LAYERS - 1];
  float* w_hh[LR_DEC_MAX_LAYERS - 1];
  float* b_ih[LR_DEC_MAX_LAYERS - 1];
  float* b_hh[LR_DEC_MAX_LAYERS - 1];
} lr_decoder_upper_grads;

/* The whole decoder loop of one batch (max_label_len = L steps): an RNN stack (mode = LR_RNN_GRU /
 * LR_RNN_LSTM / LR_RNN_TANH, num_layers layers) of hidden size Hd started from the encoder's final
 * state (h0 [num_layers][B][Hd], c0 likewise for the LSTM); the attention and the output head read the
 * top layer's state.
 *   tokens [B][L] int32    teacher inputs chars[:, i] (device)
 *   teacher_forced_host[L] HOST bytes: 1 = step i is fed tokens[:, i], 0 = fed the previous step's
 *                          multinomial sample (train_better_model.py:57-58; step 0 always uses tokens)
 *   enc [B][T][Hd], enc_lens [B] int32; step_lens [B] int32, every entry = L
 *   log_probs [B][L][V]    masked log-softmax outputs of every step (better_model.py:229)
 *   sampled [B][L] int32   multinomial(exp(log_probs)) of every step (counter-based RNG on `seed`;
 *                          equal to torch's sampler in distribution only)
 * The caller derives the loss (nll_loss, ignore_index = PAD, train_better_model.py:62) and the
 * accuracy counts (:131-133) from log_probs / sampled.  h_n / c_n [num_layers][B][Hd] (may be NULL)
 * receive the RNN state after the last step (the final_state a single reference step returns).   */
size_t lr_decoder_reserve_bytes(int mode, int attn_type, int num_layers, int B, int L, int T, int Hd, int Cd,
                                int V, int A);
size_t lr_decoder_workspace_bytes(int mode, int attn_type, int num_layers, int B, int L, int T, int Hd, int Cd,
                                  int V, int A);
int lr_decoder_forward(int mode, int attn_type, const lr_decoder_params* params_host,
                       const lr_decoder_upper* upper_host, const int32_t* tokens,
                       const uint8_t* teacher_forced_host, const float* enc, const int32_t* enc_lens,
                       const float* h0, const float* c0, const int32_t* step_lens, uint64_t seed,
                       float* log_probs, int32_t* sampled, float* h_n, float* c_n, void* reserve,
                       size_t reserve_bytes, int B, int L, int T, int Hd, int Cd, int V, int A,
                       lr_stream_t stream);
/* Backward of the loop: d_log_probs [B][L][V] (+ dh_n / dc_n [num_layers][B][Hd], gradient arriving
 * through the returned final state; may be NULL) -> d_enc [B][T][Hd] (overwritten), dh0 / dc0
 * [num_layers][B][Hd] (gradient into the encoder's final state) and every parameter gradient
 * (upper_grads_host may be NULL for a single layer).                                                 */
int lr_decoder_backward(int mode, int attn_type, const lr_decoder_params* params_host,
                        const lr_decoder_upper* upper_host, const lr_decoder_grads* grads_host,
                        const lr_decoder_upper_grads* upper_grads_host, const float* enc, const int32_t* enc_lens,
                        const float* h0, const float* c0, const int32_t* step_lens, const float* log_probs,
                        const float* d_log_probs, const float* dh_n, const float* dc_n, float* d_enc,
                        float* dh0, float* dc0, const void* reserve, size_t reserve_bytes, void* workspace,
                        size_t workspace_bytes, int accumulate, int B, int L, int T, int Hd, int Cd, int V,
                        int A, lr_stream_t stream);
/* ... in two halves (as lr_rnn_layer_backward_parts): parts 1 = the data half — d_enc, dh0, dc0: what the encoder's
 * backward waits for —, 2 = every parameter gradient from what part 1 left in `workspace` (same arguments, any stream
 * that waits for part 1; the workspace must live until it has run), 3 = both.  Separable for a single-layer loop
 * (lr_decoder_backward_splittable: every flag file the reference ships); otherwise only parts = 3 is accepted. */
int lr_decoder_backward_splittable(int attn_type, int num_layers);
int lr_decoder_backward_parts(int mode, int attn_type, const lr_decoder_params* params_host,
                              const lr_decoder_upper* upper_host, const lr_decoder_grads* grads_host,
                              const lr_decoder_upper_grads* upper_grads_host, const float* enc, const int32_t* enc_lens,
                              const float* h0, const float* c0, const int32_t* step_lens, const float* log_probs,
                              const float* d_log_probs, const float* dh_n, const float* dc_n, float* d_enc,
                              float* dh0, float* dc0, const void* reserve, size_t reserve_bytes, void* workspace,
                              size_t workspace_bytes, int accumulate, int B, int L, int T, int Hd, int Cd, int V,
                              int A, int parts, lr_stream_t stream);

/* ---- A5b: beam search through the attention decoder — src/models/lipreader/analysis.py:12-66 (inference) ---- */
/* Deterministic, batched, entirely on the device; the search rule and its two departures from the reference
 * (top-K candidates instead of multinomial draws; PAD and BOS never candidates) are stated in
 * lipreading_amd/csrc/lr_attn_beam.hip.  Same params / upper (drop_mask must be NULL), enc
 * [B][T][Hd], enc_lens [B] int32 and h0 / c0 [num_layers][B][Hd] as lr_decoder_forward.
 *   bos / eos / pad      the vocabulary's marker ids; beam_width = K, max_label_len = Lmax
 *   poll_every           the host reads the 4-byte finished counter every poll_every rounds to stop launching
 *                        (the results do not depend on it)
 *   out_ids [B][K][Lmax+1] int32 (pad past each length), out_lens [B][K] int32, out_scores [B][K] fp32: the
 *                        final beam, best first (empty slots: length 0, score -inf)
 *   rounds_host          HOST int (may be NULL): rounds the search needed (the call then synchronises the stream)
 * Limits: K <= 32, Lmax <= 65535, 3 <= V <= 1024, B*K <= 65535 (else LR_ERR_UNSUPPORTED; the workspace query
 * returns 0 for every request the search rejects). */
size_t lr_decoder_beam_workspace_bytes(int mode, int attn_type, int num_layers, int B, int K, int Lmax, int T, int Hd,
                                       int Cd, int V, int A);
int lr_decoder_beam_search(int mode, int attn_type, const lr_decoder_params* params_host,
                           const lr_decoder_upper* upper_host, const float* enc, const int32_t* enc_lens,
                           const float* h0, const float* c0, int bos, int eos, int pad, int beam_width,
                           int max_label_len, int poll_every, int32_t* out_ids, int32_t* out_lens, float* out_scores,
                           int32_t* rounds_host, void* workspace, size_t workspace_bytes, int B, int T, int Hd, int Cd,
                           int V, int A, lr_stream_t stream);

/* Joint CTC/attention beam search (Watanabe et al. 2017): the search above, each hypothesis scored
 * (1 - ctc_weight) * (attention log-prob) + ctc_weight * (CTC prefix log-prob), the CTC term computed on the device
 * in float64 from the encoder's CTC head.  Rule, structure and costs: lipreading_amd/csrc/lr_attn_beam.hip
 * (DESIGN.md §15).  Arguments as lr_decoder_beam_search, plus
 *   ctc_lp               fp32 CTC log-probs, element (b, t, c) at ctc_lp[b*stride_b + t*stride_t + c] (strides in
 *                        elements; the class dimension contiguous), C = V + 1 classes, class v + 1 = token v
 *   blank                must be 0
 *   ctc_weight           lambda in [0, 1]; at 0 the result is lr_decoder_beam_search's
 *   pre_beam             P, the candidates per hypothesis: min(K, V - 2) <= P <= min(64, V - 2)
 * out_scores are the joint scores.  Precondition: 1 <= enc_lens[b] <= T (as the attention needs; the CTC terms clamp
 * it to stay in bounds).  Limits: those above and T <= 65535 (else LR_ERR_UNSUPPORTED); C != V + 1, blank != 0 or a
 * weight outside [0, 1] (NaN included) is LR_ERR_INVALID_ARG.  The workspace query takes the search's sizes plus C
 * and P (its size does not depend on the weight) and returns 0 for every request the search rejects. */
size_t lr_decoder_joint_beam_workspace_bytes(int mode, int attn_type, int num_layers, int B, int K, int Lmax, int T,
                                             int Hd, int Cd, int V, int A, int C, int pre_beam);
int lr_decoder_joint_beam_search(int mode, int attn_type, const lr_decoder_params* params_host,
                                 const lr_decoder_upper* upper_host, const float* enc, const int32_t* enc_lens,
                                 const float* h0, const float* c0, const float* ctc_lp, int64_t stride_b,
                                 int64_t stride_t, int C, int blank, double ctc_weight, int pre_beam, int bos, int eos,
                                 int pad, int beam_width, int max_label_len, int poll_every, int32_t* out_ids,
                                 int32_t* out_lens, float* out_scores, int32_t* rounds_host, void* workspace,
                                 size_t workspace_bytes, int B, int T, int Hd, int Cd, int V, int A,
                                 lr_stream_t stream);

/* Word language model fusion: the joint search above with the ARPA word model of lr_ctc_beam_lm_decode, each
 * hypothesis scored (1 - ctc_weight) * attention + ctc_weight * CTC + the sum of alpha * lm(word | context) + beta
 * over its completed words, and kept inside the model's vocabulary letter by letter.  Rule and structure:
 * lipreading_amd/csrc/lr_attn_beam.hip.  Arguments as lr_decoder_joint_beam_search, plus
 *   lm                   the blob lr_ctc_beam_lm_pack wrote, on the device, packed for the C = V + 1 CTC classes (class
 *                        v + 1 = token v): one blob serves lr_ctc_beam_lm_decode and this search
 *   class_roles          [C] int32 on the device (0 transparent, 1 word character, 2 space)
 *   alpha, beta          the model's weight and the per-word bonus, as in lr_ctc_beam_lm_decode
 *   ctc_lp               may be NULL exactly when ctc_weight == 0 (no CTC term is computed: attention + model)
 * At ctc_weight = 0 the result is NOT lr_decoder_beam_search's: the model's terms reorder candidates, so pre_beam
 * matters there too.  Limits: those of the joint search and V + 1 <= 256 (else LR_ERR_UNSUPPORTED, workspace query 0);
 * non-finite alpha or beta, or a NULL lm or class_roles, is LR_ERR_INVALID_ARG. */
size_t lr_decoder_lm_beam_workspace_bytes(int mode, int attn_type, int num_layers, int B, int K, int Lmax, int T,
                                          int Hd, int Cd, int V, int A, int C, int pre_beam);
int lr_decoder_lm_beam_search(int mode, int attn_type, const lr_decoder_params* params_host,
                              const lr_decoder_upper* upper_host, const float* enc, const int32_t* enc_lens,
                              const float* h0, const float* c0, const float* ctc_lp, int64_t stride_b,
                              int64_t stride_t, int C, int blank, double ctc_weight, int pre_beam, const void* lm,
                              const int32_t* class_roles, float alpha, float beta, int bos, int eos, int pad,
                              int beam_width, int max_label_len, int poll_every, int32_t* out_ids, int32_t* out_lens,
                              float* out_scores, int32_t* rounds_host, void* workspace, size_t workspace_bytes, int B,
                              int T, int Hd, int Cd, int V, int A, lr_stream_t stream);

/* Attention rescoring of CTC N-best lists, the second pass of two-pass decoding: each of an utterance's N first-pass
 * hypotheses is scored once by the attention decoder, teacher-forced, and the list is reordered by
 * s = (1 - ctc_weight) * a - ctc_weight * f + length_bonus * |q|.  Rule and structure:
 * lipreading_amd/csrc/lr_attn_rescore.hip.  params / upper (drop_mask must be NULL), enc, enc_lens,
 * h0 / c0 as lr_decoder_beam_search, plus
 *   hyp_ids              int32 CTC classes (class v + 1 = token v), hypothesis (b, n)'s i-th class at
 *                        hyp_ids[b*hyp_stride_b + n*hyp_stride_n + i] (strides in elements, >= 0): the (B, beam, T)
 *                        tensor of lr_ctc_beam_decode, or a [:, :N, :W] view of it, goes in as it is
 *   hyp_lens [B][N]      int32 classes per hypothesis (clamped to [0, W]); ids past it are never read
 *   first_scores [B][N]  fp32 -log P of the first pass; a slot with length 0 and +inf, or with NaN, is empty
 *   ctc_weight           lambda in [0, 1]; length_bonus: any finite value
 *   out_order [B][N] int32, out_scores [B][N] fp32, out_attn [B][N] fp32: ranked best first, the input slot at each
 *                        rank, its s and its a; both -inf for slots that cannot be scored (a token that is PAD, BOS,
 *                        blank or outside [0, V)), which follow the scored ones in first-pass order, and for empty
 *                        slots, which come last
 * No host synchronisation.  Limits: 1 <= N <= 128, 1 <= W <= 1024, 3 <= V <= 1024, B*N <= 65535,
 * B*N*(W+1) <= 65535*64, B*N*(W+1)*max(G*Hd, T, V, A) < 2^31 and B*T*max(G*Hd, T, V, A) < 2^31 (G gates: 3 GRU, 4 LSTM,
 * 1 tanh), Hd % 4 == 0, the scoring head's LDS (Hd + V) * 4 <= 60 KB, with concat attention A > 0 and 2*A*4 <= 60 KB;
 * every RNN mode, every attention type, 1 .. LR_DEC_MAX_LAYERS layers (else LR_ERR_UNSUPPORTED; the workspace query
 * returns 0 for every request the call rejects by its sizes); a weight outside [0, 1], a non-finite weight or bonus, a
 * NULL required pointer, a negative id stride or a drop_mask is LR_ERR_INVALID_ARG. */
size_t lr_decoder_rescore_workspace_bytes(int mode, int attn_type, int num_layers, int B, int N, int W, int T, int Hd,
                                          int Cd, int V, int A);
int lr_decoder_rescore(int mode, int attn_type, const lr_decoder_params* params_host,
                       const lr_decoder_upper* upper_host, const float* enc, const int32_t* enc_lens, const float* h0,
                       const float* c0, const int32_t* hyp_ids, int64_t hyp_stride_b, int64_t hyp_stride_n,
                       const int32_t* hyp_lens, const float* first_scores, int bos, int eos, int pad,
                       double ctc_weight, double length_bonus, int32_t* out_order, float* out_scores, float* out_attn,
                       void* workspace, size_t workspace_bytes, int B, int N, int W, int T, int Hd, int Cd, int V,
                       int A, lr_stream_t stream);

/* The decoder loss of the train loop (train_better_model.py:62,65): over the R = B*L (sample, step) rows,
 * -sum_r log_probs[r][label_r] for label_r != ignore_index (F.nll_loss(ignore_index=PAD, reduction='sum') summed
 * over the steps) divided by the number of such rows ((labels != PAD).sum()).  labels: int64, row (b, i) at
 * labels[b * label_stride + i] (a view of chars[:, 1:]).  out2[0] = loss, out2[1] = count (kept for the backward).
 * Backward: d_log_probs [R][V] (every element written) from the upstream scalar gradient on the device. */
int lr_nll_mean_forward(const float* log_probs, const int64_t* labels, int64_t label_stride, int L, int ignore_index,
                        float* out2, int R, int V, lr_stream_t stream);
/* ... the same with out3 = {loss, count, the un-divided sum}: eval keeps sum and count apart
 * (train_better_model.py:127,138: nll sums added over the batches, divided by the total count at the end). */
int lr_nll_forward3(const float* log_probs, const int64_t* labels, int64_t label_stride, int L, int ignore_index,
                    float* out3, int R, int V, lr_stream_t stream);
int lr_nll_mean_backward(const int64_t* labels, int64_t label_stride, int L, int ignore_index, const float* fwd_out2,
                         const float* grad_out, float* d_log_probs, int R, int V, lr_stream_t stream);

/* ---- A10 (build-defined): transformer encoder blocks — no reference symbol ------ *
 * torch.nn.TransformerEncoderLayer(norm_first=False, activation=relu, dropout=0) arithmetic; the
 * host composition is lipreading_amd/transformer.py -> lr_tfm_* below; the pieces are entry points of their own. */

/* batch_outer x batch_inner independent fp32 products C_z = alpha op(A_z) op(B_z) + beta C_z, problem
 * z = (o, i) at element offsets o*s?_outer + i*s?_inner from the base pointers (0: shared operand).
 * Per (sample, head) attention products read Q/K/V straight out of the fused [R][3D] projection. */
int lr_sgemm_batched(int transA, int transB, int M, int N, int K, float alpha, const float* A, int lda,
                     int64_t sA_outer, int64_t sA_inner, const float* B, int ldb, int64_t sB_outer,
                     int64_t sB_inner, float beta, float* C, int ldc, int64_t sC_outer, int64_t sC_inner,
                     int batch_outer, int batch_inner, lr_stream_t stream);
/* y = LayerNorm(x + residual) * gamma + beta over rows of D (residual may be NULL); stats [R][2] =
 * (mean, rstd) for the backward.  Backward: dx is the gradient of BOTH x and residual; dgamma / dbeta
 * overwritten or (accumulate != 0) added to.  The forward takes any D; the backward keeps 4 x 2 x D floats in LDS
 * and returns LR_ERR_UNSUPPORTED past D = 1920 (nothing is written then). */
int lr_layernorm_forward(const float* x, const float* residual, const float* gamma, const float* beta,
                         float* y, float* stats, int R, int D, float eps, lr_stream_t stream);
size_t lr_layernorm_workspace_bytes(int D);
int lr_layernorm_backward(const float* x, const float* residual, const float* gamma, const float* stats,
                          const float* dy, float* dx, float* dgamma, float* dbeta, void* workspace,
                          size_t workspace_bytes, int accumulate, int R, int D, lr_stream_t stream);
/* In place: scores [B][Hh][T][T] -> softmax over keys of scale*scores with keys >= key_lens[b] masked
 * (probability 0).  key_lens[b] is clamped to [1, T]: a sample of length 0 attends to key 0 alone (every output stays
 * finite; torch gives NaN there), the same rule as lr_attn_fused_*.  Backward, in place over dprobs:
 * dscores = scale * P * (dP - sum_k dP P). */
int lr_attn_softmax_forward(float* scores, const int32_t* key_lens, float scale, int B, int Hh, int T,
                            lr_stream_t stream);
int lr_attn_softmax_backward(const float* probs, float* dprobs, float scale, int B, int Hh, int T,
                             lr_stream_t stream);
/* Chunk-limited attention (BUILD-DEFINED): the same softmax under the chunk mask a streaming model is
 * trained with.  chunk = C >= 1, left_chunks = Lc >= 0: query q of a sample of len = clamp(key_lens[b], 1, T) frames
 * sits in chunk c = q / C and attends to key k iff  max(0, c - Lc) * C <= k < min(len, (c + 1) * C)  — its own chunk to
 * the end and Lc whole chunks before it; the look-ahead is at most C - 1 frames whatever the depth of the stack.  A
 * query with no key (only a padded one, q >= len) gets probability 0 everywhere and a zero context row: finite on every
 * path.  chunk = 0 is lr_attn_softmax_forward (the same bits).  Masked keys have probability exactly 0, so
 * lr_attn_softmax_backward serves both.  Negative chunk / left_chunks: LR_ERR_INVALID_ARG before any launch.  The
 * lr_attn_fused_*_chunked and lr_tfm_*_chunked entry points below take the same two integers the same way. */
int lr_attn_softmax_forward_chunked(float* scores, const int32_t* key_lens, float scale, int B, int Hh, int T, int chunk,
                                    int left_chunks, lr_stream_t stream);
/* Fused self-attention core on the bf16 matrix cores (lr_attention.hip): per (sample, head)
 * out = softmax_keys(scale * Q K^T, keys >= key_lens[b] masked) V, with Q / K / V read in place from the fused
 * projection qkv [B][T][3*nhead*dh] (head h at columns h*dh of each third), out [B][T][nhead*dh]; backward:
 * dout -> dqkv (same layout as qkv; every element written).  One workgroup per (sample, head), T <= 96, dh in
 * {32, 64} (lr_attn_fused_supported); the T x T probabilities never leave the chip (the backward recomputes
 * them).  bf16 operands, fp32 accumulation and softmax.  key_lens[b] is clamped to [1, T] as in
 * lr_attn_softmax_forward: a sample of length 0 attends to key 0 alone. */
int lr_attn_fused_supported(int T, int dh);
int lr_attn_fused_forward(const float* qkv, const int32_t* key_lens, float* out, float scale, int B, int T,
                          int nhead, int dh, lr_stream_t stream);
int lr_attn_fused_backward(const float* qkv, const int32_t* key_lens, const float* dout, float* dqkv, float scale,
                           int B, int T, int nhead, int dh, lr_stream_t stream);
/* the fused core under the chunk mask of lr_attn_softmax_forward_chunked (the backward recomputes the probabilities, so
 * it takes the same chunk / left_chunks as the forward it differentiates); chunk = 0: the two above */
int lr_attn_fused_forward_chunked(const float* qkv, const int32_t* key_lens, float* out, float scale, int B, int T,
                                  int nhead, int dh, int chunk, int left_chunks, lr_stream_t stream);
int lr_attn_fused_backward_chunked(const float* qkv, const int32_t* key_lens, const float* dout, float* dqkv, float scale,
                                   int B, int T, int nhead, int dh, int chunk, int left_chunks, lr_stream_t stream);
/* Products straight from the tensors as they lie in memory (lr_fgemm.hip; BUILD-DEFINED, no reference symbol):
 *   C[M][N] = epilogue(sum_k op(A)[m][k] op(B)[k][n]),  form NT: A [M][K], B [N][K];  NN: A [M][K], B [K][N];
 *   TN: A [K][M], B [K][N].  prec LR_FGEMM_X3: fp32 operands split into bf16 hi + lo on the way into LDS, three
 *   products on the bf16 matrix cores (~1e-5 relative); LR_FGEMM_F32: exact fp32 matrix-core products.  a_bf16 (NT
 *   only) / b_bf16 (TN only): that operand is stored as bf16.  Epilogue per job: out = alpha * acc + bias[n] +
 *   addend[(m % add_period) * ldadd + n]; LR_FGEMM_RELU; mask (out = mask[m * ldmask + n] > 0 ? out : 0); + beta * C;
 *   LR_FGEMM_C_BF16: C is a bf16 matrix (beta must be 0).  colsum (TN only): colsum[m] = beta * colsum[m] + sum_k A[k][m] — the
 *   bias gradient of a weight-gradient product.  splits > 1: K is cut into that many ranges whose partial sums (and
 *   partial column sums) go through `slabs` (lr_fgemm_slab_floats(M, N, splits) floats) and one combine launch for all
 *   the launch's split jobs (lr_fgemm_splits suggests a count).  Up to 20 jobs of one form share a launch.  Only enqueues. */
#define LR_FGEMM_X3 0
#define LR_FGEMM_F32 1
#define LR_FGEMM_NT 0
#define LR_FGEMM_NN 1
#define LR_FGEMM_TN 2
#define LR_FGEMM_RELU 1
#define LR_FGEMM_C_BF16 2
typedef struct {
  const void* A;
  const void* B;
  void* C;
  const float* bias;
  const float* addend;
  const float* mask;
  float* colsum;
  float* slabs;
  int32_t M, N, K, lda, ldb, ldc, ldadd, add_period, ldmask, flags, splits;
  float alpha, beta;
  int32_t b_shift, b_period;   /* NN / TN, fp32 B: row k of B is read from row k + b_shift, as zeros where (k % b_period) +
                                  b_shift leaves [0, b_period) — the previous / next time step of a [B*T][N] sequence tensor
                                  (a recurrent layer's dW_hh = dG^T . h_prev straight from y); b_period 0: off */
} lr_fgemm_job;
int lr_fgemm(int prec, int form, int a_bf16, int b_bf16, const lr_fgemm_job* jobs, int njobs, lr_stream_t stream);
int lr_fgemm_splits(int M, int N, int K);
long long lr_fgemm_slab_floats(int M, int N, int splits);

/* The whole encoder stack of lipreading_amd/transformer.py as three enqueues (lr_transformer.hip):
 *   h0 = x W_p^T + b_p + pe[t];  per layer (post-LN, ReLU feed-forward, dropout 0 — torch.nn.TransformerEncoderLayer):
 *   qkv = h W_qkv^T + b;  a = attention(qkv, key_lens);  h1 = LN1(a W_o^T + b_o + h);
 *   h2 = LN2(relu(h1 W_1^T + b_1) W_2^T + b_2 + h1).
 * mode: LR_TFM_X3 (projections as split-bf16 products, else exact fp32) | LR_TFM_X_BF16 (x is stored as bf16) |
 *   LR_TFM_DX_BF16 (dx is written as bf16) | LR_TFM_ATTN_FUSED (lr_attn_fused_*; else fp32 batched products + softmax) |
 *   LR_TFM_ROWBLOCK (below).
 * weights: 2 + 12 * nlayers device pointers in torch's registration order: input_proj.weight [Dm][I], .bias, then per
 *   layer in_proj_weight [3Dm][Dm], in_proj_bias, out_proj.weight [Dm][Dm], .bias, linear1.weight [F][Dm], .bias,
 *   linear2.weight [Dm][F], .bias, norm1.weight, .bias, norm2.weight, .bias.  pe: [>= T][Dm].
 * forward: x [B*T][I] -> h_out [B*T][Dm]; `reserve` (lr_tfm_reserve_bytes) keeps what the backward reads.
 * backward_data: dh_out -> dx (NULL: not wanted) and every layer's pre-activation gradients, kept in `workspace`
 *   (lr_tfm_workspace_bytes); backward_weights (any stream that waits for backward_data) turns them into the 2 + 12 *
 *   nlayers gradients: every weight gradient of the stack with its bias gradient in ONE launch (two when x is bf16),
 *   the LayerNorm parameter gradients in one more; accumulate != 0 adds to `grads`. */
#define LR_TFM_X3 1
#define LR_TFM_X_BF16 2
#define LR_TFM_DX_BF16 4
#define LR_TFM_ATTN_FUSED 8
#define LR_TFM_ROWBLOCK 16   /* out-projection .. LN2 (and their backward) as ONE launch per layer and direction over 32-row
                                blocks (lr_tfm_rowblock.hip); needs LR_TFM_X3 and lr_tfm_rowblock_supported(): d_model 256,
                                feed-forward width 256, 512, 1024 or 2048, at most 8 layers, and B * T * max(F, 768) * 4 <
                                2^31 (the kernels form 32-bit byte offsets into [B*T][width] tensors and keep the top bit
                                for "out of range"): 699 050 rows up to F = 512, 524 287 at 1024, 262 143 at 2048 */
int lr_tfm_rowblock_supported(int B, int T, int Dm, int F, int nlayers);
size_t lr_tfm_reserve_bytes(int mode, int B, int T, int I, int Dm, int nhead, int F, int nlayers);
size_t lr_tfm_workspace_bytes(int mode, int B, int T, int I, int Dm, int nhead, int F, int nlayers);
int lr_tfm_forward(int mode, const void* x, const int32_t* key_lens, const float* const* weights, const float* pe,
                   float* h_out, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, int B, int T,
                   int I, int Dm, int nhead, int F, int nlayers, float eps, lr_stream_t stream);
int lr_tfm_backward_data(int mode, const int32_t* key_lens, const float* const* weights, const float* dh_out, void* dx,
                         void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, int B, int T, int I,
                         int Dm, int nhead, int F, int nlayers, lr_stream_t stream);
int lr_tfm_backward_weights(int mode, const void* x, float* const* grads, int accumulate, void* reserve,
                            size_t reserve_bytes, void* workspace, size_t workspace_bytes, int B, int T, int I, int Dm,
                            int nhead, int F, int nlayers, lr_stream_t stream);
/* the stack with every layer's self-attention under the chunk mask of lr_attn_softmax_forward_chunked (training and
 * one-shot inference of a model that is to stream); the same reserve / workspace sizes, and lr_tfm_backward_weights
 * as it is (attention has no weights).  backward_data must be given the forward's chunk / left_chunks.  chunk = 0: the
 * two entry points above, bit for bit. */
int lr_tfm_forward_chunked(int mode, const void* x, const int32_t* key_lens, const float* const* weights, const float* pe,
                           float* h_out, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes, int B,
                           int T, int I, int Dm, int nhead, int F, int nlayers, float eps, int chunk, int left_chunks,
                           lr_stream_t stream);
int lr_tfm_backward_data_chunked(int mode, const int32_t* key_lens, const float* const* weights, const float* dh_out,
                                 void* dx, void* reserve, size_t reserve_bytes, void* workspace, size_t workspace_bytes,
                                 int B, int T, int I, int Dm, int nhead, int F, int nlayers, int chunk, int left_chunks,
                                 lr_stream_t stream);

/* ---- A10 sessions (BUILD-DEFINED, no reference symbol): the chunk-limited encoder stack fed chunk by chunk -------- */
/* A transformer session is one device buffer owned by the caller: for B independent slots the input frames of the
 * attention chunk that is not whole yet and, per layer, the keys and values of the last left_chunks * chunk positions
 * (lipreading_amd/csrc/lr_tfm_stream.hip).  It computes, chunk by chunk, what lr_tfm_forward_chunked
 * (mode 0: exact fp32 products, fp32 softmax) computes on the whole clip with key_lens = the frames fed: a chunk's rows
 * are emitted once its last frame is in, or when the stream ends.  Fed the same frames in any pieces, in any slot of any
 * batch, whatever the other slots do, a slot computes the same bits and leaves the same state bytes.  Inference only.
 * With C = chunk, Lc = left_chunks, a256(n) = n rounded up to a multiple of 256:
 *   state     B slots of a256(64 + a16(4 * (C - 1) * I) + 4 * nlayers * Lc * C * 2 * Dm) bytes each: 16 int32 of header
 *             (magic, I, Dm, nhead, F, nlayers, C, Lc, frames consumed n, rows emitted, ended, status bits, 0 ...), the
 *             PENDING frames [C - 1][I] fp32 (frames E(n) .. n - 1 from row 0, zeros behind them), then per layer a RING
 *             [Lc * C][2 * Dm] fp32 of keys | values, position p at index p % (Lc * C)
 *   workspace rows of this advance, R = B * (chunk_T + C - 1): the gathered input [R][I], positional rows, two [R][Dm]
 *             activations, [nlayers][R][3 Dm] projections, one layer's intermediates, logits [R][Cv]
 * Limits (else 0 bytes / LR_ERR_UNSUPPORTED): 1 <= C <= 32, (Lc + 1) * C <= 128, head dimension a multiple of 4 and
 * <= 64, what lr_tfm_reserve_bytes(0, ...) accepts, B <= 65535, chunk_T <= 65536, Cv <= 4096, R <= 2^20 - 16.
 * NULLs, negative sizes and misaligned buffers answer LR_ERR_INVALID_ARG, buffers smaller than their *_bytes
 * LR_ERR_WORKSPACE, before any launch: nothing is written.  state and workspace must be 16-byte aligned. */
#define LR_TFM_STREAM_MISMATCH 1   /* a call's configuration is not the slot's */
#define LR_TFM_STREAM_AFTER_END 2  /* frames were given to a slot whose stream had ended */
#define LR_TFM_STREAM_FULL 4       /* the slot's frames would pass pe_rows */

size_t lr_tfm_stream_state_bytes(int B, int I, int Dm, int nhead, int F, int nlayers, int chunk,
                                 int left_chunks);                                    /* 0 for arguments it rejects */
size_t lr_tfm_stream_workspace_bytes(int B, int chunk_T, int I, int Dm, int nhead, int F, int nlayers, int Cv, int chunk,
                                     int left_chunks);                                /* 0 for arguments it rejects */

/* Slots with mask[b] != 0 (mask [B] int32 on the device; NULL: all) get the header of this configuration, no pending
 * frame, zero rings, 0 frames, not ended and no status bit, whatever they held; the others keep every bit. */
int lr_tfm_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int B, int I, int Dm, int nhead, int F,
                        int nlayers, int chunk, int left_chunks, lr_stream_t stream);

/* Slot b consumes frames [0, clamp(sizes[b], 0, chunk_T)) of x[b] (x + b * stride_b + t * stride_t in floats, I
 * contiguous floats; sizes NULL = chunk_T; 0 without end: the slot is idle and keeps every bit).  end [B] int32 or NULL:
 * non-zero = the slot's stream ends with this call's frames (chunk_T == 0, x NULL: a flush).  weights / pe / eps as
 * lr_tfm_forward (host array of 2 + 12 * nlayers device pointers); the frame at absolute position t takes pe[t], and a
 * slot holds at most pe_rows frames.  head_w [Cv][Dm], head_b, head_mask [Cv] (all three or none; none: log_probs NULL).
 * With E(n, ended) = ended ? n : (n / C) * C the slot emits counts[b] = E(after) - E(before) rows, packed from row 0 of
 * h_out [B][rows][Dm] (may be NULL) and log_probs [B][rows][Cv], rows = chunk_T + C - 1; at and past counts[b] h_out
 * holds zeros and log_probs the head of the zero row.  An advance may complete several chunks of a slot.  A slot whose
 * header is not this configuration keeps its bytes and gets LR_TFM_STREAM_MISMATCH, an ended slot given frames
 * LR_TFM_STREAM_AFTER_END, one whose frames would pass pe_rows LR_TFM_STREAM_FULL (counts[b] = 0; only the status word
 * changes, and the bit stays until a reset).  Launches: 1 gather, 1 input projection, 7 per layer (QKV, cached
 * attention, out-projection, LN1, two feed-forward products, LN2), 2 for the head, 1 commit. */
int lr_tfm_stream_advance(const float* x, int64_t stride_b, int64_t stride_t, const int32_t* sizes, const int32_t* end,
                          const float* const* weights, const float* pe, int pe_rows, const float* head_w,
                          const float* head_b, const float* head_mask, float* h_out, float* log_probs, int32_t* counts,
                          void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, int B, int chunk_T,
                          int I, int Dm, int nhead, int F, int nlayers, int Cv, int chunk, int left_chunks, float eps,
                          lr_stream_t stream);

/* frames consumed, rows emitted, ended, status, each [B] int32 on the device (each may be NULL, not all): what the
 * slots hold, without changing a byte of the state.  A slot whose header is not this configuration reads as zeros with
 * LR_TFM_STREAM_MISMATCH in status[b]. */
int lr_tfm_stream_read(const void* state, size_t state_bytes, int32_t* frames, int32_t* emitted, int32_t* ended,
                       int32_t* status, int B, int I, int Dm, int nhead, int F, int nlayers, int chunk, int left_chunks,
                       lr_stream_t stream);

/* ---- A4: CTC loss — src/train/ctc_loss.py:28-114 ---------------------------------------- */

/* Per-sample CTC negative log-likelihood and its gradient, blank = 0, the same recursion as
 * torch.nn.functional.ctc_loss which the reference calls at ctc_loss.py:85.
 *   log_probs  element (b,t,c) at log_probs[b*stride_b + t*stride_t + c]; so both the
 *              reference's (B,T,V') tensor and its transposed (T,B,V') view are accepted
 *   labels     [B, label_stride] int32, ALREADY shifted by +1 (ctc_loss.py:80), PAD after
 *              label_lens[b]
 *   frame_lens [B] int32 (input lengths), label_lens [B] int32
 *   nll        [B]  out: -log p(labels | log_probs); +inf when no valid alignment
 *   grad       out, same addressing as log_probs, or NULL for loss only.  grad[b,t,c] =
 *              grad_weight[b] * (exp(lp) - exp(log sum_{s:l'_s=c} alpha_t(s) beta_t(s) + nll - lp))
 *              for t < frame_lens[b], 0 after — torch's ctc_loss backward formula.
 *              grad_weight may be NULL (= 1).  Samples whose nll is inf or whose
 *              grad_weight is 0 get an all-zero gradient.
 *   workspace  lr_ctc_workspace_bytes(B, T, C, max_label_len) bytes; lr_ctc_grad must get the
 *              workspace lr_ctc_nll filled (alpha/beta tables and label chains), unmodified.
 * T is the padded time extent (number of t rows addressed), C = V'+... number of classes,
 * max_label_len <= 256 bounds label_lens (ctc_loss.py:46). */
size_t lr_ctc_workspace_bytes(int B, int T, int C, int max_label_len);

int lr_ctc_nll(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* labels,
               int label_stride, const int32_t* frame_lens, const int32_t* label_lens, float* nll,
               void* workspace, size_t workspace_bytes, int B, int T, int C, int max_label_len,
               lr_stream_t stream);

int lr_ctc_grad(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* labels,
                int label_stride, const int32_t* frame_lens, const int32_t* label_lens,
                const float* nll, const float* grad_weight, float* grad, void* workspace,
                size_t workspace_bytes, int B, int T, int C, int max_label_len,
                lr_stream_t stream);

/* lr_ctc_grad with every grad_weight[b] multiplied by the DEVICE scalar grad_scale[0] (NULL = 1): the incoming
 * gradient of the reduced loss in an autograd backward (_CTCLossFunction.backward), without an elementwise launch
 * to fold it into the weights first. */
int lr_ctc_grad_scaled(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* labels,
                       int label_stride, const int32_t* frame_lens, const int32_t* label_lens,
                       const float* nll, const float* grad_weight, const float* grad_scale, float* grad,
                       void* workspace, size_t workspace_bytes, int B, int T, int C, int max_label_len,
                       lr_stream_t stream);

/* The reference's batch reduction (ctc_loss.py:46-114) evaluated on the device from the
 * per-sample nll, so no host round trip is needed to apply it:
 *   - samples with label_lens > 256 are dropped (:46);
 *   - the (ascending) batch is cut into runs of equal frame_len (:64-65);
 *   - a run containing an inf nll drops those samples (:87-101); a run with none left is
 *     skipped WITHOUT advancing the run start (:92 `continue` before :107), so its samples
 *     are re-examined as part of the next run;
 *   - 'mean': each run's torch-'mean' (mean of nll/clamp(label_len,1)) is multiplied by
 *     `minibatch_size`, which the reference reads BEFORE slicing (:74) — the whole batch for
 *     the first run, the previous run's size afterwards — and `count` accumulates the same
 *     number (:103-105); 'sum': plain sum.
 *   out_loss[0]   the loss (total/count or total); 0 when status != 0
 *   out_status[0] 0 = ok, 1 = reference would return None (everything dropped / total == 0)
 *   grad_weight   [B] d out_loss / d nll[b]  (0 for dropped samples) -> lr_ctc_grad */
int lr_ctc_reduce(const float* nll, const int32_t* frame_lens, const int32_t* label_lens,
                  int reduction, float* out_loss, int32_t* out_status, float* grad_weight, int B,
                  lr_stream_t stream);

/* lr_ctc_nll followed by lr_ctc_reduce with the same arguments, as ONE launch when every label has at most 31
 * characters (the one-wave recursion kernel: its last workgroup to finish runs the batch reduction — round 5; the
 * train step's path, lipreading_amd/ctc.py), as the two launches otherwise.  Launches of this entry must not overlap
 * in time within a process (one completion counter; launches on one stream never do). */
int lr_ctc_nll_reduce(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* labels,
                      int label_stride, const int32_t* frame_lens, const int32_t* label_lens, float* nll,
                      void* workspace, size_t workspace_bytes, int reduction, float* out_loss, int32_t* out_status,
                      float* grad_weight, int B, int T, int C, int max_label_len, lr_stream_t stream);

/* The train loop's label plumbing in ONE launch (train_better_model.py:31-32 labels = chars[:, 1:], label_lens =
 * char_lens - 1; ctc_loss.py:42,80 int32 integers, labels moved up by one so that index 0 is the blank):
 *   labels_p1[b][l]  = (int32) chars[b * chars_stride + 1 + l] + 1     l < L (= chars' width - 1)
 *   frame_lens32[b]  = (int32) frame_lens[b];   label_lens32[b] = (int32) char_lens[b] - 1
 * (as torch ops these are five elementwise launches at the head of every step). */
int lr_ctc_prepare_i64(const int64_t* chars, int64_t chars_stride, const int64_t* frame_lens, const int64_t* char_lens,
                       int32_t* labels_p1, int32_t* frame_lens32, int32_t* label_lens32, int B, int L,
                       lr_stream_t stream);

/* ---- A6: CTC greedy decode — src/models/lipreader/decoder.py:165-197 -------------------- */

/* argmax over classes (first maximum, as torch.max), then per sample for t < sizes[b]:
 * drop blanks, drop a frame whose argmax equals the previous FRAME's argmax (:168-173).
 *   probs    element (b,t,c) at probs[b*stride_b + t*stride_t + c]
 *   sizes    [B] int32 or NULL (= T)
 *   class_map [C] int32 or NULL: the reference compares CHARACTERS (labels[i] == labels[j]),
 *            so with duplicate label strings the caller passes the canonical index per class
 *   out_ids  [B,T] int32 kept (mapped) class ids, out_offsets [B,T] int32 frame index of each kept id,
 *   out_lens [B] int32 number kept.  Entries past out_lens[b] are -1. */
int lr_ctc_greedy_decode(const float* probs, int64_t stride_b, int64_t stride_t,
                         const int32_t* sizes, const int32_t* class_map, int32_t* out_ids,
                         int32_t* out_offsets, int32_t* out_lens, int B, int T, int C, int blank,
                         lr_stream_t stream);

/* ---- A6b: CTC prefix beam search — src/models/lipreader/decoder.py:90-143 (BeamCTCDecoder) ------- */
/* The reference delegates to ctcdecode's CTCBeamDecoder(lm_path=None) on the CPU; the specification
 * here is this build's (lipreading_amd/csrc/lr_ctc_beam.hip).  No language model.
 *   probs     element (b,t,c) at probs[b*stride_b + t*stride_t + c], fp32; log_input = 1 when the values
 *             are log-probabilities.  sizes [B] int32 or NULL (= T); frames t >= sizes[b] are never read.
 *   cutoff_top_n, cutoff_prob, beam_width, blank: ctcdecode's parameters of the same names.
 *   out_ids / out_offsets [B][W][T] int32 (-1 padded), out_lens [B][W] int32 (0 = empty slot),
 *   out_scores [B][W] fp32 = -log P(prefix), ascending (+inf in empty slots).
 * Limits: beam_width <= 128, cutoff_top_n <= 64, C <= 256, 1 + T*beam_width < 2^31 (else LR_ERR_UNSUPPORTED). */

/* Workspace lr_ctc_beam_decode needs (0 for arguments it rejects) — replaces the CPU buffers of
 * ctcdecode's CTCBeamDecoder.decode (decoder.py:139-140). */
size_t lr_ctc_beam_workspace_bytes(int B, int T, int C, int beam_width, int cutoff_top_n);

/* CTCBeamDecoder.decode (decoder.py:139-140): per-frame pruning across the chip, then one workgroup per
 * utterance for the frame loop. */
int lr_ctc_beam_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                       int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                       int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens, float* out_scores,
                       void* workspace, size_t workspace_bytes, int B, int T, int C, lr_stream_t stream);

/* ---- A6c: the same search with an ARPA n-gram word language model — the reference's lm_path / alpha / beta ---- */
/* The specification and the blob's layout are in lipreading_amd/csrc/lr_ctc_beam.hip.
 * Limits: order <= 6, vocabulary < 2^24 (the packer's LR_ERR_UNSUPPORTED); the search's limits as above. */

/* Bytes of the packed LM blob (0 for arguments lr_ctc_beam_lm_pack rejects).  counts[order]: n-grams per order;
 * dict_chars: total class ids of the dictionary's spellings. */
size_t lr_ctc_beam_lm_pack_bytes(int order, const int64_t* counts, int64_t dict_chars);

/* Host only (no device call): pack an ARPA model and its dictionary into `out` (host memory).
 *   words       every n-gram's word ids, order 1 first, each n-gram's words oldest first; unigram i is word id i
 *   log10_prob, log10_backoff  per n-gram, as in the ARPA text (an absent backoff is 0)
 *   bos         word id of <s>, -1 if none
 *   dict_word[dict_n], dict_off[dict_n+1], dict_cls[dict_off[dict_n]]: the dictionary's words and their
 *               spellings in class ids (< n_classes <= 256).
 * A duplicate n-gram, an n-gram whose (k-1)-gram prefix is not listed, or two words with one spelling is
 * LR_ERR_INVALID_ARG. */
int lr_ctc_beam_lm_pack(void* out, size_t out_bytes, int order, const int64_t* counts, const int32_t* words,
                        const double* log10_prob, const double* log10_backoff, int bos, int64_t dict_n,
                        const int32_t* dict_word, const int64_t* dict_off, const int32_t* dict_cls, int n_classes);

/* lr_ctc_beam_decode plus the language model: lm = the packed blob on the device, class_roles [C] int32 on the
 * device (0 transparent, 1 word character, 2 space), alpha / beta finite.  Workspace: lr_ctc_beam_workspace_bytes.
 * out_scores = -(log mass + the final word's term), ascending. */
int lr_ctc_beam_lm_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                          int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                          const void* lm, const int32_t* class_roles, float alpha, float beta,
                          int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens, float* out_scores,
                          void* workspace, size_t workspace_bytes, int B, int T, int C, lr_stream_t stream);

/* ---- A6c': the same searches with hotwords (contextual biasing) — no counterpart in the reference ---- */
/* Phrases given as class ids raise the selection key of hypotheses that spell them, while the search runs; the
 * specification and the blob's layout are in lipreading_amd/csrc/lr_ctc_beam.hip.
 * Limits: at most 4096 automaton nodes and 1024 phrases, n_classes <= 256 (LR_ERR_UNSUPPORTED). */

/* Bytes of the packed hotword blob (0 for arguments lr_ctc_beam_bias_pack rejects).  phrase_off[n_phrases+1]
 * (phrase_off[0] = 0) delimits the phrases' class ids in phrase_cls; anchor: the class of ' ' (a phrase then matches
 * only at the start of a word) or -1. */
size_t lr_ctc_beam_bias_pack_bytes(int n_phrases, const int64_t* phrase_off, const int32_t* phrase_cls, int anchor,
                                   int n_classes);

/* Host only (no device call): build the Aho-Corasick automaton over the phrases and write it into `out` (host
 * memory) as one dense table.  weights[n_phrases] fp32, each finite and > 0.  An empty phrase, a class id outside
 * [0, n_classes), a bad weight or no phrase at all is LR_ERR_INVALID_ARG. */
int lr_ctc_beam_bias_pack(void* out, size_t out_bytes, int n_phrases, const int64_t* phrase_off,
                          const int32_t* phrase_cls, const float* weights, int anchor, int n_classes);

/* lr_ctc_beam_decode plus the hotwords: bias = the packed blob on the device.  Workspace:
 * lr_ctc_beam_workspace_bytes.  out_scores = -(log mass + the completed hotwords' weights), ascending. */
int lr_ctc_beam_bias_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                            int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                            const void* bias, int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens,
                            float* out_scores, void* workspace, size_t workspace_bytes, int B, int T, int C,
                            lr_stream_t stream);

/* lr_ctc_beam_lm_decode plus the hotwords.  The dictionary is unchanged: a hotword whose words are not ARPA
 * unigrams stays unreachable.  out_scores = -(log mass + the final word's term + the completed hotwords' weights). */
int lr_ctc_beam_lm_bias_decode(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                               int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                               const void* lm, const int32_t* class_roles, float alpha, float beta, const void* bias,
                               int32_t* out_ids, int32_t* out_offsets, int32_t* out_lens, float* out_scores,
                               void* workspace, size_t workspace_bytes, int B, int T, int C, lr_stream_t stream);

/* ---- A6c'': sessions — the same four searches fed chunk by chunk — no counterpart in the reference ---- */
/* A session is one device buffer owned by the caller: for B independent utterance slots a 32-byte header each (the
 * configuration of the last reset, frames consumed, live hypotheses, status bits), the beam's arrays in beam order and
 * the trie's three node tables [B][1 + max_frames * beam_width] (lipreading_amd/csrc/lr_ctc_beam.hip).
 * Fed the same frames in any chunks, a session holds what the one-shot entry computes, bit for bit; offsets count the
 * session's frames.  lm == NULL / bias == NULL select the variant as with_lm / with_bias do at the reset.
 * Limits: the one-shot search's, with max_frames in T's place (else 0 bytes / LR_ERR_UNSUPPORTED). */
#define LR_BEAM_STREAM_OVERFLOW 1 /* frames past max_frames were offered and not consumed */
#define LR_BEAM_STREAM_MISMATCH 2 /* a call's beam_width, max_frames, B or variant is not the slot's */

/* Bytes of the state (0 for arguments the reset rejects). */
size_t lr_ctc_beam_stream_state_bytes(int B, int max_frames, int beam_width, int with_lm, int with_bias);

/* Workspace of one advance of chunk_T frames: the pruned per-frame class lists (0 for arguments it rejects). */
size_t lr_ctc_beam_stream_workspace_bytes(int B, int chunk_T, int C, int beam_width, int cutoff_top_n);

/* Slots with mask[b] != 0 (mask [B] int32 on the device; NULL: all slots) go back to the empty prefix, the model's
 * <s> context and the automaton's start state, with 0 frames and no status bit; every other slot keeps every bit.
 * Under a mask the slot must already carry this configuration (else it is left alone and gets
 * LR_BEAM_STREAM_MISMATCH); with NULL whatever the buffer held is overwritten.  The node tables are not cleared. */
int lr_ctc_beam_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int B, int max_frames,
                             int beam_width, int with_lm, int with_bias, const void* lm, const void* bias,
                             lr_stream_t stream);

/* Consumes frames [0, clamp(sizes[b], 0, chunk_T)) of slot b's chunk (sizes NULL = chunk_T): two launches, the
 * pruning of lr_ctc_beam_decode over the chunk and the frame loop from the slot's beam.  A slot with no frame keeps
 * every bit.  Frames past max_frames are not consumed (LR_BEAM_STREAM_OVERFLOW); a slot whose header disagrees with
 * beam_width, max_frames, B or the variant is left alone (LR_BEAM_STREAM_MISMATCH).  The bits stay until a reset. */
int lr_ctc_beam_stream_advance(const float* probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                               int log_input, int cutoff_top_n, float cutoff_prob, int beam_width, int blank,
                               const void* lm, const int32_t* class_roles, float alpha, float beta, const void* bias,
                               void* state, size_t state_bytes, int max_frames, void* workspace,
                               size_t workspace_bytes, int B, int chunk_T, int C, lr_stream_t stream);

/* What the one-shot entry would answer if every slot's stream ended now — the variant's end terms and re-sort
 * applied — without changing a byte of the state.  The layout is read from the slots' headers.
 *   out_ids / out_offsets [B][n_out][out_width] int32, -1 padded: the first n_out hypotheses, of each the first
 *                         min(len, out_width) ids;  out_lens [B][n_out] the TRUE lengths;  out_scores [B][n_out]
 *                         (+inf in empty slots)
 *   out_stable  [B]  length of the longest common prefix, as id strings, of ALL live hypotheses: every later
 *                    hypothesis extends a live one, so these ids of the best hypothesis are final (their offsets
 *                    are not: two trie nodes can spell one prefix)
 *   out_frames, out_status [B]  frames consumed, LR_BEAM_STREAM_* bits (MISMATCH also for a header that does not
 *                    fit state_bytes or the variant lm / bias select; the slot's outputs are then empty) */
int lr_ctc_beam_stream_read(const void* state, size_t state_bytes, const void* lm, float alpha, float beta,
                            const void* bias, int n_out, int out_width, int32_t* out_ids, int32_t* out_offsets,
                            int32_t* out_lens, float* out_scores, int32_t* out_stable, int32_t* out_frames,
                            int32_t* out_status, int B, lr_stream_t stream);

/* ---- A6d: edit-distance scoring of decoded ids — decoder.py:44-73 (Decoder.wer / Decoder.cer) on the device ---- */
/* The reference scores joined label strings on the host with the Levenshtein package.  Here the ids stay on the
 * device (lipreading_amd/csrc/lr_edit.hip): every class id spells a string over the caller's
 * alphabet of K symbols — spell_sym[spell_off[c] .. spell_off[c+1]) for class c, spell_off [n_classes+1], both int32
 * on the device; a dropped marker spells nothing — and a sequence expands to the concatenation of its spellings.
 *   LR_EDIT_CHARS        symbols equal to space_sym (-1: none) are deleted from both expansions; Levenshtein distance
 *                        over symbols (Decoder.cer).
 *   LR_EDIT_WORDS        both expansions are split at runs of space_sym, no empty words (str.split()); Levenshtein
 *                        distance over words, two words equal iff their symbols are (Decoder.wer).
 *   LR_EDIT_CHARS_ALIGN  LR_EDIT_CHARS plus the alignment: from (n, m), at (i, j) the diagonal if i, j > 0 and
 *                        D[i][j] == D[i-1][j-1] + (h[i-1] != r[j-1]) (a hit, or a substitution), else the reference
 *                        side if j > 0 and D[i][j] == D[i][j-1] + 1 (a deletion), else the hypothesis side (an
 *                        insertion).  conf [(K+1)][(K+1)] int64, or NULL: conf[r][h] += 1 per diagonal step,
 *                        conf[r][K] per deletion, conf[K][h] per insertion.
 *   hyp / ref            int32 ids, pair b's row at hyp + b * hyp_stride (elements), hyp_width / ref_width ids wide;
 *                        hyp_lens / ref_lens int32, pair b's at [b * *_lens_stride].  Ids past the length are never
 *                        read.
 *   out                  [B][LR_EDIT_OUT_STRIDE] int32: status, distance, reference length, hypothesis length (in
 *                        units), hits, substitutions, insertions, deletions (0 without alignment).  status 0, or
 *                        LR_EDIT_BAD_ID (an id inside the length outside [0, n_classes)), LR_EDIT_BAD_LENGTH (a length
 *                        outside [0, width]), LR_EDIT_BAD_SPELLING (an expansion longer than width * max_spelling):
 *                        such a pair reads nothing out of bounds, writes zeros and adds to nothing.
 *   totals               NULL or int64 [16], ACCUMULATED: [0..7] for the character unit, [8..15] for the word unit:
 *                        distance, reference length, hypothesis length, hits, substitutions, insertions, deletions,
 *                        pairs.
 *   gate                 NULL or one int32 on the device: when *gate != 0, totals and conf are left untouched (out is
 *                        still written) — lets a caller discard a batch by a device-side fault word without reading it.
 * Limits, decided from the widths and max_spelling (the longest spelling) alone: width * max_spelling <=
 * LR_EDIT_MAX_CHARS per side, LR_EDIT_MAX_ALIGN_CHARS per side with the alignment, else LR_ERR_UNSUPPORTED before
 * any launch.  K < 65535. */
#define LR_EDIT_CHARS 0
#define LR_EDIT_WORDS 1
#define LR_EDIT_CHARS_ALIGN 2
#define LR_EDIT_OUT_STRIDE 8
#define LR_EDIT_MAX_CHARS 4096
#define LR_EDIT_MAX_ALIGN_CHARS 2048
#define LR_EDIT_BAD_ID (-1)
#define LR_EDIT_BAD_LENGTH (-2)
#define LR_EDIT_BAD_SPELLING (-3)

/* Workspace lr_edit_distance needs; 0 for arguments it rejects (invalid or past the limits).  16 bytes, except for an
 * alignment whose 2-bit-per-cell walk-back table does not fit beside the sequences in 64 KB of LDS: then
 * B * align4(hyp_width * max_spelling * ceil(ref_width * max_spelling / 4)) bytes. */
size_t lr_edit_workspace_bytes(int B, int hyp_width, int ref_width, int max_spelling, int mode);

/* One launch, one pair per workgroup. */
int lr_edit_distance(const int32_t* hyp, int64_t hyp_stride, const int32_t* hyp_lens, int64_t hyp_lens_stride,
                     const int32_t* ref, int64_t ref_stride, const int32_t* ref_lens, int64_t ref_lens_stride,
                     const int32_t* spell_off, const int32_t* spell_sym, int n_classes, int max_spelling,
                     int space_sym, int mode, int32_t* out, int64_t* totals, int64_t* conf, int K,
                     const int32_t* gate, void* workspace, size_t workspace_bytes, int B, int hyp_width,
                     int ref_width, lr_stream_t stream);

/* ---- A6e (BUILD-DEFINED, no reference symbol): CTC forced alignment — when is each character and word spoken ---- */
/* The reference has no aligner; the specification is this build's (lipreading_amd/csrc/lr_align.hip),
 * the yardstick a NumPy restatement kept with the tests.  Per sample b, n = sizes[b] frames of fp32 log-probabilities
 * and a target y[0..L) of class ids (L = target_lens[b], blank excluded).  States s = 0..2L, even = blank, odd s =
 * y[(s-1)/2].  v[0][0] = lp[0][blank], v[0][1] = lp[0][y[0]], -inf elsewhere; for t >= 1 v[t][s] = best +
 * lp[t][cls(s)], best over v[t-1][s] (code 0), v[t-1][s-1] (code 1, s >= 1), v[t-1][s-2] (code 2; s odd, s >= 3,
 * cls(s) != cls(s-2)) IN THIS ORDER, a later candidate replacing an earlier one only if strictly greater.  All fp32:
 * one add per cell and comparisons.  End state 0 if L == 0, else 2L if v[n-1][2L] > v[n-1][2L-1], else 2L-1; total =
 * v[n-1][end]; the path is read backwards through the codes.
 *   log_probs    element (b,t,c) at log_probs[b*stride_b + t*stride_t + c]; NaN is unspecified
 *   sizes        [B] int32 or NULL (= T);  targets [B][target_stride] int32, ids past target_lens[b] are never read
 *   class_roles  [C] int32 (0 transparent, 1 word character, 2 space, as lr_ctc_beam_lm_decode) or NULL: no word
 *                outputs, the word pointers and n_words may then be NULL
 *   frame_token  [B][T]: the token index a frame belongs to, -1 on blank frames and for t >= n
 *   tok_start / tok_end / tok_logp  [B][target_stride]: token i holds the contiguous frames [start, end); logp = the fp32
 *                sum of lp[t][y[i]] over them in ascending t
 *   word_first / word_count / word_start / word_end / word_logp  [B][target_stride]: a word is a maximal run of
 *                consecutive role-1 tokens: its first token, token count, tok_start[first], tok_end[last], and the fp32
 *                sum of its tokens' tok_logp in order.  n_words [B].
 *   total        [B] fp32;  status [B]: 0, LR_ALIGN_INFEASIBLE (total = -inf: no path spells the target in n frames),
 *                LR_ALIGN_BAD_ID (an id inside its length outside [0, C) or equal to blank), LR_ALIGN_BAD_LENGTH
 *                (sizes[b] outside [1, T] or target_lens[b] outside [0, target_stride]).
 * Entries past L / n_words are -1 (integers) and 0 (floats).  A sample with a non-zero status reads nothing out of
 * bounds and writes -1 / 0 everywhere, total = -inf and n_words = 0.
 * Limits, from the arguments alone: target_stride <= max_label_len <= 256, T <= LR_ALIGN_MAX_T, else
 * LR_ERR_UNSUPPORTED before any launch.  One launch, one sample per workgroup. */
#define LR_ALIGN_MAX_T 2048
#define LR_ALIGN_INFEASIBLE 1
#define LR_ALIGN_BAD_ID (-1)
#define LR_ALIGN_BAD_LENGTH (-2)

/* Workspace lr_ctc_align needs; 0 for arguments it rejects.  16 bytes while the 2-bit back-pointer table
 * (ceil(T / 16) dwords per state, states rounded up to 64) fits in LDS beside the sample's rows; B times that table
 * otherwise. */
size_t lr_ctc_align_workspace_bytes(int B, int T, int C, int max_label_len);

/* What lr_ctc_align will launch for these sizes, decided on the host (no device call): plan [LR_ALIGN_PLAN_WORDS]
 * int32 on the HOST = {1 for the one-wave kernel / 0 for the multi-wave one, threads per workgroup, 1 if the sample's
 * rows are staged into LDS / 0 if they are read from global memory, 1 if the back-pointer table lies in LDS / 0 if in
 * the workspace, dynamic LDS bytes}.  Same status as lr_ctc_align would give for the sizes. */
#define LR_ALIGN_PLAN_WORDS 5
int lr_ctc_align_plan(int B, int T, int C, int max_label_len, int32_t* plan);

int lr_ctc_align(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                 const int32_t* targets, int target_stride, const int32_t* target_lens, const int32_t* class_roles,
                 int blank, int32_t* frame_token, int32_t* tok_start, int32_t* tok_end, float* tok_logp,
                 int32_t* word_first, int32_t* word_count, int32_t* word_start, int32_t* word_end, float* word_logp,
                 int32_t* n_words, float* total, int32_t* status, void* workspace, size_t workspace_bytes, int B, int T,
                 int C, int max_label_len, lr_stream_t stream);

/* ---- A6f (BUILD-DEFINED, no reference symbol): CTC keyword spotting — where is each keyword spoken -------------- */
/* The reference has no spotter; the specification is this build's (lipreading_amd/csrc/lr_spot.hip),
 * the yardstick a NumPy restatement kept with the tests (tests/spot_cases.py).  Per sample b with n = sizes[b] frames
 * and per keyword y[0..L) (L = kw_lens[k], blank excluded): m[t] = max_c lp[t][c], d[t][c] = lp[t][c] - m[t] (one fp32
 * subtraction).  States j = 0..2L-2: even j is token y[j/2], odd j the blank BETWEEN two tokens; no leading or trailing
 * blank.  Every state carries (v, st), (-inf, -1) before frame 0.  For t = 0..n-1 and every j, `best` is chosen among
 * stay (v[t-1][j]), step (v[t-1][j-1], j >= 1), skip (v[t-1][j-2]; j even, j >= 2, y[j/2] != y[j/2-1]) and, for j = 0
 * only, the fresh start (0.0f, t), IN THIS ORDER, a later candidate replacing an earlier one only if strictly greater;
 * v[t][j] = best.v + d[t][cls(j)] (one fp32 add), st[t][j] = best.st, or -1 when v[t][j] is -inf.
 *   log_probs   element (b,t,c) at log_probs[b*stride_b + t*stride_t + c]; a row needs one finite value; NaN and +inf
 *               are unspecified but stay in bounds
 *   sizes       [B] int32 or NULL (= T);  keywords [K][kw_stride] int32, ids past kw_lens[k] are never read
 *   min_scores  [K] fp32 or NULL
 *   end_score / end_start  [B][K][T] or both NULL: v and st of the last state per frame, -inf / -1 for t >= n
 *   hit_score / hit_start / hit_end  [B][K][max_hits] in pick order, padded with -inf / -1 / -1;  n_hits [B][K].
 *               Candidates are the frames t with a finite end_score[t] (>= min_scores[k] when given), spans
 *               [end_start[t], t + 1).  Up to max_hits times: among the candidates whose span overlaps no span already
 *               taken (s1 < e2 && s2 < e1) the greatest score, the smallest t on ties.
 *   status      [B][K]: 0, LR_SPOT_BAD_LENGTH (sizes[b] outside [1, T] or kw_lens[k] outside [1, kw_stride]; judged
 *               first), LR_SPOT_BAD_ID (an id inside the length outside [0, C) or equal to blank).  Such a pair reads
 *               nothing out of bounds and writes the padding values everywhere, n_hits = 0.
 * Limits, from the arguments alone: 1 <= kw_stride <= LR_SPOT_MAX_KW_LEN, T <= LR_SPOT_MAX_T, 1 <= max_hits <=
 * LR_SPOT_MAX_HITS, K >= 1, else LR_ERR_UNSUPPORTED before any launch.  One launch. */
#define LR_SPOT_MAX_KW_LEN 32
#define LR_SPOT_MAX_T 2048
#define LR_SPOT_MAX_HITS 16
#define LR_SPOT_BAD_ID (-1)
#define LR_SPOT_BAD_LENGTH (-2)

/* Workspace lr_ctc_spot needs when end_score is NULL; 0 for arguments it rejects.  16 bytes while the end traces of the
 * keywords a workgroup has in flight fit in LDS beside the sample's rows; B * K * T * 8 bytes otherwise.  `workspace`
 * is touched, and has to be non-NULL, only in that last case: it may be NULL with end_score given or an answer of 16. */
size_t lr_ctc_spot_workspace_bytes(int B, int T, int C, int K, int max_kw_len, int max_hits);

/* What lr_ctc_spot will launch for these sizes, decided on the host (no device call): plan [LR_SPOT_PLAN_WORDS] int32
 * on the HOST = {lanes of the segment a keyword of max_kw_len tokens takes (16 / 32 / 64), threads per workgroup,
 * keywords of that length side by side in a wave, keyword groups (wave slots: one per wave) per workgroup, 1 if the sample's rows are
 * staged into LDS as ratios / 0 if they are read from global memory with only m[t] in LDS, where the end trace lives
 * without end_score (0 LDS, 1 workspace; with end_score it is the caller's buffer), dynamic LDS bytes, keywords per
 * workgroup, the longest keyword of a 16-lane segment, the longest of a 32-lane segment, workgroups of the launch}.
 * Same status as lr_ctc_spot would give for the sizes. */
#define LR_SPOT_PLAN_WORDS 11
int lr_ctc_spot_plan(int B, int T, int C, int K, int max_kw_len, int max_hits, int32_t* plan);

int lr_ctc_spot(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                const int32_t* keywords, int kw_stride, const int32_t* kw_lens, const float* min_scores, int blank,
                int max_hits, float* hit_score, int32_t* hit_start, int32_t* hit_end, int32_t* n_hits, int32_t* status,
                float* end_score, int32_t* end_start, void* workspace, size_t workspace_bytes, int B, int T, int C, int K,
                lr_stream_t stream);

/* ---- A6g (BUILD-DEFINED, no reference symbol): CTC segmentation — re-time a whole video's captions -------------- */
/* The reference has no segmenter; the specification is this build's (lipreading_amd/csrc/lr_segment.hip, DESIGN.md
 * §24, after Kuerzinger et al. 2020), the yardstick a NumPy restatement kept with the tests (tests/segment_cases.py).
 * Per sample b: n = sizes[b] frames of fp32 log-probabilities, a target y[0..L) of class ids (L = target_lens[b], blank
 * excluded) and utterances u = 0..U-1 (U = n_utts[b]), each the token range [utt_first[u], utt_first[u] +
 * utt_count[u]) of the target; ranges may leave tokens unowned, may be empty and need not be ordered.  States as A6e:
 * s = 0..2L, even = blank, odd s = y[(s-1)/2].  Before frame 0 every v is -inf.  For t = 0..n-1 and every s, `best` is
 * chosen among stay v[t-1][s] (code 0), step v[t-1][s-1] (code 1, s >= 1), skip v[t-1][s-2] (code 2; s odd, s >= 3,
 * cls(s) != cls(s-2)) and the fresh start 0.0f (code 3; s <= 1 and (t == 0 or LR_SEG_FREE_START)) IN THIS ORDER, a
 * later candidate replacing an earlier one only if strictly greater; v[t][s] = best + lp[t][cls(s)] (one fp32 add) and
 * the code goes into the 2-bit table.  With LR_SEG_FREE_START clear this is A6e's recursion (0.0f + x == x).
 * End: the candidates of frame t are v[t][2L-1] then v[t][2L] (L == 0: v[t][0] alone), over t = 0..n-1 ascending with
 * LR_SEG_FREE_END, t = n-1 alone without, the same strictly-greater rule; total = the chosen value.  The walk back
 * follows the codes and stops after the frame whose code is 3, or at frame 0.
 *   log_probs    element (b,t,c) at log_probs[b*stride_b + t*stride_t + c]; frames t >= n are never read; NaN is
 *                unspecified but stays in bounds
 *   sizes        [B] int32 or NULL (= T);  targets [B][target_stride] int32, ids past target_lens[b] are never read
 *   utt_first / utt_count  [B][utt_stride] int32, n_utts [B] int32; all three (and the utt_* outputs) may be NULL:
 *                no utterance outputs
 *   flags        LR_SEG_FREE_START | LR_SEG_FREE_END
 *   span         [B][2]: {first frame of the path, one past its last}
 *   frame_token  [B][T]: the token of an odd state on the path, -1 on blank frames, outside the span and for t >= n
 *   tok_start / tok_end / tok_logp  [B][target_stride]: as A6e (contiguous frames, fp32 sum in ascending t)
 *   utt_start / utt_end / utt_frames / utt_logp / utt_worst  [B][utt_stride]: tok_start[first], tok_end[last], the
 *                int32 sum of tok_end - tok_start over its tokens, the fp32 sum of their tok_logp in token order, the
 *                target index of its token with the smallest tok_logp (the first on ties).  An empty utterance and
 *                entries past U get -1, -1, 0, 0.0f, -1.
 *   total        [B] fp32;  status [B], judged in this order: LR_SEG_BAD_LENGTH (sizes[b] outside [1, T], target_lens[b]
 *                outside [0, target_stride] or n_utts[b] outside [0, utt_stride]), LR_SEG_BAD_ID (an id inside its
 *                length outside [0, C) or equal to blank), LR_SEG_BAD_UTTERANCE (a negative first or count, or first +
 *                count > L), LR_SEG_INFEASIBLE (total is -inf), else 0.
 * Entries past L are -1 (integers) and 0 (floats).  A sample with a non-zero status reads nothing out of bounds and
 * writes -1 / 0 everywhere (span included) and total = -inf.
 * Limits, from the arguments alone: T <= LR_SEG_MAX_T, target_stride <= max_tokens <= LR_SEG_MAX_TOKENS, B <=
 * LR_SEG_MAX_B (a sample is a row of the launch grids), C >= 2, else
 * LR_ERR_UNSUPPORTED / LR_ERR_INVALID_ARG before any launch.  One prepare launch, ceil(T / frames per launch) forward
 * launches whose order on `stream` is the only order between state tiles, one walk-back launch, three span launches. */
#define LR_SEG_MAX_T 65536
#define LR_SEG_MAX_TOKENS 16384
#define LR_SEG_MAX_B 65535
#define LR_SEG_FREE_START 1
#define LR_SEG_FREE_END 2
#define LR_SEG_INFEASIBLE 1
#define LR_SEG_BAD_ID (-1)
#define LR_SEG_BAD_LENGTH (-2)
#define LR_SEG_BAD_UTTERANCE (-3)

/* Workspace lr_ctc_segment needs; 0 for arguments it rejects.  With S = 2 * max_tokens + 1 rounded up to a multiple of
 * the states a workgroup owns (plan[0]): B * ((ceil(T / 16) + 2) * S * 4 + 64) bytes — the 2-bit table, 16 steps per
 * dword, the two value rows between forward launches and the sample's end record.  Past 4 GB at the limits. */
size_t lr_ctc_segment_workspace_bytes(int B, int T, int C, int max_tokens);

/* What lr_ctc_segment will launch for these sizes, decided on the host (no device call): plan [LR_SEG_PLAN_WORDS] int32
 * on the HOST = {states a workgroup owns, frames one forward launch advances, forward launches, workgroups per forward
 * launch, threads per workgroup, dynamic LDS bytes}.  Same status as lr_ctc_segment would give for the sizes. */
#define LR_SEG_PLAN_WORDS 6
int lr_ctc_segment_plan(int B, int T, int C, int max_tokens, int32_t* plan);

int lr_ctc_segment(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                   const int32_t* targets, int target_stride, const int32_t* target_lens, const int32_t* utt_first,
                   const int32_t* utt_count, int utt_stride, const int32_t* n_utts, int blank, int flags,
                   int32_t* frame_token, int32_t* tok_start, int32_t* tok_end, float* tok_logp, int32_t* utt_start,
                   int32_t* utt_end, int32_t* utt_frames, float* utt_logp, int32_t* utt_worst, int32_t* span,
                   float* total, int32_t* status, void* workspace, size_t workspace_bytes, int B, int T, int C,
                   int max_tokens, lr_stream_t stream);

/* lr_ctc_segment with its phases timed (tools/bench_segment.py): the same launches with device events between them,
 * then a wait for the last one — the one entry of A6g that synchronises.  phase_ms [3] fp32 on the HOST = milliseconds
 * of {the forward launches, the walk back, the span launches}. */
int lr_ctc_segment_phases(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                          const int32_t* targets, int target_stride, const int32_t* target_lens,
                          const int32_t* utt_first, const int32_t* utt_count, int utt_stride, const int32_t* n_utts,
                          int blank, int flags, int32_t* frame_token, int32_t* tok_start, int32_t* tok_end,
                          float* tok_logp, int32_t* utt_start, int32_t* utt_end, int32_t* utt_frames, float* utt_logp,
                          int32_t* utt_worst, int32_t* span, float* total, int32_t* status, void* workspace,
                          size_t workspace_bytes, int B, int T, int C, int max_tokens, float* phase_ms,
                          lr_stream_t stream);

/* ---- A6h (BUILD-DEFINED, no reference symbol): N-best minimum error rate training of the CTC head --------------- */
/* The reference trains the CTC head on the frame-synchronous likelihood alone; the specification is this build's
 * (lipreading_amd/csrc/lr_nbest.hip), the yardstick a float64 torch restatement kept with the tests
 * (tests/mwer_cases.py).  Per utterance b: n_b = sizes[b] frames (clamped into [0, T]) of fp32 log-probabilities
 * lp[t][c] over C classes, a blank class, and N hypothesis slots; slot n holds a class-id string y_n of len_n ids and
 * a risk r_n.
 *   hyp_status [B][N]  LR_NBEST_USED (0);
 *                      LR_NBEST_EMPTY (1): len_n < 0;
 *                      LR_NBEST_REJECTED (2): len_n > max_hyp_len, an id inside the length outside [0, C) or equal to
 *                        blank, or a non-finite r_n — such a slot reads nothing out of bounds;
 *                      LR_NBEST_INFEASIBLE (3): no alignment of y_n fits n_b frames (n_b == 0, or n_b < len_n + the
 *                        number of adjacent equal ids; also a lattice that -inf log-probabilities leave empty).
 * Over the LR_NBEST_USED slots only:
 *   ll_n   = log sum over alignments of prod_t p_t(.): the CTC recursion, a blank between repeats; len_n == 0 is
 *            legal (all blank)
 *   p_n    = exp(ll_n - logsumexp_m ll_m);   R_b = sum_n p_n r_n
 *   U      = number of utterances with at least one used slot
 *   loss   = sum_b R_b / max(U, 1) (LR_CTC_MEAN) or sum_b R_b (LR_CTC_SUM);  out_status[0] = 1 when U == 0: the loss
 *            is then 0 with an all-zero gradient (lr_ctc_reduce's "skip this batch" contract)
 *   grad[b][t][c] = g * w * sum_n p_n (r_n - R_b) occ_n(t, c) for t < n_b, exactly 0 for n_b <= t < T, where
 *            occ_n(t, c) = d ll_n / d lp[t][c] is the posterior probability, under y_n's alignments, that frame t
 *            emits class c;  g = grad_scale[0] (a DEVICE scalar, NULL = 1);  w = 1 / U (mean) or 1 (sum).  Every row
 *            sums to 0 over c, so the gradient at the logits in front of a log_softmax is the same tensor; with one
 *            used slot the coefficient, and the gradient, is exactly 0.
 * Arguments:
 *   log_probs   element (b,t,c) at log_probs[b*stride_b + t*stride_t + c];  sizes [B] int32 or NULL (= T)
 *   hyps        int32 ids, slot (b,n)'s row at hyps + b*hyp_stride_b + n*hyp_stride_n (elements): `ids[:, :N]` of the
 *               beam search's (B, W, T) output goes in as it is.  Ids past len_n are never read.
 *   hyp_lens    slot (b,n)'s at hyp_lens[b*lens_stride_b + n];  risk [B][N] fp32
 *   hyp_ll      [B][N] fp32, -inf where the status is not 0;  post [B][N] = p_n, 0 where the status is not 0
 *   utt_risk    [B] = R_b (0 without a used slot);  out_loss [1], out_status [1]
 *   grad_weight [B] = w for utterances with a used slot, 0 for the others
 *   grad        addressed like log_probs; EVERY one of its B * T * C elements is written
 * The lattices, the softmax and the occupancy sums are fp64 in log space; every sum has a fixed order and nothing is
 * accumulated with atomics: two launches on the same inputs give bit-identical hyp_ll, loss and grad.
 * Limits, from the arguments alone: N <= LR_NBEST_MAX_SLOTS, C <= LR_NBEST_MAX_CLASSES, max_hyp_len <=
 * LR_NBEST_MAX_HYP_LEN, B, T >= 1, else LR_ERR_UNSUPPORTED before any launch. */
#define LR_NBEST_MAX_SLOTS 16
#define LR_NBEST_MAX_CLASSES 256
#define LR_NBEST_MAX_HYP_LEN 256
#define LR_NBEST_USED 0
#define LR_NBEST_EMPTY 1
#define LR_NBEST_REJECTED 2
#define LR_NBEST_INFEASIBLE 3

/* Workspace of the two entries below; 0 for arguments it rejects.  With S = 2 * max_hyp_len + 1 rounded up to 8:
 * two fp64 tables (alpha, beta) of B * N * T * S cells behind 2 * B * N fp64 words (ll_n and p_n (r_n - R_b)). */
size_t lr_ctc_nbest_workspace_bytes(int B, int T, int C, int N, int max_hyp_len);

/* Two launches: B * N workgroups, one per (utterance, slot), walk alpha forwards and beta backwards side by side;
 * one workgroup then takes the softmax over each utterance's slots, the expected risks and the loss. */
int lr_ctc_nbest_risk(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                      const int32_t* hyps, int64_t hyp_stride_b, int64_t hyp_stride_n, const int32_t* hyp_lens,
                      int64_t lens_stride_b, const float* risk, int blank, int reduction, float* hyp_ll, float* post,
                      int32_t* hyp_status, float* utt_risk, float* out_loss, int32_t* out_status, float* grad_weight,
                      void* workspace, size_t workspace_bytes, int B, int T, int C, int N, int max_hyp_len,
                      lr_stream_t stream);

/* One launch, one workgroup per (utterance, frame): the same inputs, lr_ctc_nbest_risk's outputs and its workspace,
 * unmodified.  Per frame the slots are added in slot order, a class's states in ascending order. */
int lr_ctc_nbest_risk_grad(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                           const int32_t* hyps, int64_t hyp_stride_b, int64_t hyp_stride_n, const int32_t* hyp_lens,
                           int64_t lens_stride_b, const float* risk, int blank, int reduction, const float* hyp_ll,
                           const float* post, const int32_t* hyp_status, const float* utt_risk,
                           const float* grad_weight, const float* grad_scale, float* grad, void* workspace,
                           size_t workspace_bytes, int B, int T, int C, int N, int max_hyp_len, lr_stream_t stream);

/* ---- A6i (BUILD-DEFINED, no reference symbol): the transducer head — RNN-T loss and greedy decoding ------------- */
/* The reference has no transducer; the specification is this build's (lipreading_amd/csrc/lr_transducer.hip,
 * lipreading_amd/transducer.py), the yardstick a float64 torch restatement kept with the tests
 * (tests/transducer_cases.py).  V1 classes in the CTC head's layout (class 0 the blank), a joint width J, per sample b
 * T_b = frame_lens[b] frames and U_b = label_lens[b] labels y_1 .. y_U_b:
 *   z(t,u)      = tanh(e[b][t][:] + p[b][u][:])                           t < T_b, 0 <= u <= U_b
 *   logits(t,u) = joint_w . z(t,u) + joint_b, classes with class_mask[c] == 0 at -inf;  lp(t,u) = log_softmax over V1
 *   alpha(0,0) = 0;  alpha(t,u) = logaddexp(alpha(t-1,u) + lp(t-1,u)[0], alpha(t,u-1) + lp(t,u-1)[y_u])
 *   nll[b] = -(alpha(T_b-1,U_b) + lp(T_b-1,U_b)[0]);  every sample with T_b >= 1 is feasible
 *   sample_status[b]  0;  LR_RNNT_BAD_LENGTH: T_b < 1, T_b > T, U_b < 0 or U_b > U;  LR_RNNT_BAD_ID: a label inside the
 *                     length that is <= 0, >= V1 or masked.  Such a sample reads nothing out of bounds, has nll 0 and
 *                     contributes nothing to the loss or to any gradient.
 *   N = number of samples with status 0;  loss = sum nll / max(N, 1) (LR_CTC_MEAN) or sum nll (LR_CTC_SUM);
 *   out_status[0] = 1 when N == 0 (lr_ctc_reduce's "skip this batch" word).
 * The gradients are those of g * loss, g = grad_scale[0] (a DEVICE scalar, NULL = 1): per node the gradient at the
 * logits is w g (occ(t,u) softmax - occ_blank(t,u) [c == 0] - occ_label(t,u) [c == y_{u+1}]) with the occupancies
 * exp(alpha + lp + beta - log Z), w = 1 / N or 1.
 * Arguments:
 *   e           element (b,t,j) at e[b*e_stride_b + t*e_stride_t + j] (the transposed view of a (T,B,J) tensor goes in
 *               as it is);  p [B][U+1][J] contiguous;  joint_w [V1][J], joint_b [V1], class_mask [V1] fp32
 *   labels      int32, sample b's row at labels + b*label_stride; ids past U_b are never read (NULL with U == 0)
 *   d_e [B][T][J], d_p [B][U+1][J] contiguous, EVERY element written;  d_joint_w [V1][J], d_joint_b [V1] written, or
 *               added onto with accumulate != 0 (as lr_tfm_backward_weights)
 * The forward writes three floats per node (log p(blank), log p(next label), the row's log-sum-exp) and alpha; no
 * (B,T,U+1,V1) or (B,T,U+1,J) tensor exists.  The backward recomputes z and the logits tile by tile (32 nodes of one
 * frame).  Products are v_mfma_f32_32x32x2_f32 (fp32 operands and accumulation); alpha, beta and log Z are fp64 in log space
 * (fp32 occupancies exp(alpha + lp + beta - log Z) lose 1e-4 of a gradient at U = 256: three numbers near 700 cancel).  Sums
 * over u (d_e), over t (d_p) and over nodes (the weights) go through per-workgroup slabs in the workspace and a
 * fixed-order combine; nothing is accumulated with atomics: two runs on the same inputs give the same bits.
 * Limits, from the arguments alone (else LR_ERR_UNSUPPORTED, workspace query 0): T <= LR_RNNT_MAX_T,
 * U <= LR_RNNT_MAX_U, V1 <= LR_RNNT_MAX_CLASSES, J <= LR_RNNT_MAX_JOINT, B <= 65535.  NULLs, B or T < 1, U < 0,
 * V1 < 2, negative strides, a misaligned (16 bytes) workspace answer LR_ERR_INVALID_ARG, a small one LR_ERR_WORKSPACE,
 * before any launch. */
#define LR_RNNT_MAX_T 4096
#define LR_RNNT_MAX_U 256
#define LR_RNNT_MAX_CLASSES 256
#define LR_RNNT_MAX_JOINT 512
#define LR_RNNT_BAD_ID (-1)
#define LR_RNNT_BAD_LENGTH (-2)

/* Workspace of the two loss entries (the backward takes the forward's, unmodified); 0 for arguments it rejects. */
size_t lr_rnnt_workspace_bytes(int B, int T, int U, int V1, int J);

/* Four launches: weight operand + statuses; the joint stage, one tile per workgroup; alpha over anti-diagonals, one
 * workgroup per sample; the batch reduction. */
int lr_rnnt_loss_forward(const float* e, int64_t e_stride_b, int64_t e_stride_t, const float* p, const float* joint_w,
                         const float* joint_b, const float* class_mask, const int32_t* labels, int64_t label_stride,
                         const int32_t* frame_lens, const int32_t* label_lens, int reduction, float* nll,
                         int32_t* sample_status, float* out_loss, int32_t* out_status, void* workspace,
                         size_t workspace_bytes, int B, int T, int U, int V1, int J, lr_stream_t stream);

/* Three launches: beta; the tiles' gradients into slabs; the combine.  nll and sample_status are the forward's. */
int lr_rnnt_loss_backward(const float* e, int64_t e_stride_b, int64_t e_stride_t, const float* p, const float* joint_w,
                          const float* joint_b, const float* class_mask, const int32_t* labels, int64_t label_stride,
                          const int32_t* frame_lens, const int32_t* label_lens, const float* nll,
                          const int32_t* sample_status, const float* grad_scale, float* d_e, float* d_p,
                          float* d_joint_w, float* d_joint_b, int accumulate, void* workspace, size_t workspace_bytes,
                          int B, int T, int U, int V1, int J, lr_stream_t stream);

/* Greedy decoding, one launch, one workgroup per sample.  For each frame t < sizes[b] (clamped into [0, T]; NULL = T):
 * the argmax of the masked logits of tanh(e_t + tables[0][c0] + tables[1][c1]) (ties to the lowest class), c0 the last
 * emitted class and c1 the one before it (0 at the start; `context` 1 or 2 tables [context][V1][J], the prediction
 * network's bias folded into table 0).  The blank ends the frame; another class is emitted, shifted into the context,
 * and the frame is evaluated again, at most max_symbols times: a frame that emits max_symbols symbols is ended and
 * counted in forced[b].  Symbol n of sample b goes to ids / frames / logp [b][n] for n < max_out; out_lens[b] counts
 * every symbol, written or not.  logp is the symbol's log-probability under the masked softmax.
 * state (may be NULL) [B][context] int32 = (c0, c1), read and written: with it out_lens and forced are read and
 * continued, and frame_base[b] (NULL = 0) is added to the reported frames, so a clip fed in pieces at any frame
 * boundaries gives the bits of the one-shot call.  Without it the decode starts from zeros.  At most
 * sizes[b] * max_symbols evaluations per sample.  Limits as above; context outside {1, 2}, max_symbols or max_out < 1
 * are LR_ERR_INVALID_ARG. */
int lr_rnnt_greedy_decode(const float* e, int64_t e_stride_b, int64_t e_stride_t, const int32_t* sizes,
                          const float* tables, const float* joint_w, const float* joint_b, const float* class_mask,
                          int32_t* state, const int32_t* frame_base, int32_t* ids, int32_t* frames, float* logp,
                          int32_t* out_lens, int32_t* forced, int B, int T, int V1, int J, int context, int max_symbols,
                          int max_out, lr_stream_t stream);

/* ---- A6j (BUILD-DEFINED, no reference symbol): transducer beam search — N-best lists, resumable ------------------ */
/* Time-synchronous beam search over A6i's model (lipreading_amd/csrc/lr_transducer_beam.hip; the
 * yardstick is the torch restatement tests/transducer_beam_cases.py).  Classes, class_mask, tables [context][V1][J]
 * (prediction bias folded into table 0) and the context (c0 = a prefix's last label, c1 = the one before it, 0 where
 * there is none) are A6i's.  A hypothesis is (prefix, score, frames): the label string, the log of the summed
 * probability of every alignment of it that the search has kept, and the frame at which each label was emitted.
 * A sample's beam starts as the empty prefix with score 0.  For every frame t < sizes[b] (clamped into [0, T]; NULL = T):
 *   1. A = the beam (at most beam_width hypotheses, in beam order); F = empty, kept in insertion order.
 *   2. Rounds s = 0 .. max_symbols.  For every h of A, in order,
 *        lp = masked log_softmax(joint_w . tanh(e_t + tables[0][c0] + tables[1][c1]) + joint_b):
 *      blank   (h.prefix, h.score + lp[0], h.frames) is offered to F.  If F holds the prefix already the two merge: the
 *              score becomes logaddexp of the two, the frames are those of the constituent whose own, unmerged score is
 *              larger (the earlier-inserted one on a tie), the entry keeps its insertion position.
 *      labels  only while s < max_symbols and len(h.prefix) < max_out: every unmasked class k >= 1 gives the candidate
 *              (h.prefix + k, h.score + lp[k], h.frames + t) of C, ordered by (rank of h in A, k).  A hypothesis
 *              already at max_out labels gives none and adds one to truncated[b] for that round.
 *      Then A = the first beam_width of a stable descending sort of C by score; an empty A ends the frame's rounds.
 *      Round max_symbols offers blanks only.
 *   3. The new beam = the first beam_width of a stable descending sort of F by score.
 * Prefixes are equal when their label strings are, label by label.  Inside a round C holds no prefix twice; the only
 * merges are F's.  Every frame ends with a blank, so a score is a partial sum of the alignments of A6i's loss: at most
 * -nll(prefix), and equal to it when nothing was pruned and max_symbols >= len(prefix).
 * Arithmetic: the joint stage (MFMA operands and accumulation) and the log-softmax are fp32; scores are accumulated,
 * compared and merged in float64, in the kernel and in the state, and reported as float32.  No atomics: two runs give
 * the same bits, and a clip fed in pieces at any frame boundaries gives the one-shot call's bits, outputs and state.
 * state   an opaque device buffer of lr_rnnt_beam_state_bytes(B, beam_width, max_out) bytes (8-byte aligned), owned by
 *         the caller: a header of 8 int32 {magic, B, beam_width, max_out, context, status, 0, 0}, then every sample's
 *         beam (float64 scores, count, lengths, labels, frames).  fresh != 0 starts every sample from the empty prefix
 *         and ignores the contents; fresh == 0 continues.  A state_bytes that is not the size of (B, beam_width,
 *         max_out) is LR_ERR_INVALID_ARG before any launch; a buffer of the right size whose header names another B,
 *         beam_width, max_out or context (or none) is refused on the device: word 5 of the header is set to
 *         LR_RNNT_BEAM_BAD_STATE (0 by every accepted call), the rest of the buffer and `truncated` are left as they
 *         are, and every sample answers out_count 0 with all scores -inf.  Nothing past state_bytes is read.
 * outputs the beam's first nbest hypotheses after the call's frames: out_ids, out_frames [B][nbest][max_out] int32 (0
 *         past the length), out_lens [B][nbest], out_scores [B][nbest] fp32 descending, -inf in empty slots (the empty
 *         prefix is a hypothesis of length 0: empty slots are told by the score), out_count [B] = hypotheses written,
 *         truncated [B] (read and continued when fresh == 0).  frame_base[b] (NULL = 0) is added to the frames emitted
 *         in this call.
 * Limits, from the arguments alone (LR_ERR_UNSUPPORTED, size queries 0): A6i's on T, V1, J and B; beam_width <=
 * LR_RNNT_BEAM_MAX_WIDTH, max_symbols <= LR_RNNT_BEAM_MAX_SYMBOLS, max_out <= LR_RNNT_MAX_U.  NULLs, sizes below 1,
 * context outside {1, 2}, nbest outside [1, beam_width], negative strides, a misaligned state or workspace (16 bytes)
 * are LR_ERR_INVALID_ARG, a small workspace LR_ERR_WORKSPACE, all before any launch. */
#define LR_RNNT_BEAM_MAX_WIDTH 32
#define LR_RNNT_BEAM_MAX_SYMBOLS 8
#define LR_RNNT_BEAM_BAD_STATE (-3)

size_t lr_rnnt_beam_state_bytes(int B, int beam_width, int max_out);
/* The zero-padded weight operand and the second buffer of the beams' frames. */
size_t lr_rnnt_beam_workspace_bytes(int B, int V1, int J, int beam_width, int max_symbols);

/* Two launches: the weight operand; the search, one workgroup per sample with the frame loop inside it. */
int lr_rnnt_beam_decode(const float* e, int64_t e_stride_b, int64_t e_stride_t, const int32_t* sizes,
                        const float* tables, const float* joint_w, const float* joint_b, const float* class_mask,
                        void* state, size_t state_bytes, int fresh, const int32_t* frame_base, int32_t* out_ids,
                        int32_t* out_frames, int32_t* out_lens, float* out_scores, int32_t* out_count,
                        int32_t* truncated, void* workspace, size_t workspace_bytes, int B, int T, int V1, int J,
                        int context, int beam_width, int max_symbols, int nbest, int max_out, lr_stream_t stream);

/* ---- A8 (BUILD-DEFINED, no reference symbol): 3-D conv frontend on bf16 MFMA -------------- */
/* The reference has no conv frontend (src/models/lipreader/model.py:122,153-156 are comments, the
 * `ced` configs are empty); BASELINE.json's north_star asks for one ("im2col + MFMA GEMM for the 3D
 * convs").  The specification is this build's; the oracle is torch conv3d on the CPU.
 * Activations are channels-last bf16 [B][T][H][W][C]; accumulation is fp32.                      */

/* clips [frames][3][H][W] (uint8, scaled by 1/255, or fp32 taken as is) -> [frames][H][W][4] bf16. */
int lr_clip_to_ndhwc_bf16(const void* clips, int is_u8, void* out, int64_t frames, int H, int W,
                          lr_stream_t stream);

/* fp32 torch Conv3d weight [Cout][Cin_real][KT][KH][KW] -> bf16 operand of the implicit GEMM:
 *   dgrad & 1 == 0: out[Cout][taps][Cin_pad]          (forward; channels >= Cin_real are zero)
 *   dgrad & 1 == 1: out[Cin_real][taps][Cout], taps flipped (data gradient of a stride-1 "same" conv
 *                   becomes lr_conv3d_forward on dZ with this operand).
 *   dgrad & 2 / dgrad & 4: the same elements in the fragment-major order of a patch-resident kernel
 *              (every 32-output-channel x 16-k, resp. 16-output-channel x 32-k, MFMA operand 1 KB
 *              contiguous); the bit is what lr_conv3d_patch_supported() returns for the layer and
 *              is passed on to lr_conv3d_forward in `flags`. */
int lr_conv3d_pack_weights(const float* W, void* out, int Cout, int Cin_real, int Cin_pad, int KT,
                           int KH, int KW, int dgrad, lr_stream_t stream);
/* n <= 8 operands in ONE launch (HOST arrays of n entries each, meaning as above): a training step packs the
 * forward operand of every layer and the data-gradient operand of the upper layers together. */
int lr_conv3d_pack_weights_multi(int n, const float* const* W, void* const* out, const int* Cout, const int* Cin_real,
                                 const int* Cin_pad, const int* KT, const int* KH, const int* KW, const int* dgrad,
                                 lr_stream_t stream);

/* Y[b,t,ho,wo,n] = act( sum_{kt,kh,kw,c} X[b,t+kt-pt,ho*s+kh-ph,wo*s+kw-pw,c] * Wp[n][(kt,kh,kw)][c]
 *                       + bias[n] ),  zero padding, temporal stride 1 and KT = 2*pt+1, spatial stride s.
 *   X bf16 [B][T][Hin][Win][Cin] (Cin % 4 == 0), Wp from lr_conv3d_pack_weights, bias fp32 or NULL,
 *   Y bf16 [B][T][Ho][Wo][Cout]; flags & 1 applies max(.,0) (ReLU);
 *   flags & 2 / flags & 4: Wp is fragment-major (lr_conv3d_pack_weights dgrad & 2 / & 4);
 *   flags & 8 (first STCNN layer only, LR_ERR_UNSUPPORTED elsewhere): X is the raw clip, uint8
 *   [B][T][3][Hin][Win], scaled by 1/255 on the way into LDS exactly as lr_clip_to_ndhwc_bf16
 *   would have — no bf16 copy of the clip is made.
 *   The first STCNN layer's geometry (Cin = 4, Cout = 32, taps 3x5x5, stride 2, padding 1,2,2) is a 3-channel
 *   layer padded to four: its kernel contracts channels 0..2 only — X[...,3] and Wp[...][3] are padding (zero, as
 *   lr_clip_to_ndhwc_bf16 and lr_conv3d_pack_weights with Cin_real = 3 write them) and are not read.
 *   Supported: that geometry; the patch-resident kernels (flags & 6); and otherwise the (Cin, Cout) pairs of the upper
 *   layers' forwards, (32, 64) and (64, 96), and of their data gradients, (64, 32) and (96, 64).  Any other shape
 *   returns LR_ERR_UNSUPPORTED.  */
int lr_conv3d_forward(const void* X, const void* Wp, const float* bias, void* Y, int B, int T, int Hin,
                      int Win, int Cin, int Cout, int KT, int KH, int KW, int stride, int pt, int ph,
                      int pw, int flags, lr_stream_t stream);
/* Forward with the ReLU -> MaxPool3d((1,2,2)) that follows it fused into the epilogue, for layers
 * with lr_conv3d_pool_fusion_supported() == 1: P bf16 [B][T][Ho/2][Wo/2][Cout] receives the pooled
 * activation and code (uint8, same shape) each window's CODE: the position 0..3 (row-major in the 2x2
 * window) of its first maximum, or 4 when the pooled activation is 0 (ReLU blocks the window's gradient);
 * the full-resolution activation is never written.  Backward of the pair: lr_unpool_code_bf16 (materialises
 * dZ), or — never writing dZ — lr_conv3d_dgrad_pooled / lr_conv3d_wgrad_pooled. */
int lr_conv3d_pool_fusion_supported(int Hin, int Win, int Cin, int Cout, int KT, int KH, int KW, int stride,
                                    int pt, int ph, int pw);
int lr_conv3d_forward_pooled(const void* X, const void* Wp, const float* bias, void* P, void* code, int B,
                             int T, int Hin, int Win, int Cin, int Cout, int KT, int KH, int KW, int stride,
                             int pt, int ph, int pw, int flags, lr_stream_t stream);
/* Data gradient of a stride-1 "same" layer whose forward fused ReLU + MaxPool, taken straight from the pooled
 * gradient dP bf16 [B][T][Ho/2][Wo/2][Cout] and the window codes (uint8, same shape): dX bf16 [B][T][Ho][Wo][Cin]
 * = conv(un-pool(dP, code), flipped / channel-transposed weights).  The kernel rebuilds its dZ patch on the way
 * into LDS; dZ itself (Ho x Wo, 75 % zeros) is never written.  Wd: lr_conv3d_pack_weights with the dgrad flag and
 * the fragment bit `_supported` returns (0: not supported — use lr_unpool_code_bf16 + lr_conv3d_forward).
 * Build-defined like the rest of the frontend (no reference symbol). */
int lr_conv3d_dgrad_pooled_supported(int Ho, int Wo, int Cout, int Cin, int KT, int KH, int KW, int pt, int ph, int pw);
int lr_conv3d_dgrad_pooled(const void* dP, const void* code, const void* Wd, void* dX, int B, int T, int Ho, int Wo,
                           int Cout, int Cin, int KT, int KH, int KW, int pt, int ph, int pw, lr_stream_t stream);
/* Non-zero when the layer (as lr_conv3d_forward sees it: Cin = contraction channels, Cout = output
 * channels) has a patch-resident kernel — the input patch of an output tile is loaded into LDS
 * once and all taps run out of LDS, instead of re-gathering it per tap.  The value is the weight
 * packing bit that kernel reads: 2 (24x24, taps 3x5x5) or 4 (12x12, taps 3x3x3). */
int lr_conv3d_patch_supported(int Hin, int Win, int Cin, int Cout, int KT, int KH, int KW, int stride,
                              int pt, int ph, int pw);

/* dW[Cout][Cin_real][KT][KH][KW] (fp32) (+)= sum_pixels dZ[pixel][n] * im2col(X)[pixel][(tap,c)];
 * dbias[n] (+)= sum_pixels dZ[pixel][n] (NULL to skip).  dZ bf16 [B][T][Ho][Wo][Cout].
 * Supported: the first STCNN layer's geometry with Cin_real = 3 (as lr_conv3d_forward) and the (Cin_pad, Cout) pairs
 * of the upper layers, (32, 64) and (64, 96); any other shape returns LR_ERR_UNSUPPORTED.                        */
size_t lr_conv3d_wgrad_workspace_bytes(int Cout, int Cin_pad, int KT, int KH, int KW);
int lr_conv3d_wgrad(const void* X, const void* dZ, float* dW, float* dbias, void* workspace,
                    size_t workspace_bytes, int accumulate, int B, int T, int Hin, int Win, int Cin_pad,
                    int Cin_real, int Cout, int KT, int KH, int KW, int stride, int pt, int ph, int pw,
                    lr_stream_t stream);

/* The same weight (and bias) gradient for a layer whose forward fused ReLU + MaxPool
 * (lr_conv3d_forward_pooled), taken straight from the pooled gradient dP and the window codes: the
 * un-pooled dZ is rebuilt tile by tile inside the kernel and never touches memory.  Build-defined like the rest of the frontend (the reference has no conv
 * stage; its only trace is the commented-out stack at src/models/lipreader/model.py:122,153-156).
 * `_supported` is non-zero for the layers that have this kernel: 1 = the first STCNN layer (flags bit 0: X is the raw
 * clip, uint8 [B][T][3][Hin][Win], scaled by 1/255 on the way into LDS as lr_clip_to_ndhwc_bf16 would, not bf16 NDHWC);
 * 2 = the stride-1 layers 2 and 3 (LR_ERR_UNSUPPORTED for a frame count whose tile table does not fit the kernel's LDS:
 * use lr_unpool_code_bf16 + lr_conv3d_wgrad then).  The codes carry the ReLU mask — code 4 — so `pooled` is not read
 * and may be NULL; dbias = column sums of dP over the windows ReLU did not block.  Workspace as for lr_conv3d_wgrad. */
int lr_conv3d_wgrad_pooled_supported(int Hin, int Win, int Cin_pad, int Cin_real, int Cout, int KT, int KH,
                                     int KW, int stride, int pt, int ph, int pw);
/* The same answer for a given frame count B * T: 0 where lr_conv3d_wgrad_pooled would return LR_ERR_UNSUPPORTED for it
 * (the stride-1 layers' kernel keeps a tile table in LDS that has to fit). */
int lr_conv3d_wgrad_pooled_supported_frames(int frames, int Hin, int Win, int Cin_pad, int Cin_real, int Cout, int KT,
                                            int KH, int KW, int stride, int pt, int ph, int pw);
int lr_conv3d_wgrad_pooled(const void* X, const void* pooled, const void* code, const void* dP, float* dW,
                           float* dbias, void* workspace, size_t workspace_bytes, int accumulate, int B, int T,
                           int Hin, int Win, int Cin_pad, int Cin_real, int Cout, int KT, int KH, int KW,
                           int stride, int pt, int ph, int pw, int flags, lr_stream_t stream);

/* MaxPool3d((1,2,2)) on channels-last bf16, and the backward of ReLU -> that pool: the gradient of
 * a window goes to its FIRST maximum (row-major, torch's rule) if the activation there is > 0.   */
int lr_maxpool_hw2_bf16(const void* in, void* out, int64_t frames, int H, int W, int C,
                        lr_stream_t stream);
/* dbias (may be NULL) receives the layer's bias gradient sum_pos dZ[pos][n] (fp32 [C]; added to
 * when accumulate != 0), computed in the same pass; it needs lr_unpool_workspace_bytes(C) bytes. */
size_t lr_unpool_workspace_bytes(int C);
int lr_unpool_relu_mask_bf16(const void* act, const void* dP, void* dZ, float* dbias, int accumulate,
                             void* workspace, size_t workspace_bytes, int64_t frames, int H, int W, int C,
                             lr_stream_t stream);
/* the same from the pooled activation and the window codes of lr_conv3d_forward_pooled (H, W: the
 * UN-pooled extent of dZ) */
int lr_unpool_code_bf16(const void* pooled, const void* code, const void* dP, void* dZ, float* dbias,
                        int accumulate, void* workspace, size_t workspace_bytes, int64_t frames, int H, int W,
                        int C, lr_stream_t stream);
int lr_bf16_to_f32(const void* in, float* out, int64_t n, lr_stream_t stream);
int lr_f32_to_bf16(const float* in, void* out, int64_t n, lr_stream_t stream);

/* ---- A8 sessions (BUILD-DEFINED, no reference symbol): the conv frontend fed chunk by chunk ---------------------- */
/* A frontend session is one device buffer owned by the caller: for B independent slots the last two input frames of
 * each of the three convolutions and the slot's counters (lipreading_amd/csrc/lr_conv_stream.hip).
 * Every layer has KT = 3, pt = 1, so feature frame t depends on clip frames t-3 .. t+3: a session has an inherent
 * look-ahead of 3 frames.  A slot's features are the one-shot frontend's on that slot's frames ALONE, zero temporal
 * padding before frame 0 and after the last frame; fed the same frames in any chunks, in any slot of any batch, a
 * session computes the same bits and leaves the same state bytes.  (The one-shot frontend on a PADDED batch lets the
 * padding frames reach the last two feature frames of a shorter clip; a session has no padding to see.  The two agree
 * on unpadded clips.)  Arithmetic as the one-shot path: byte * (1.f/255.f) rounded to bf16, bf16 operands, fp32
 * accumulation, bias -> bf16 -> ReLU -> 2x2 max-pool on the values that would be stored, bf16 at every level.
 * With H % 16 == 0, W % 16 == 0, a256(n) = n rounded up to a multiple of 256, plane(h, w, c) = a256(2 * h * w * c):
 *   state     a256(32 * B) bytes of slot headers (int32: magic, H, W, frames consumed n — saturating —, features
 *             emitted, ended, status bits, 0), then per slot 2 * (plane(H, W, 4) + plane(H/4, W/4, 32) +
 *             plane(H/8, W/8, 64)) bytes: a ring of TWO bf16 frames [h][w][c] for the input of layer 1 (the ingested
 *             clip), of layer 2 (pooled layer-1 output) and of layer 3 (pooled layer-2 output), older frame first
 *   workspace a256(48 * B) + a256(48 * B * (chunk_T + 3)) bytes of plan, then B * chunk_T * plane(H, W, 4) +
 *             B * (chunk_T + 1) * plane(H/4, W/4, 32) + B * (chunk_T + 2) * plane(H/8, W/8, 64) bytes of new frames
 * Limits: 16 <= H, W <= 1024, B * (chunk_T + 3) <= 65535 (else 0 bytes / LR_ERR_UNSUPPORTED).  NULLs, negative sizes,
 * H % 16 or W % 16, misaligned buffers answer LR_ERR_INVALID_ARG, buffers smaller than their *_bytes LR_ERR_WORKSPACE,
 * before any launch.  state, workspace and the weight operands must be 16-byte aligned. */
#define LR_CONV_STREAM_MISMATCH 1  /* a call's H or W is not the slot's */
#define LR_CONV_STREAM_AFTER_END 2 /* frames were given to a slot whose stream had ended */
#define LR_CONV_STREAM_F32 1       /* advance flags: x is fp32 (else uint8) */

size_t lr_conv_stream_state_bytes(int B, int H, int W);                     /* 0 for arguments it rejects */
size_t lr_conv_stream_workspace_bytes(int B, int chunk_T, int H, int W);    /* 0 for arguments it rejects */

/* Slots with mask[b] != 0 (mask [B] int32 on the device; NULL: all) go back to zero rings, 0 frames, not ended and
 * no status bit; the others keep every bit.  Under a mask the slot must already carry (H, W) (else it is left alone
 * and gets LR_CONV_STREAM_MISMATCH); with NULL whatever the buffer held is overwritten. */
int lr_conv_stream_reset(void* state, size_t state_bytes, const int32_t* mask, int B, int H, int W, lr_stream_t stream);

/* Slot b consumes frames [0, clamp(sizes[b], 0, chunk_T)) of x[b] (x + b * stride_b + t * stride_t in elements, then
 * (3, H, W) contiguous; uint8, or fp32 with LR_CONV_STREAM_F32 in flags; sizes NULL = chunk_T; 0: the slot is idle
 * and keeps every bit).  end [B] int32 or NULL: non-zero = the slot's stream ends with this call's frames.
 * w1 / w2 / w3: the layers' bf16 operands [Cout][taps][Cin_pad] of lr_conv3d_pack_weights (dgrad 0), packed once per
 * weight set; bias1 / bias2 / bias3 fp32.  feat fp32 [B][rows][96 * (H/16) * (W/16)] with rows = chunk_T + (end ? 3 :
 * 0), (h, w, c) order: the slot's newly completed feature frames packed from row 0, zero rows at and past counts[b].
 * With E(n, ended) = ended ? n : max(0, n - 3): counts[b] = E(after) - E(before).  chunk_T == 0 without end does
 * nothing; with end it is a flush.  An ended slot given frames keeps its bytes and gets LR_CONV_STREAM_AFTER_END; a slot
 * whose header is not (H, W) keeps its bytes and gets LR_CONV_STREAM_MISMATCH; both bits stay until a reset.
 * One plan launch, one ingest launch, three conv launches, two commit launches. */
int lr_conv_stream_advance(const void* x, int flags, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                           const int32_t* end, const void* w1, const void* w2, const void* w3, const float* bias1,
                           const float* bias2, const float* bias3, float* feat, int32_t* counts, void* state,
                           size_t state_bytes, void* workspace, size_t workspace_bytes, int B, int chunk_T, int H, int W,
                           lr_stream_t stream);

/* frames consumed, features emitted, ended, status, each [B] int32 on the device (each may be NULL, not all): what
 * the slots hold, without changing a byte of the state.  A slot whose header is not (H, W) reads as zeros with
 * LR_CONV_STREAM_MISMATCH in status[b]. */
int lr_conv_stream_read(const void* state, size_t state_bytes, int32_t* frames, int32_t* emitted, int32_t* ended,
                        int32_t* status, int B, int H, int W, lr_stream_t stream);

/* Inter-layer dropout of nn.GRU / nn.LSTM(dropout = p) in training mode (better_model.py:47-49 hands rnn_dropout to
 * torch; every shipped config sets 0): mask[i] = 0 with probability p, else 1 / (1 - p) (Philox4x32-10, key = seed,
 * counter = i / 4: the same mask for a (seed, n) whatever the launch geometry), y = x * mask (x == y == NULL: only
 * the mask is written — the decoder loop applies it inside its own kernels).  Backward: dx = dy * mask
 * (lr_mul_f32).  lr_cat_directions: (D, B, H) -> (B, D*H), forward direction first (better_model.py:98-112
 * _cat_directions), for one or two tensors (h, c) in one launch; inverse != 0: the way back (its gradient). */
int lr_dropout_forward(const float* x, float* y, float* mask, int64_t n, float p, uint64_t seed, lr_stream_t stream);
int lr_mul_f32(const float* a, const float* b, float* out, int64_t n, lr_stream_t stream);
int lr_cat_directions(const float* in0, float* out0, const float* in1, float* out1, int B, int H, int D, int inverse,
                      lr_stream_t stream);

/* ---- A5 tail: optimiser side of the reference step — train_better_model.py:78-80 -------- */

/* sum of squares of n floats accumulated into out[0] (caller zeroes it); used for
 * clip_grad_norm_ (train_better_model.py:78) over a flat gradient buffer. */
int lr_sumsq(const float* x, int64_t n, float* out, lr_stream_t stream);

/* Fused clip + Adam step over a flat parameter buffer (torch.optim.Adam defaults as used at
 * src/scripts/train.py:280: betas (0.9,0.999), eps 1e-8, no weight decay, no amsgrad).
 *   grad_scale multiplies the gradient first (1/world_size after an all-reduce sum);
 *   max_norm > 0 applies clip_grad_norm_ (train_better_model.py:78) with the total norm taken
 *   from sumsq[0] (lr_sumsq over the same gradient buffer): coef = min(1, max_norm/(norm+1e-6)).
 *   step_count  [2] int32 DEVICE counters: [0] updates taken, incremented here (bias correction uses the new
 *               value), so a captured hipGraph replays correct corrections; [1] steps skipped (skip != 0 or a
 *               pending recurrence fault), so the caller can report them without a per-step host read;
 *   skip        [1] int32 DEVICE flag or NULL: non-zero = the reference skipped this batch
 *               (`continue`, train_better_model.py:49-50): nothing is updated, step_count stays;
 *   scratch     [4] floats of device scratch;
 *   dist_words  NULL, or (data parallel) the two summed words of lr_fault_export_f32 with `world` = the number of
 *               ranks: they then decide skip / fault instead of `skip` (a local fault still counts), and skip[0]
 *               is overwritten with the ranks' verdict (1 = every rank skipped the batch, else 0). */
int lr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                 const float* sumsq, float max_norm, float grad_scale, float lr, float beta1,
                 float beta2, float eps, int32_t* step_count, int32_t* skip, float* scratch,
                 const float* dist_words, float world, lr_stream_t stream);
/* lr_sumsq + lr_adam_step with max_norm > 0 in TWO launches instead of three: the sum-of-squares kernel's last workgroup
 * (a ticket in sumsq[1]) derives the step's coefficients.  sumsq [2]: {accumulator, ticket}, both zero before the first
 * call and put back to zero by every call (lr_step_begin's also_zero clears them as well: a launch that was torn down
 * half-way leaves nothing behind); scratch8: EIGHT floats of device scratch: [0..3] the step's coefficients, [5] the sum
 * of squares of this step; n_sumsq (<= n): the sum of squares is taken over grad[0 .. n_sumsq) only — the rest of the
 * buffer's was added to sumsq[0] by lr_sumsq calls earlier in the step (FusedAdam.sum_squares_early: the encoder's share,
 * beside the conv backward); n_sumsq = n: over everything; everything else as lr_adam_step. */
int lr_clip_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* sumsq,
                      float max_norm, float grad_scale, float lr, float beta1, float beta2, float eps,
                      int32_t* step_count, int32_t* skip, float* scratch8, const float* dist_words, float world,
                      int64_t n_sumsq, lr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LIPREADING_HIP_H */
