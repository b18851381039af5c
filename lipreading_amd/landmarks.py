"""Landmark step on the device — the arithmetic of `src/utils/data/face.py` and
`src/models/face/prnet.py` that surrounds the two networks (dlib detector, PRNet) between a video
frame and the dataview's `face_lmk_seq` rows:

  `_applyPadding` face.py:76-90 · PRNet crop geometry prnet.py:112-119,136-140 · restore
  prnet.py:150-156 · `get_landmarks` prnet.py:162-170 · `getFace` face.py:164-175,
  composed as `_gen_data` does (generate_dataview.py:58-64: the UNPADDED rect defines the crop, the
  PADDED one the translation).

The reference does this per frame in NumPy inside the offline ETL; here whole clips go through one
launch so the step can sit in front of the encoder on the GPU.  dlib / PRNet inference itself is out
of scope (third-party nets, weights not shipped): `landmark_step` takes the network's position maps.
"""
import ctypes

import numpy as np
import torch

from . import _C
from ._host import PerDevice

_mouth = slice(48, 68)  # face.py:21 (defined, unused by the reference as well)


def apply_padding(dims, rects, padding):
  """Batched `_applyPadding` (face.py:76-90).

  dims (n,2|3) int = (img_h, img_w[, c]); rects (n,4) int = (left,right,top,bottom) ->
  padded rects (n,4) int32 on the device.  Integer arithmetic is the reference's:
  int(padding * box_w) truncates toward zero, then clamps to the image."""
  _C.require_cuda(rects, dims)
  assert dims.shape[-1] in (2, 3) and rects.shape[-1] == 4
  n = rects.shape[0]
  r = rects.to(torch.int32).contiguous()
  d = dims[:, :2].to(torch.int32).contiguous()
  out = torch.empty_like(r)
  _C.check(_C.lib().lr_lmk_apply_padding(r.data_ptr(), d.data_ptr(), out.data_ptr(), n,
                                         float(padding), _C.stream_handle()), "lr_lmk_apply_padding")
  return out


def get_face(lmks, rects):
  """Batched `getFace` (face.py:164-175): x -= left, y -= top, z untouched.

  lmks (n,P,3) float; rects (n,4) int (left,right,top,bottom) -> (n,P,3) float32."""
  _C.require_cuda(lmks, rects)
  assert lmks.dim() == 3 and lmks.shape[2] == 3
  assert rects.dim() == 2 and rects.shape[1] == 4 and rects.shape[0] == lmks.shape[0]
  x = lmks.to(torch.float32).contiguous()
  r = rects.to(torch.int32).contiguous()
  out = torch.empty_like(x)
  _C.check(_C.lib().lr_lmk_translate(x.data_ptr(), r.data_ptr(), out.data_ptr(), x.shape[0],
                                     x.shape[1], _C.stream_handle()), "lr_lmk_translate")
  return out


def crop_transform(rects, resolution=256):
  """PRNet crop geometry (prnet.py:112-119,136-140) for n face rects (left,right,top,bottom):
  -> (tform (n,3,3) float64 — what `estimate_transform('similarity', src_pts, DST_PTS).params` is in
  the reference — and the crop side `size` (n,) int32)."""
  _C.require_cuda(rects)
  assert rects.dim() == 2 and rects.shape[1] == 4
  r = rects.to(torch.int32).contiguous()
  n = r.shape[0]
  tform = torch.empty((n, 3, 3), dtype=torch.float64, device=r.device)
  sizes = torch.empty((n,), dtype=torch.int32, device=r.device)
  _C.check(_C.lib().lr_lmk_crop_transform(r.data_ptr(), tform.data_ptr(), sizes.data_ptr(), n, int(resolution),
                                          _C.stream_handle()), "lr_lmk_crop_transform")
  return tform, sizes


def restore(cropped_pos, tform):
  """prnet.py:150-156: position maps of the crops (n,res,res,3) float32 + tform (n,3,3) float64 ->
  position maps in image coordinates (n,res,res,3) float64."""
  _C.require_cuda(cropped_pos, tform)
  assert cropped_pos.dim() == 4 and cropped_pos.shape[3] == 3 and tform.shape == (cropped_pos.shape[0], 3, 3)
  cp = cropped_pos.to(torch.float32).contiguous()
  tf = tform.to(torch.float64).contiguous()
  pos = torch.empty(cp.shape, dtype=torch.float64, device=cp.device)
  n = cp.shape[0]
  _C.check(_C.lib().lr_lmk_restore(cp.data_ptr(), tf.data_ptr(), pos.data_ptr(), n, cp.shape[1] * cp.shape[2],
                                   _C.stream_handle()), "lr_lmk_restore")
  return pos


def get_landmarks(pos, uv_kpt_ind, rects=None):
  """prnet.py:162-170: kpt = pos[uv_kpt_ind[1], uv_kpt_ind[0], :] for n position maps (n,res,res,3)
  float64 -> (n,K,3) float64; with `rects` also getFace's translation (face.py:164-175)."""
  _C.require_cuda(pos, uv_kpt_ind, rects)
  assert pos.dim() == 4 and pos.shape[1] == pos.shape[2] and pos.shape[3] == 3 and uv_kpt_ind.shape[0] == 2
  p = pos.to(torch.float64).contiguous()
  uv = uv_kpt_ind.to(torch.int32).contiguous()
  r = None if rects is None else rects.to(torch.int32).contiguous()
  n, K = p.shape[0], uv.shape[1]
  out = torch.empty((n, K, 3), dtype=torch.float64, device=p.device)
  _C.check(_C.lib().lr_lmk_gather(p.data_ptr(), uv.data_ptr(), _C.ptr(r), out.data_ptr(), n, p.shape[1], K,
                                  _C.stream_handle()), "lr_lmk_gather")
  return out


def landmark_step(cropped_pos, rects, dims, uv_kpt_ind, padding=0.3, dtype=torch.float64):
  """`_gen_data` (generate_dataview.py:58-64) around the networks, one launch for n frames:
  cropped_pos (n,res,res,3) float32 = PRNet's output for the crop of each frame, rects (n,4) the
  detector's UNPADDED face rects, dims (n,2|3) = (img_h, img_w[, c]) -> (face landmarks (n,K,3)
  relative to the padded rect — a `face_lmk_seq` row per frame; float64 as the reference stores them,
  or float32 as the encoder consumes them — and the padded rects (n,4) int32)."""
  _C.require_cuda(cropped_pos, rects, dims, uv_kpt_ind)
  assert cropped_pos.dim() == 4 and cropped_pos.shape[1] == cropped_pos.shape[2] and cropped_pos.shape[3] == 3
  assert dtype in (torch.float64, torch.float32)
  cp = cropped_pos.to(torch.float32).contiguous()
  r = rects.to(torch.int32).contiguous()
  d = dims[:, :2].to(torch.int32).contiguous()
  uv = uv_kpt_ind.to(torch.int32).contiguous()
  n, K = cp.shape[0], uv.shape[1]
  out = torch.empty((n, K, 3), dtype=dtype, device=cp.device)
  padded = torch.empty((n, 4), dtype=torch.int32, device=cp.device)
  f64 = out.data_ptr() if dtype == torch.float64 else None
  f32 = out.data_ptr() if dtype == torch.float32 else None
  _C.check(_C.lib().lr_lmk_landmarks(cp.data_ptr(), r.data_ptr(), d.data_ptr(), float(padding), uv.data_ptr(), f64, f32,
                                     padded.data_ptr(), n, cp.shape[1], K, _C.stream_handle()), "lr_lmk_landmarks")
  return out, padded


def lip_crop(frames, lmks, size=96, margin=0.3, mouth=_mouth):
  """BUILD-DEFINED (the reference never crops the mouth, face.py:21 is unused):
  frames (n,3,H,W) uint8 + landmarks (n,68,3) in image pixels -> (n,3,size,size) uint8 mouth crops:
  bounding box of landmarks `mouth` -> square window of side max(w,h)*(1+2*margin) about its centre
  -> bilinear resize (half-pixel centres, edge clamping), rounded to nearest."""
  _C.require_cuda(frames, lmks)
  assert frames.dim() == 4 and frames.shape[1] == 3 and frames.dtype == torch.uint8
  assert lmks.dim() == 3 and lmks.shape[2] == 3 and lmks.shape[0] == frames.shape[0]
  f = frames.contiguous()
  l = lmks.to(torch.float32).contiguous()
  n, _, H, W = f.shape
  out = torch.empty((n, 3, size, size), dtype=torch.uint8, device=f.device)
  _C.check(_C.lib().lr_lip_crop_u8(f.data_ptr(), l.data_ptr(), out.data_ptr(), n, H, W, size, l.shape[1],
                                   mouth.start, mouth.stop, float(margin), _C.stream_handle()),
           "lr_lip_crop_u8")
  return out


_eyes = (slice(36, 42), slice(42, 48))  # the 68-point scheme's two eye contours


def stable_crop_collate(frames, lmks, offsets, lens, t_max, size, extent, radius, clip_aug=None, tmap=None,
                        mouth=_mouth, eyes=_eyes, pose=None, workspace=None):
  """lr_lip_stable_collate_u8 on device tensors: ragged frames u8 (rows,3,H,W), landmarks f32 (rows,npts,3), offsets
  i64 (B,), lens i32 (B,) -> the padded batch u8 (B,t_max,3,size,size) in ONE call.  clip_aug f32 (B,4) and tmap i32
  (rows,): both or neither.  pose: an f32 (rows,4) tensor to receive the smoothed poses.  workspace: a u8 tensor of
  lr_lip_stable_workspace_bytes(rows, radius) bytes (allocated when None)."""
  L = _C.lib()
  rows, _, H, W = frames.shape
  B = offsets.shape[0]
  need = L.lr_lip_stable_workspace_bytes(rows, int(radius))
  if workspace is None:
    workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=frames.device)
  out = torch.empty((B, int(t_max), 3, size, size), dtype=torch.uint8, device=frames.device)
  _C.check(L.lr_lip_stable_collate_u8(frames.data_ptr(), lmks.data_ptr(), offsets.data_ptr(), lens.data_ptr(),
                                      _C.ptr(clip_aug), _C.ptr(tmap), out.data_ptr(), _C.ptr(pose),
                                      workspace.data_ptr(), workspace.numel(), B, rows, int(t_max), H, W, int(size),
                                      lmks.shape[1], mouth.start, mouth.stop, eyes[0].start, eyes[0].stop,
                                      eyes[1].start, eyes[1].stop, float(extent), int(radius), _C.stream_handle()),
           "lr_lip_stable_collate_u8")
  return out


def lip_crop_stable(frames, lmks, size=96, extent=1.25, radius=2, mouth=_mouth, eyes=_eyes, return_pose=False):
  """BUILD-DEFINED, the stabilised counterpart of `lip_crop` (include/lipreading_hip.h, "A9, stabilised"): the n rows
  are ONE clip.  The window's centre is the mean of landmarks `mouth`, its side `extent` times the distance between
  the means of the two `eyes` ranges, its axes follow the line between them (roll correction), and all of it is
  averaged over the 2*radius+1 neighbouring frames.  frames (n,3,H,W) uint8 + landmarks (n,68,3) in image pixels ->
  (n,3,size,size) uint8; with return_pose also the smoothed pose (n,4) float32 = (mx, my, ax, ay)."""
  _C.require_cuda(frames, lmks)
  assert frames.dim() == 4 and frames.shape[1] == 3 and frames.dtype == torch.uint8
  assert lmks.dim() == 3 and lmks.shape[2] == 3 and lmks.shape[0] == frames.shape[0]
  f = frames.contiguous()
  l = lmks.to(torch.float32).contiguous()
  n = f.shape[0]
  offsets = torch.zeros(1, dtype=torch.int64, device=f.device)
  lens = torch.full((1,), n, dtype=torch.int32, device=f.device)
  pose = torch.empty((n, 4), dtype=torch.float32, device=f.device) if return_pose else None
  with torch.cuda.device(f.device):
    out = stable_crop_collate(f, l, offsets, lens, n, size, extent, radius, mouth=mouth, eyes=eyes, pose=pose)[0]
  return (out, pose) if return_pose else out


# ---- head-pose normalisation (include/lipreading_hip.h, "Landmark pose") ------------------------------
RIGID_68 = (27, 28, 29, 30, 33, 36, 39, 42, 45)   # nose bridge, nose base and the four eye corners


class PoseSpec(object):
  """What lr_lmk_pose_collate_f32 aligns to and how: the canonical face `template` (npts, 3), the indices `rigid` of
  the points the alignment is estimated from, the half-width `radius` of the smoothing window (frames either side) and
  `scale` (True: similarity, False: rigid).  Validated on the host: a ValueError carries the offending value.  The
  template is uploaded once per device."""

  def __init__(self, template, rigid=RIGID_68, radius=0, scale=True):
    t = np.array(template.detach().cpu().numpy() if torch.is_tensor(template) else template, dtype=np.float32)
    if t.ndim != 2 or t.shape[1] != 3 or not 1 <= t.shape[0] <= _C.LR_POSE_MAX_POINTS:
      raise ValueError("template must be (npts, 3) with 1 <= npts <= %d, got shape %r"
                       % (_C.LR_POSE_MAX_POINTS, tuple(t.shape)))
    if not np.isfinite(t).all():
      raise ValueError("template has a non-finite coordinate at point %d" % int(np.argwhere(~np.isfinite(t))[0][0]))
    try:
      rigid = tuple(int(i) for i in rigid)
    except (TypeError, ValueError):
      raise ValueError("rigid must be a sequence of point indices, got %r" % (rigid,))
    if not 3 <= len(rigid) <= _C.LR_POSE_MAX_RIGID:
      raise ValueError("rigid must name 3 .. %d points, got %d" % (_C.LR_POSE_MAX_RIGID, len(rigid)))
    for i in rigid:
      if not 0 <= i < t.shape[0]:
        raise ValueError("rigid index %d is outside [0, %d)" % (i, t.shape[0]))
      if rigid.count(i) > 1:
        raise ValueError("rigid index %d is repeated" % i)
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= _C.LR_POSE_MAX_RADIUS:
      raise ValueError("radius must be an integer in [0, %d], got %r" % (_C.LR_POSE_MAX_RADIUS, radius))
    t.setflags(write=False)
    self.template, self.npts, self.rigid, self.radius, self.scale = t, int(t.shape[0]), rigid, radius, bool(scale)
    self.flags = _C.LR_POSE_SCALE if self.scale else 0
    self._rigid_c = (ctypes.c_int32 * len(rigid))(*rigid)     # the HOST array the entry reads
    self.rigid_ptr = ctypes.addressof(self._rigid_c)
    self._dev = PerDevice()

  def template_on(self, dev):
    return self._dev.get(dev, lambda d: torch.from_numpy(self.template.copy()).to(d))

  def workspace_bytes(self, rows):
    return int(_C.lib().lr_lmk_pose_workspace_bytes(int(rows), len(self.rigid), self.radius))

  def __repr__(self):
    return "PoseSpec(npts=%d, rigid=%r, radius=%d, scale=%r)" % (self.npts, self.rigid, self.radius, self.scale)


def pose_collate(lmks, offsets, lens, t_max, spec, tmap=None, return_pose=False, workspace=None):
  """lr_lmk_pose_collate_f32 on device tensors, the twin of `stable_crop_collate`: ragged landmarks f32 (rows,npts,3),
  offsets i64 (B,), lens i32 (B,) -> the padded, pose-normalised batch f32 (B,t_max,npts,3) in ONE call.  tmap i32
  (rows,) or None (identity).  return_pose: also pose f32 (rows,13) = (R row-major, s, centroid) and status i32 (rows,)
  of every row.  workspace: a u8 tensor of spec.workspace_bytes(rows) bytes (allocated when None)."""
  _C.require_cuda(lmks, offsets, lens, tmap)
  L = _C.lib()
  if lmks.dim() != 3 or tuple(lmks.shape[1:]) != (spec.npts, 3) or lmks.dtype != torch.float32:
    raise ValueError("landmarks must be float32 (rows, %d, 3), got %s %r" % (spec.npts, lmks.dtype, tuple(lmks.shape)))
  assert lmks.is_contiguous() and offsets.dtype == torch.int64 and lens.dtype == torch.int32
  assert tmap is None or (tmap.dtype == torch.int32 and tmap.shape == (lmks.shape[0],))
  rows, B, dev = lmks.shape[0], offsets.shape[0], lmks.device
  if workspace is None:
    workspace = torch.empty(max(spec.workspace_bytes(rows), 16), dtype=torch.uint8, device=dev)
  out = torch.empty((B, int(t_max), spec.npts, 3), dtype=torch.float32, device=dev)
  status = torch.empty((rows,), dtype=torch.int32, device=dev)
  pose = torch.empty((rows, 13), dtype=torch.float32, device=dev) if return_pose else None
  _C.check(L.lr_lmk_pose_collate_f32(lmks.data_ptr(), offsets.data_ptr(), lens.data_ptr(), _C.ptr(tmap),
                                     spec.template_on(dev).data_ptr(), spec.rigid_ptr, len(spec.rigid), out.data_ptr(),
                                     _C.ptr(pose), status.data_ptr(), workspace.data_ptr(), workspace.numel(), B, rows,
                                     int(t_max), spec.npts, spec.radius, spec.flags, _C.stream_handle()),
           "lr_lmk_pose_collate_f32")
  return (out, pose, status) if return_pose else out


def normalise_pose(lmks, spec, return_pose=False):
  """One clip: landmarks (n,npts,3) on the device -> the clip aligned to spec.template, f32 (n,npts,3); with
  return_pose also pose (n,13) and status (n,) (see `pose_collate`)."""
  _C.require_cuda(lmks)
  if lmks.dim() != 3 or lmks.shape[0] < 1:
    raise ValueError("a clip is (n >= 1, npts, 3), got %r" % (tuple(lmks.shape),))
  l = lmks.to(torch.float32).contiguous()
  n = l.shape[0]
  offsets = torch.zeros(1, dtype=torch.int64, device=l.device)
  lens = torch.full((1,), n, dtype=torch.int32, device=l.device)
  with torch.cuda.device(l.device):
    got = pose_collate(l, offsets, lens, n, spec, return_pose=return_pose)
  return (got[0][0], got[1], got[2]) if return_pose else got[0]


# ---- landmark-space augmentation (include/lipreading_hip.h, "Landmark augmentation") ------------------
def _mirror_68():
  """The iBUG 68-point scheme's left/right partners: jaw 0..16 <-> 16..0, brows 17..21 <-> 26..22, nostrils
  31..35 <-> 35..31, the eyes and the mouth contour by contour; the points on the face's midline are their own."""
  pairs = [(i, 16 - i) for i in range(8)] + [(17 + i, 26 - i) for i in range(5)] + [(31, 35), (32, 34)]
  pairs += [(36, 45), (37, 44), (38, 43), (39, 42), (40, 47), (41, 46)]
  pairs += [(48, 54), (49, 53), (50, 52), (55, 59), (56, 58), (60, 64), (61, 63), (65, 67)]
  perm = list(range(68))
  for a, b in pairs:
    perm[a], perm[b] = b, a
  return tuple(perm)


MIRROR_68 = _mirror_68()
_perm_on = {}                                 # perm -> PerDevice: a permutation is uploaded once per device


def check_mirror_perm(perm, npts):
  """perm as a tuple of ints; ValueError unless it is an involution of range(npts)."""
  try:
    perm = tuple(int(i) for i in perm)
  except (TypeError, ValueError):
    raise ValueError("perm must be a sequence of point indices, got %r" % (perm,))
  if len(perm) != npts:
    raise ValueError("perm names the partner of each of the %d points, got %d entries" % (npts, len(perm)))
  for j, p in enumerate(perm):
    if not 0 <= p < npts:
      raise ValueError("perm[%d] = %d is outside [0, %d)" % (j, p, npts))
    if perm[p] != j:
      raise ValueError("perm is not an involution: perm[%d] = %d but perm[%d] = %d" % (j, p, p, perm[p]))
  return perm


def mirror_perm_on(perm, dev):
  """The int32 device copy of a (validated) permutation, made once per device."""
  per = _perm_on.setdefault(perm, PerDevice())
  return per.get(dev, lambda d: torch.tensor(perm, dtype=torch.int32).to(d))


def augment_landmarks(batch, lens, rec, perm=MIRROR_68, out=None, return_stats=False):
  """lr_lmk_augment_f32 on device tensors: a COLLATED batch f32 (B,t_max,npts,3), lens int32 or int64 (B,) on the
  device, rec = augment.LandmarkAugmentSpec.draw's records — uint64 numpy (B,16), or a device tensor of (B,16)
  eight-byte elements — -> the augmented batch f32 (B,t_max,npts,3).  out: the tensor to write (`batch` itself: in
  place; otherwise it must not share memory with it); None: a new one.  perm: the left/right partner of every point,
  an involution of range(npts).  return_stats: also the clips' (c_x, c_y, c_z, r) as f64 (B,4)."""
  _C.require_cuda(batch, lens, out)
  if batch.dim() != 4 or batch.shape[3] != 3 or batch.dtype != torch.float32 or not batch.is_contiguous():
    raise ValueError("a collated batch is contiguous float32 (B, t_max, npts, 3), got %s %r"
                     % (batch.dtype, tuple(batch.shape)))
  B, t_max, npts = int(batch.shape[0]), int(batch.shape[1]), int(batch.shape[2])
  if B < 1 or t_max < 1 or not 1 <= npts <= _C.LR_LMK_AUG_MAX_POINTS:
    raise ValueError("B and t_max must be positive and 1 <= npts <= %d, got %r"
                     % (_C.LR_LMK_AUG_MAX_POINTS, tuple(batch.shape)))
  if lens.dtype not in (torch.int32, torch.int64) or tuple(lens.shape) != (B,):
    raise ValueError("lens must be int32 or int64 (%d,), got %s %r" % (B, lens.dtype, tuple(lens.shape)))
  perm = check_mirror_perm(perm, npts)
  dev = batch.device
  if isinstance(rec, np.ndarray):
    if rec.dtype != np.uint64 or rec.shape != (B, _C.LR_LMK_AUG_REC_WORDS):
      raise ValueError("rec must be uint64 (%d, %d), got %s %r" % (B, _C.LR_LMK_AUG_REC_WORDS, rec.dtype, rec.shape))
    rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int64)).to(dev)
  else:
    _C.require_cuda(rec)
    if rec.element_size() != 8 or tuple(rec.shape) != (B, _C.LR_LMK_AUG_REC_WORDS) or not rec.is_contiguous():
      raise ValueError("rec must be (%d, %d) contiguous eight-byte words, got %s %r"
                       % (B, _C.LR_LMK_AUG_REC_WORDS, rec.dtype, tuple(rec.shape)))
  if out is None:
    out = torch.empty_like(batch)
  elif out.shape != batch.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
    raise ValueError("out must be contiguous float32 %r on %s, got %s %r on %s"
                     % (tuple(batch.shape), dev, out.dtype, tuple(out.shape), out.device))
  L = _C.lib()
  with torch.cuda.device(dev):
    lens32 = lens.to(torch.int32).contiguous()
    need = int(L.lr_lmk_augment_workspace_bytes(B))
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    stats = torch.empty((B, 4), dtype=torch.float64, device=dev) if return_stats else None
    _C.check(L.lr_lmk_augment_f32(batch.data_ptr(), lens32.data_ptr(), rec.data_ptr(),
                                  mirror_perm_on(perm, dev).data_ptr(), out.data_ptr(), _C.ptr(stats), work.data_ptr(),
                                  need, B, t_max, npts, _C.stream_handle()), "lr_lmk_augment_f32")
  return (out, stats) if return_stats else out


def canonical_orientation(points):
  """The host half of `fit_template`, float64: (68,3) points -> the same points about their origin in the face's own
  axes.  x runs along the mean of points 42..47 minus the mean of points 36..41 (eye to eye), y from the eyes' midpoint
  to the mean of points 48..67 (the mouth), orthogonalised against x, z = x × y.  ValueError when the three anchor
  means are collinear (or coincide)."""
  p = np.asarray(points, dtype=np.float64)
  if p.shape != (68, 3):
    raise ValueError("the orientation is defined on the 68-point scheme, got shape %r" % (tuple(p.shape),))
  eye_a, eye_b, mouth = p[36:42].mean(axis=0), p[42:48].mean(axis=0), p[48:68].mean(axis=0)
  x = eye_b - eye_a
  y = mouth - 0.5 * (eye_a + eye_b)
  nx, ny = np.linalg.norm(x), np.linalg.norm(y)
  if not (nx > 0 and ny > 0):
    raise ValueError("the eye and mouth anchor means coincide: %r %r %r" % (eye_a, eye_b, mouth))
  x = x / nx
  y = y - (y @ x) * x
  if not np.linalg.norm(y) > 1e-9 * ny:
    raise ValueError("the eye and mouth anchor means are collinear: %r %r %r" % (eye_a, eye_b, mouth))
  y = y / np.linalg.norm(y)
  z = np.cross(x, y)
  return p @ np.stack([x, y, z], axis=1)


def _rigid_frame(points, rigid):
  """points (..., npts, 3) float64 -> (points about their rigid centroid, the rigid RMS radius)."""
  c = points[..., list(rigid), :].mean(axis=-2, keepdims=True)
  d = points - c
  return d, np.sqrt((d[..., list(rigid), :] ** 2).sum(axis=-1).mean(axis=-1))


def fit_template(clips, rigid=RIGID_68, iters=3, max_frames=20000, device=None):
  """Generalised Procrustes on the device: the canonical face of a set of clips [(len_i,68,3)], as (68,3) float32.
  Start from the first frame about its rigid centroid; `iters` times align the first `max_frames` frames (dataset
  order) to the current template with `pose_collate` (radius 0, scale on), average in float64, re-centre on the rigid
  centroid and rescale so that the rigid RMS radius is the mean rigid RMS radius of the raw frames (magnitudes stay in
  the pixels range the reference feeds); then `canonical_orientation` on the host."""
  dev = torch.device("cuda" if device is None else device)
  if dev.type != "cuda":
    raise _C.LipReadingHipError("the template is fitted on the MI355X only (no CPU fallback)")
  if iters < 1 or max_frames < 1:
    raise ValueError("iters and max_frames must be positive, got %r and %r" % (iters, max_frames))
  rows, left = [], int(max_frames)
  for c in clips:
    if left <= 0:
      break
    a = np.asarray(c.detach().cpu().numpy() if torch.is_tensor(c) else c, dtype=np.float32)[:left]
    if a.ndim != 3 or a.shape[1:] != (68, 3):
      raise ValueError("a clip is (len, 68, 3), got shape %r" % (tuple(a.shape),))
    rows.append(a)
    left -= len(a)
  if not rows or not sum(len(a) for a in rows):
    raise ValueError("no frame to fit the template from")
  frames = np.ascontiguousarray(np.concatenate(rows))
  good = np.isfinite(frames).all(axis=(1, 2))
  if not good.any():
    raise ValueError("every frame has a non-finite coordinate")
  first = int(np.argmax(good))
  target = float(_rigid_frame(frames[good].astype(np.float64), rigid)[1].mean())
  tmpl = _rigid_frame(frames[first].astype(np.float64), rigid)[0]
  n = len(frames)
  with torch.cuda.device(dev):
    frames_d = torch.from_numpy(frames).to(dev)
    offsets = torch.zeros(1, dtype=torch.int64, device=dev)
    lens = torch.full((1,), n, dtype=torch.int32, device=dev)
    for _ in range(int(iters)):
      spec = PoseSpec(tmpl.astype(np.float32), rigid=rigid, radius=0, scale=True)
      out, _, status = pose_collate(frames_d, offsets, lens, n, spec, return_pose=True)
      keep = (status == _C.LR_POSE_OK).cpu().numpy()
      if not keep.any():
        raise ValueError("no frame could be aligned (the rigid points of every frame, or of the template, coincide)")
      mean = out[0].cpu().numpy()[keep].astype(np.float64).mean(axis=0)
      d, radius = _rigid_frame(mean, rigid)
      if not radius > 0:
        raise ValueError("the rigid points of the mean face coincide")
      tmpl = d * (target / radius)
  return canonical_orientation(tmpl).astype(np.float32)
