"""Shared by tests/test_stable_crop_cpu.py and tests/test_gpu_stable_crop.py: a numpy restatement of the stabilised crop
(lr_lip_stable_collate_u8; the specification is include/lipreading_hip.h, "A9, stabilised") and the batches both files
grade on.

The pose is float64 sums rounded once to float32, as specified; the tests keep every landmark's magnitude inside
[2^-10, 2^14] (or zero), where those sums are exact and the pose has ONE right answer, bit for bit.  From the pose on
the arithmetic is float32.  fused=True evaluates every a + b * c with ONE rounding, as the kernel's fmaf does (through
float64, where a product of two float32 is exact); fused=False rounds the product and the sum, in the manner of
tests/augment_cases.py.  The bilinear tail is oracle.torch_oracle.lip_crop's, with both source coordinates per pixel.
"""
import numpy as np

from tests import augment_cases as AC
from tests.augment_cases import _madd, f32, identity_records  # noqa: F401

MOUTH = (48, 68)
EYES = ((36, 42), (42, 48))
T_MAX = AC.T_MAX


def _mean(v):
  """float64 sum in ascending index / count, rounded once."""
  s = np.float64(0)
  for x in np.asarray(v, np.float32):
    s = s + np.float64(x)
  return f32(s / np.float64(len(v)))


def raw_pose(row, mouth=MOUTH, eyes=EYES):
  """One row of landmarks [npts][3] -> (mx, my, ax, ay) float32."""
  row = np.asarray(row, np.float32)
  (lo, hi), ((a0, a1), (b0, b1)) = mouth, eyes
  return np.array([_mean(row[lo:hi, 0]), _mean(row[lo:hi, 1]),
                   f32(_mean(row[b0:b1, 0]) - _mean(row[a0:a1, 0])),
                   f32(_mean(row[b0:b1, 1]) - _mean(row[a0:a1, 1]))], np.float32)


def smoothed_poses(lmk, offsets, lens, radius, mouth=MOUTH, eyes=EYES):
  """[rows][4] float32: every row's raw pose averaged over its neighbours within its own sample."""
  raw = np.stack([raw_pose(r, mouth, eyes) for r in lmk])
  out = np.zeros_like(raw)
  for b in range(len(lens)):
    first, n = int(offsets[b]), int(lens[b])
    for i in range(n):
      j0, j1 = max(0, i - radius), min(n - 1, i + radius)
      for c in range(4):
        out[first + i, c] = _mean(raw[first + j0:first + j1 + 1, c])
  return out


def window(pose, record, size, extent, fused=False):
  """(cx, cy, ux, uy) float32 of a smoothed pose and a record (dx, dy, zoom, flip)."""
  mx, my, ax, ay = (f32(v) for v in pose)
  dx, dy, zoom, _ = (f32(v) for v in record)
  extent, S = f32(extent), f32(size)
  with np.errstate(all="ignore"):
    d = np.sqrt(f32(_madd(f32(ax * ax), ay, ay, fused)))
    if not (f32(f32(extent * d) * zoom) >= f32(2)):
      ax, ay = f32(f32(2) / f32(extent * zoom)), f32(0)
    ex, ey = f32(extent * ax), f32(extent * ay)
    cx = f32(_madd(_madd(mx, dx, ex, fused), -dy, ey, fused))
    cy = f32(_madd(_madd(my, dx, ey, fused), dy, ex, fused))
    ux, uy = f32(f32(ex * zoom) / S), f32(f32(ey * zoom) / S)
  return cx, cy, ux, uy


def stable_crop(frame, pose, record, size=96, extent=1.25, fused=False):
  """One frame uint8 [3][H][W], the smoothed pose of its row and a record -> uint8 [3][size][size]."""
  frame = np.asarray(frame)
  _, H, W = frame.shape
  cx, cy, ux, uy = window(pose, record, size, extent, fused)
  p = (np.arange(size, dtype=np.float32) + f32(0.5)) - f32(0.5) * f32(size)
  px, py = p[None, :], p[:, None]                                       # [oy][ox]
  sx = (_madd(_madd(cx, px, ux, fused), -py, uy, fused) - f32(0.5)).astype(np.float32)
  sy = (_madd(_madd(cy, px, uy, fused), py, ux, fused) - f32(0.5)).astype(np.float32)
  sx = np.clip(sx, 0, W - 1).astype(np.float32)
  sy = np.clip(sy, 0, H - 1).astype(np.float32)
  ix, iy = np.floor(sx).astype(int), np.floor(sy).astype(int)
  ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
  fx, fy = (sx - ix).astype(np.float32), (sy - iy).astype(np.float32)
  img = frame.astype(np.float32)
  a, b = img[:, iy, ix], img[:, iy, ix1]
  d, e = img[:, iy1, ix], img[:, iy1, ix1]
  tv = _madd(a, b - a, fx[None], fused)
  bv = _madd(d, e - d, fx[None], fused)
  v = _madd(tv, bv - tv, fy[None], fused)
  out = np.clip(np.floor(v + f32(0.5)), 0, 255).astype(np.uint8)
  return out[:, :, ::-1] if f32(record[3]) != 0 else out


def stable_batch(frames, lmk, offsets, lens, clip, tmap, t_max, size, extent=1.25, radius=2, mouth=MOUTH, eyes=EYES,
                 fused=False, poses=None):
  """The whole padded batch uint8 [B][t_max][3][size][size] (clip / tmap None: the identity) and the smoothed poses
  [rows][4].  poses: smoothed_poses' result, if the caller has it."""
  B = len(lens)
  if clip is None:
    clip, tmap = identity_records(lens)
  if poses is None:
    poses = smoothed_poses(lmk, offsets, lens, radius, mouth, eyes)
  out = np.zeros((B, t_max, 3, size, size), np.uint8)
  for b in range(B):
    first, n = int(offsets[b]), int(lens[b])
    for t in range(min(n, t_max)):
      m = int(tmap[first + t])
      if m < 0:
        continue
      row = first + min(m, n - 1)
      out[b, t] = stable_crop(frames[row], poses[row], clip[b], size, extent, fused)
  return out, poses


def in_exact_range(lmk):
  """Every magnitude is zero or inside [2^-10, 2^14]: the float64 sums of the pose are then exact."""
  a = np.abs(np.asarray(lmk, np.float32))
  return bool(((a == 0) | ((a >= 2.0 ** -10) & (a <= 2.0 ** 14))).all())


def stable_case(B, hw, S, roll=0.0, t_max=T_MAX):
  """augment_cases.ragged_case (a 1-frame sample first, a full one last, windows over the left and right edge,
  degenerate mouths) plus what the stabilised window adds: eye contours at `roll` degrees, the sign alternating from
  sample to sample (0: level, both eyes at the same heights), jittered from row to row so that smoothing has work to
  do; windows hanging over the top and the bottom edge; one row whose eye points all coincide."""
  frames, lm, offsets, lens = AC.ragged_case(B, hw, S, t_max)
  H, W = hw
  rng = np.random.RandomState(77 * B + H + S + int(roll))
  rows = lm.shape[0]
  sample = np.repeat(np.arange(B), lens)
  ang = np.deg2rad(roll) * np.where(sample % 2 == 0, 1.0, -1.0) + (rng.uniform(-0.03, 0.03, rows) if roll else 0.0)
  dist = rng.uniform(0.28, 0.34, rows) * W
  mid_x, mid_y = rng.uniform(0.48, 0.52, rows) * W, rng.uniform(0.38, 0.42, rows) * H
  ring = np.stack([np.cos(np.arange(6) * np.pi / 3), 0.5 * np.sin(np.arange(6) * np.pi / 3)], 1) * 0.04 * W   # [6][2]
  for k, (a, sign) in enumerate(((36, -0.5), (42, 0.5))):
    lm[:, a:a + 6, 0] = (mid_x + sign * dist * np.cos(ang))[:, None] + ring[None, :, 0]
    lm[:, a:a + 6, 1] = (mid_y + sign * dist * np.sin(ang))[:, None] + ring[None, :, 1]
  lm[3::7, 48:68, 1] = rng.uniform(-3, 8, lm[3::7, 48:68, 1].shape)          # windows hanging over the top edge
  lm[4::7, 48:68, 1] = rng.uniform(H - 8, H + 5, lm[4::7, 48:68, 1].shape)   # and over the bottom edge
  lm[rows // 2, 36:48, :2] = 40.0                                            # coincident eye points -> minimum side
  lm = lm.astype(np.float32)
  lm[np.abs(lm) < 2.0 ** -10] = 0.0                                          # (a draw that close to zero: zero)
  assert in_exact_range(lm)
  return frames, lm, offsets, lens


def smooth_frames(rng, rows, H, W):
  """uint8 [rows][3][H][W] with a slope of well under ten grey levels per pixel: two sinusoids per plane plus a little
  noise.  For comparisons between two rules that cut the same window but round the source coordinate differently (by
  some 1e-5 px): a pixel differs where its value lies within slope * 1e-5 of a rounding boundary.  On uniform noise
  (slope ~ 100 per pixel) the restatement against lip_crop gave shares of 0.7e-4 .. 2.9e-4 on level_case's windows,
  on these frames at most 2.2e-5: the bar of 1e-3 is then far from what rounding alone does, while a window that is
  off by a tenth of a pixel still moves most of the pixels by one level."""
  yy, xx = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
  wl = rng.uniform(50, 80, (rows, 3, 2))
  ph = rng.uniform(0, 2 * np.pi, (rows, 3, 2))
  v = (128 + 60 * np.sin(2 * np.pi * xx[None, None] / wl[:, :, 0, None, None] + ph[:, :, 0, None, None]) +
       50 * np.sin(2 * np.pi * yy[None, None] / wl[:, :, 1, None, None] + ph[:, :, 1, None, None]) +
       rng.uniform(-2, 2, (rows, 3, H, W)))
  return np.clip(np.round(v), 0, 255).astype(np.uint8)


def level_case(B, hw, S, margin=0.3, extent=2.0, t_max=T_MAX):
  """A batch on which the box rule and the stabilised rule (radius 0) define the SAME window: the mouth points are ten
  pairs mirrored about a centre, so their mean is the box's centre (to a rounding), the eyes are level, eye A at x = 0
  and eye B at the box's side / extent (extent = 2: exact).  Windows reach over every edge of the frame.  Centres and
  half extents are NOT round numbers: with multiples of 1/8 whole columns of an overhanging window land on exact ties
  (a clamped row has fy = 0, and (b - a) * fx = k + 1/2 for a simple fraction fx), which the two rules' roundings then
  break differently — 3e-3 of the pixels, whatever the frames.  The frames are smooth_frames."""
  H, W = hw
  rng = np.random.RandomState(500 * B + W + S)
  lens = np.array([t_max]) if B == 1 else np.concatenate([[1], rng.randint(1, t_max + 1, B - 2), [t_max]])
  rows = int(lens.sum())
  frames = smooth_frames(rng, rows, H, W)
  lm = np.zeros((rows, 68, 3), np.float32)
  lm[:, :, 0] = rng.uniform(20, W - 20, (rows, 68))
  lm[:, :, 1] = rng.uniform(20, H - 20, (rows, 68))
  cx, cy = rng.uniform(0.0, W, rows), rng.uniform(0.0, H, rows)           # centres from edge to edge
  cx[0], cy[0] = 2.3, 3.1
  hx = rng.uniform(2, 0.2 * W, (rows, 10))                                # half extents of ten mirrored pairs
  hy = rng.uniform(1, 0.1 * H, (rows, 10))
  lm[:, 48:58, 0], lm[:, 58:68, 0] = cx[:, None] + hx, cx[:, None] - hx
  lm[:, 48:58, 1], lm[:, 58:68, 1] = cy[:, None] + hy, cy[:, None] - hy
  x, y = lm[:, 48:68, 0], lm[:, 48:68, 1]
  extent_px = np.maximum(x.max(1) - x.min(1), y.max(1) - y.min(1)).astype(np.float32)
  side = np.maximum(extent_px * f32(f32(1) + f32(2) * f32(margin)), f32(2)).astype(np.float32)   # lip_crop's
  eye = (side / f32(extent)).astype(np.float32)
  lm[:, 36:42, 0], lm[:, 36:42, 1] = 0.0, 24.0
  lm[:, 42:48, 0], lm[:, 42:48, 1] = eye[:, None], 24.0
  offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  lm[np.abs(lm) < 2.0 ** -10] = 0.0
  assert in_exact_range(lm)
  return frames, lm, offsets, lens.astype(np.int64)


def within_bar(got, want, real):
  """(max difference, share of the `real` pixels that differ): the bar is <= 1 and < 1e-3."""
  diff = np.abs(np.asarray(got).astype(np.int16) - np.asarray(want).astype(np.int16))
  return int(diff.max()), float((diff > 0).sum()) / real
