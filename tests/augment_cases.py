"""Shared by tests/test_augment_cpu.py and tests/test_gpu_augment.py: a float32 numpy restatement of the augmented
crop (lr_lip_crop_collate_aug_u8) and the ragged batches both files grade on.

`augmented_crop` is oracle.torch_oracle.lip_crop's arithmetic, line for line, with the window taken from the box rule
of the augmented kernel: side' = max(side * zoom, 2), left = (dx * side + cx) - side' / 2 (top likewise),
scale = side' / S, mirrored columns when flip is set.  With the identity record it equals lip_crop byte for byte
(test_augment_cpu checks that).  fused=True evaluates every a + b * c with ONE rounding, as the kernel's fmaf does
(through float64, where a product of two float32 is exact); the default is lip_crop's plain float32 products and sums.
"""
import numpy as np

f32 = np.float32


def _madd(a, b, c, fused):
  """a + b * c in float32: two roundings (plain) or one (fused)."""
  if fused:
    return (np.asarray(a, np.float64) + np.asarray(b, np.float64) * np.asarray(c, np.float64)).astype(np.float32)
  return (np.asarray(a, np.float32) + (np.asarray(b, np.float32) * np.asarray(c, np.float32)).astype(np.float32)
          ).astype(np.float32)


def augmented_crop(frame, lmk, record, size=96, margin=0.3, lo=48, hi=68, fused=False):
  """One frame uint8 [3][H][W] with its landmarks [68][3] and a record (dx, dy, zoom, flip) -> uint8 [3][size][size]."""
  frame = np.asarray(frame)
  lmk = np.asarray(lmk, dtype=np.float32)
  dx, dy, zoom, flip = (f32(v) for v in record)
  _, H, W = frame.shape
  x, y = lmk[lo:hi, 0], lmk[lo:hi, 1]
  x0, x1, y0, y1 = x.min(), x.max(), y.min(), y.max()
  side = max(f32(max(x1 - x0, y1 - y0)) * f32(f32(1) + f32(2) * f32(margin)), f32(2))
  side_z = max(f32(side * zoom), f32(2))
  left = f32(_madd(f32(0.5) * (x0 + x1), dx, side, fused)) - f32(0.5) * side_z
  top = f32(_madd(f32(0.5) * (y0 + y1), dy, side, fused)) - f32(0.5) * side_z
  scale = f32(side_z / f32(size))
  o = np.arange(size, dtype=np.float32)
  sx = np.clip(_madd(left, o + f32(0.5), scale, fused) - f32(0.5), 0, W - 1).astype(np.float32)
  sy = np.clip(_madd(top, o + f32(0.5), scale, fused) - f32(0.5), 0, H - 1).astype(np.float32)
  ix, iy = np.floor(sx).astype(int), np.floor(sy).astype(int)
  ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
  fx, fy = (sx - ix).astype(np.float32), (sy - iy).astype(np.float32)
  img = frame.astype(np.float32)
  a, b = img[:, iy][:, :, ix], img[:, iy][:, :, ix1]
  d, e = img[:, iy1][:, :, ix], img[:, iy1][:, :, ix1]
  tv = _madd(a, b - a, fx[None, None, :], fused)
  bv = _madd(d, e - d, fx[None, None, :], fused)
  v = _madd(tv, bv - tv, fy[None, :, None], fused)
  out = np.clip(np.floor(v + f32(0.5)), 0, 255).astype(np.uint8)
  return out[:, :, ::-1] if flip != 0 else out      # pixel (oy, ox) of the mirrored clip is pixel (oy, S - 1 - ox)


def augmented_batch(frames, lmk, offsets, lens, clip, tmap, t_max, size, margin=0.3, lo=48, hi=68, fused=False):
  """The whole padded batch uint8 [B][t_max][3][size][size]: zeros past a sample's length and at masked frames, the
  map's value clamped to the sample's last frame."""
  B = len(lens)
  out = np.zeros((B, t_max, 3, size, size), np.uint8)
  for b in range(B):
    first, n = int(offsets[b]), int(lens[b])
    for t in range(min(n, t_max)):
      m = int(tmap[first + t])
      if m < 0:
        continue
      row = first + min(m, n - 1)
      out[b, t] = augmented_crop(frames[row], lmk[row], clip[b], size, margin, lo, hi, fused)
  return out


def identity_records(lens):
  """The record and the map that change nothing."""
  lens = np.asarray(lens, dtype=np.int64)
  clip = np.zeros((len(lens), 4), np.float32)
  clip[:, 2] = 1.0
  tmap = np.concatenate([np.arange(int(n), dtype=np.int32) for n in lens])
  return clip, tmap


T_MAX = 7


def ragged_case(B, hw, S, t_max=T_MAX):
  """The batch of test_collate_kernel_equals_per_sample_launches (tests/test_gpu_loader.py) for one point of its grid:
  a 1-frame sample first and a full-t_max sample last, windows hanging over the left and the right edge, degenerate
  boxes.  Returns frames u8 [rows][3][H][W], lmk f32 [rows][68][3], offsets i64 [B], lens i64 [B]."""
  H, W = hw
  rng = np.random.RandomState(1000 * B + H + S)
  if B == 1:
    lens = np.array([t_max])
  else:
    lens = rng.randint(1, t_max + 1, B)
    lens[0], lens[-1] = 1, t_max
  rows = int(lens.sum())
  frames = rng.randint(0, 256, (rows, 3, H, W)).astype(np.uint8)
  lm = np.zeros((rows, 68, 3), np.float32)
  lm[:, :, 0] = rng.uniform(20, W - 20, (rows, 68))
  lm[:, :, 1] = rng.uniform(20, H - 20, (rows, 68))
  lm[:, 48:68, 0] = rng.uniform(0.4 * W, 0.6 * W, (rows, 20))
  lm[:, 48:68, 1] = rng.uniform(0.6 * H, 0.75 * H, (rows, 20))
  lm[1::5, 48:68, 0] = rng.uniform(-5, 12, lm[1::5, 48:68, 0].shape)   # windows hanging over the left edge
  lm[2::5, 48:68, :2] = 50.0                                          # degenerate boxes -> minimum side
  lm[0, 48:68, 0] = rng.uniform(W - 10, W + 6, 20)                    # and one over the right edge
  offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  return frames, lm, offsets, lens.astype(np.int64)
