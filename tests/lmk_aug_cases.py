"""The float64 numpy restatement of lr_lmk_augment_f32 (include/lipreading_hip.h, "Landmark augmentation") and the cases
the CPU and GPU tests share.  The restatement is written from the header's text, clip by clip and point by point; its
records are built by hand (`record`), not by LandmarkAugmentSpec.draw, so the device is graded against nothing of the new
code.

Tolerance: tests/pose_cases.py's, unchanged — `worst_ulps(got, want) <= 1`, one fp32 ulp taken at max(|want|, 2^-10).
Restatement and device differ only in float64 summation order and fused multiply-adds; next to the one fp32 rounding
that moves a result only across a rounding tie.  `pairwise=True` evaluates the statistics with np.sum's pairwise sums
in place of ascending ones: tests/test_lmk_aug_cpu.py pins that the two stay within that ulp of each other."""
import numpy as np

from tests import pose_cases as PC

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
UNIT = 2.6428997921303014e-05            # 1 / sqrt(4 * (65536^2 - 1) / 12)
WORDS = 16
LENS = PC.LENS                           # (1, 4, 9)
T_MAXES = PC.T_MAXES                     # (9, 12)

MIRROR_68_FIXED = (8, 27, 28, 29, 30, 33, 51, 57, 62, 66)


def mirror_68():
  """The iBUG partners, from the issue's list (the product's own table is landmarks.MIRROR_68)."""
  p = list(range(68))
  pairs = [(i, 16 - i) for i in range(8)] + [(17 + i, 26 - i) for i in range(5)] + [(31, 35), (32, 34)]
  pairs += [(36, 45), (37, 44), (38, 43), (39, 42), (40, 47), (41, 46)]
  pairs += [(48, 54), (49, 53), (50, 52), (55, 59), (56, 58), (60, 64), (61, 63), (65, 67)]
  for a, b in pairs:
    p[a], p[b] = b, a
  return p


def perm_for(npts):
  """An involution of range(npts): the 68-point partners, otherwise j <-> npts - 1 - j."""
  return mirror_68() if npts == 68 else [npts - 1 - j for j in range(npts)]


# ---- the restatement ------------------------------------------------------------------------------------------------
def mix(z):
  """splitmix64's finaliser over uint64 (wrapping)."""
  z = np.asarray(z, dtype=np.uint64)
  with np.errstate(over="ignore"):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
  return z ^ (z >> np.uint64(31))


def unit_noise(key, t_max, npts):
  """g [t_max][npts][3] float64 of one clip."""
  idx = np.arange(t_max * npts * 3, dtype=np.uint64).reshape(t_max, npts, 3)
  with np.errstate(over="ignore"):
    z = mix(np.uint64(key) + GOLDEN + idx)
  m = np.uint64(0xFFFF)
  s = (z & m) + ((z >> np.uint64(16)) & m) + ((z >> np.uint64(32)) & m) + (z >> np.uint64(48))
  return (s.astype(np.int64) - 131070).astype(np.float64) * UNIT


def record(A=None, shift=(0.0, 0.0, 0.0), jitter=0.0, mirror=False, key=0):
  """One clip's 16 words, uint64."""
  r = np.zeros(WORDS, np.float64)
  r[:9] = np.eye(3).ravel() if A is None else np.asarray(A, dtype=np.float64).ravel()
  r[9:12] = shift
  r[12] = jitter
  r[13] = 1.0 if mirror else 0.0
  w = r.view(np.uint64)
  w[14] = np.uint64(key)
  return w


def live_rows(x, lens):
  """bool [B][t_max]: inside the clip, not all zero, all finite."""
  x = np.asarray(x, dtype=np.float32)
  t_max = x.shape[1]
  n = np.clip(np.asarray(lens, dtype=np.int64), 0, t_max)
  inside = np.arange(t_max)[None, :] < n[:, None]
  with np.errstate(invalid="ignore"):
    return inside & ~(x == 0).all(axis=(2, 3)) & np.isfinite(x).all(axis=(2, 3))


def _total(v, pairwise):
  v = np.asarray(v, dtype=np.float64).ravel()
  if not v.size:
    return 0.0
  return float(np.sum(v)) if pairwise else float(np.cumsum(v)[-1])


def clip_stats(x, lens, pairwise=False):
  """(c_x, c_y, c_z, r) float64 [B][4]."""
  x = np.asarray(x, dtype=np.float32)
  live = live_rows(x, lens)
  out = np.zeros((x.shape[0], 4))
  for b in range(x.shape[0]):
    v = x[b][live[b]].astype(np.float64).reshape(-1, 3)
    n = float(len(v))
    if n == 0:
      continue
    c = np.array([_total(v[:, k], pairwise) / n for k in range(3)])
    m2 = _total(v * v, pairwise) / n
    out[b, :3] = c
    out[b, 3] = np.sqrt(max(m2 - float(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), 0.0))
  return out


def augment(x, lens, rec, perm, pairwise=False):
  """-> y f32 [B][t_max][npts][3], stats f64 [B][4], y64 (the values before their one rounding)."""
  x = np.asarray(x, dtype=np.float32)
  B, t_max, npts, _ = x.shape
  rec = np.asarray(rec, dtype=np.uint64).reshape(B, WORDS)
  live = live_rows(x, lens)
  stats = clip_stats(x, lens, pairwise)
  src = np.clip(np.asarray(perm, dtype=np.int64), 0, npts - 1)
  y64 = np.zeros(x.shape, np.float64)
  for b in range(B):
    f = rec[b].view(np.float64)
    A, shift, jitter, mirror, key = f[:9].reshape(3, 3), f[9:12], f[12], f[13] != 0.0, rec[b, 14]
    c, r = stats[b, :3], stats[b, 3]
    xs = x[b].astype(np.float64)
    if mirror:
      xs = xs[:, src]
    d = xs - c
    add = np.broadcast_to(shift, d.shape).copy()
    if jitter != 0.0:
      add = add + jitter * unit_noise(key, t_max, npts)
    with np.errstate(all="ignore"):
      for k in range(3):
        lin = A[k, 0] * d[..., 0] + A[k, 1] * d[..., 1] + A[k, 2] * d[..., 2]
        y64[b, :, :, k] = (lin + c[k]) + r * add[..., k]
    y64[b][~live[b]] = 0.0
  return y64.astype(np.float32), stats, y64


# ---- tolerances: tests/pose_cases.py's, unchanged -----------------------------------------------------------------------
worst_ulps = PC.worst_ulps


# ---- the cases ------------------------------------------------------------------------------------------------------
def pad(lmk, offsets, lens, t_max, fill=0.0):
  """Ragged [rows][npts][3] -> the collated batch [B][t_max][npts][3] (rows past a clip hold `fill`)."""
  lmk = np.asarray(lmk, dtype=np.float32)
  out = np.full((len(lens), t_max) + lmk.shape[1:], fill, np.float32)
  for b, (lo, n) in enumerate(zip(offsets, lens)):
    n = min(int(n), t_max)
    out[b, :n] = lmk[int(lo):int(lo) + n]
  return out


def clips(npts, lens=LENS, seed=0):
  """Face-like clips for any npts: pose_cases.make_clips for 68 and 4 points, otherwise the first npts points of the
  68-point clips tiled with a small offset per copy."""
  if npts in (68, 4):
    return PC.make_clips(npts, lens=lens, seed=seed)
  lmk, offsets, lens = PC.make_clips(68, lens=lens, seed=seed)
  reps = -(-npts // 68)
  wide = np.concatenate([lmk + np.float32(3.0 * i) for i in range(reps)], axis=1)[:, :npts]
  return np.ascontiguousarray(wide), offsets, lens


def full_matrix(mirror):
  """A full policy's matrix: scale 1.07, a turn of 0.3 rad about a skew axis, stretches 1.04 / 0.97, the mirror's sign."""
  A = 1.07 * PC.rot([0.3, 1.0, -0.5], 0.3) @ np.diag([1.04, 0.97, 1.0])
  return A @ np.diag([-1.0 if mirror else 1.0, 1.0, 1.0])


RECORDS = ("identity", "mirror", "rotation", "full", "full_jitter")


def records(kind, B):
  """uint64 [B][16]: clip b's record of the named kind (the clips of a batch differ where the kind allows it)."""
  out = []
  for b in range(B):
    if kind == "identity":
      out.append(record())
    elif kind == "mirror":
      out.append(record(A=np.diag([-1.0, 1.0, 1.0]), mirror=True))
    elif kind == "rotation":
      out.append(record(A=PC.rot([0.2 * b, 1.0, 0.4], 0.25 - 0.2 * b)))
    elif kind == "full":
      out.append(record(A=full_matrix(b % 2 == 0), shift=(0.05, -0.03 * b, 0.02), mirror=b % 2 == 0))
    elif kind == "full_jitter":
      out.append(record(A=full_matrix(b % 2 == 1), shift=(-0.04, 0.01, 0.05 * b), jitter=0.01 * (b + 1),
                        mirror=b % 2 == 1, key=0xC0FFEE0000000000 + 977 * b))
    else:
      raise KeyError(kind)
  return np.stack(out)


_cache = {}


def case(npts, t_max, kind, lens=LENS):
  """One parity case, computed once and shared (read only): the inputs and the restatement's answer."""
  key = (npts, t_max, kind, tuple(lens))
  if key not in _cache:
    lmk, offsets, n = clips(npts, lens=lens)
    x = pad(lmk, offsets, n, t_max)
    rec = records(kind, len(n))
    perm = perm_for(npts)
    y, stats, y64 = augment(x, n, rec, perm)
    for a in (x, rec, y, stats, y64):
      a.setflags(write=False)
    _cache[key] = dict(x=x, lens=np.asarray(n, dtype=np.int32), rec=rec, perm=perm, y=y, stats=stats, y64=y64,
                       npts=npts, t_max=t_max, kind=kind)
  return _cache[key]


def parity_cases():
  """The issue's grid: npts 68 and 4, t_max 9 and 12, the five records; then npts 1 and 256 and one clip of 130 rows."""
  for npts in (68, 4):
    for t_max in T_MAXES:
      for kind in RECORDS:
        yield case(npts, t_max, kind)
  for npts in (1, 256):
    for kind in ("full", "full_jitter"):
      yield case(npts, 9, kind)
  for kind in ("mirror", "full_jitter"):
    yield case(68, 130, kind, lens=(130,))


def semantics_case(t_max=9):
  """Garbage in the padding rows, an all-zero masked row and a NaN row inside clips, a clip without a LIVE row and
  lens[b] > t_max.  -> x, lens (int32 [4])."""
  lmk, offsets, lens = clips(68, lens=(4, 9, 3, 9), seed=2)
  x = pad(lmk, offsets, lens, t_max, fill=777.25)            # the padding rows hold garbage
  x[1, 3] = 0.0                                              # a masked frame
  x[1, 5, 11, 2] = -0.0
  x[1, 6, 50, 1] = np.nan                                    # a NaN row
  x[3, 2, 7, 0] = np.inf
  x[2, :3] = 0.0                                             # no LIVE row at all ...
  x[2, 1, 3, 1] = np.nan                                     # ... one of them by a NaN
  return x, np.array([4, 9, 3, t_max + 5], dtype=np.int32)


def exact_case():
  """npts 4, len 4, integer coordinates about the centre (10, 20, 5) at distance 5: c = (10, 20, 5) and r = 5 exactly.
  A quarter turn about z and shift * r = (2, -1, 1).  -> x [1][4][4][3], rec, the integer answer."""
  d = np.array([[[3, 4, 0], [-3, -4, 0], [4, -3, 0], [-4, 3, 0]],
                [[0, 5, 0], [0, -5, 0], [5, 0, 0], [-5, 0, 0]],
                [[3, 0, 4], [-3, 0, -4], [0, 4, 3], [0, -4, -3]],
                [[0, 0, 5], [0, 0, -5], [4, 3, 0], [-4, -3, 0]]], dtype=np.float64)
  c = np.array([10.0, 20.0, 5.0])
  turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
  want = d @ turn.T + c + np.array([2.0, -1.0, 1.0])
  rec = record(A=turn, shift=(0.4, -0.2, 0.2))[None]
  return (d + c).astype(np.float32)[None], rec, want.astype(np.float32)[None]
