"""The float64 numpy restatement of lr_lmk_pose_collate_f32 (include/lipreading_hip.h, "Landmark pose") and the cases
the CPU and GPU tests share.  The restatement solves by SVD (Kabsch with the determinant fix), not by the kernel's
quaternion eigenproblem; the 4x4 Horn matrix appears here only in `horn_gap`, which the generator uses to assert that
every window of every case has ONE best rotation.

The generator asserts two properties of its cases, both of the restatement alone (no GPU):
  * the relative gap between the two largest eigenvalues of every window's Horn matrix is at least MIN_GAP, so that the
    rotation is well conditioned and a different method finds the same one;
  * no expected value lies within TIE_MARGIN of an fp32 rounding tie.  The margin is relative to the distance between
    the two fp32 neighbours of the value: relative to the value itself, 1e-9 is a sixtieth of that distance and a
    couple of per cent of ANY set of values lie that close to a tie, so no generator could assert it."""
import numpy as np

RIGID_68 = (27, 28, 29, 30, 33, 36, 39, 42, 45)
RIGID_4 = (3, 0, 1)               # the minimal case: four points, three of them rigid, given out of order
LENS = (1, 4, 9)
MIN_GAP = 0.05
TIE_MARGIN = 1e-9
OK, DEGENERATE, BAD_ROW = 0, 1, 2


# ---- the restatement ------------------------------------------------------------------------------------------------
def row_stats(lmk, tmpl, rigid):
  """-> pbar [rows][3], M [rows][3][3], v [rows], bad [rows] and qbar [3], all float64."""
  x = np.asarray(lmk, dtype=np.float32).astype(np.float64)
  idx = list(rigid)
  q = np.asarray(tmpl, dtype=np.float32).astype(np.float64)[idx]
  with np.errstate(all="ignore"):
    qbar = q.mean(axis=0)
    p = x[:, idx]
    pbar = p.mean(axis=1)
    dp, dq = p - pbar[:, None], q - qbar
    M = np.einsum("ia,nib->nab", dq, dp)
    v = (dp * dp).sum(axis=(1, 2))
  bad = ~np.isfinite(x).all(axis=(1, 2))
  return pbar, M, v, bad, qbar


def rotation(M, det_fix=True):
  """The rotation that maximises tr(R M^T): for M = U S V^T, R = U diag(1, 1, det(U V^T)) V^T."""
  U, _, Vt = np.linalg.svd(M)
  d = np.sign(np.linalg.det(U @ Vt)) if det_fix else 1.0
  return U @ np.diag([1.0, 1.0, d]) @ Vt


def horn_matrix(M):
  S = np.asarray(M, dtype=np.float64).T    # Horn's S = sum p q^T
  (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = S
  return np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                   [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                   [zx - xz, xy + yx, -xx + yy - zz, yz + zy],
                   [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])


def horn_gap(M):
  """(largest - second largest eigenvalue) / largest magnitude of the window's Horn matrix."""
  w = np.linalg.eigvalsh(horn_matrix(M))
  return float((w[3] - w[2]) / np.abs(w).max())


def windows(offsets, lens, radius, cross=False):
  """row -> the rows of its window (before the BAD rows are dropped).  cross: the WRONG window that ignores samples."""
  rows = int(np.sum(lens))
  out = {}
  for b in range(len(lens)):
    lo, n = int(offsets[b]), int(lens[b])
    for i in range(n):
      if cross:
        out[lo + i] = list(range(max(0, lo + i - radius), min(rows - 1, lo + i + radius) + 1))
      else:
        out[lo + i] = list(range(lo + max(0, i - radius), lo + min(n - 1, i + radius) + 1))
  return out


def poses(lmk, offsets, lens, tmpl, rigid, radius, scale, variant=None):
  """-> R [rows][3][3], s [rows], pbar [rows][3], status [rows] int32, qbar [3], gaps [rows] (float64).
  variant: None, or one of the deliberately WRONG 'cross' (the window runs into the neighbouring sample),
  'smooth_centroid' (the translation is averaged over the window) and 'no_det' (no determinant fix)."""
  assert variant in (None, "cross", "smooth_centroid", "no_det")
  pbar, M, v, bad, qbar = row_stats(lmk, tmpl, rigid)
  rows = len(pbar)
  R = np.tile(np.eye(3), (rows, 1, 1))
  s = np.ones(rows)
  pb = np.zeros((rows, 3))
  status = np.zeros(rows, dtype=np.int32)
  gaps = np.full(rows, np.nan)
  for n, win in windows(offsets, lens, radius, cross=variant == "cross").items():
    if bad[n]:
      status[n] = BAD_ROW
      continue
    use = [m for m in win if not bad[m]]
    pb[n] = pbar[n] if variant != "smooth_centroid" else np.mean([pbar[m] for m in use], axis=0)
    Mw, vw = np.zeros((3, 3)), 0.0
    for m in use:                              # ascending
      Mw = Mw + M[m]
      vw = vw + v[m]
    if not use or vw == 0.0:
      status[n] = DEGENERATE
      continue
    R[n] = rotation(Mw, det_fix=variant != "no_det")
    gaps[n] = horn_gap(Mw)
    if scale:
      s[n] = np.trace(R[n] @ Mw.T) / vw
  return R, s, pb, status, qbar, gaps


def pose_batch(lmk, offsets, lens, tmap, t_max, tmpl, rigid, radius, scale, variant=None):
  """-> out f32 [B][t_max][npts][3], pose f32 [rows][13], status int32 [rows], out64 (the values before their one
  rounding), gaps."""
  x = np.asarray(lmk, dtype=np.float32).astype(np.float64)
  R, s, pb, status, qbar, gaps = poses(lmk, offsets, lens, tmpl, rigid, radius, scale, variant)
  B, npts = len(lens), x.shape[1]
  out64 = np.zeros((B, t_max, npts, 3))
  for b in range(B):
    lo, n = int(offsets[b]), int(lens[b])
    for t in range(min(n, t_max)):
      m = t if tmap is None else int(tmap[lo + t])
      if m < 0:
        continue
      r = lo + min(m, n - 1)
      if status[r] == BAD_ROW:
        continue
      out64[b, t] = s[r] * ((x[r] - pb[r]) @ R[r].T) + qbar
  pose = np.concatenate([R.reshape(-1, 9), s[:, None], pb], axis=1).astype(np.float32)
  return out64.astype(np.float32), pose, status, out64, gaps


# ---- tolerances -----------------------------------------------------------------------------------------------------
def ulp(want):
  """One fp32 ulp of the restatement's value, taken at max(|want|, 2^-10)."""
  return np.spacing(np.maximum(np.abs(np.asarray(want, dtype=np.float32)), np.float32(2.0 ** -10))).astype(np.float64)


def worst_ulps(got, want):
  """max |got - want| in units of `ulp(want)`."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float32)
  return float(np.max(np.abs(got - want.astype(np.float64)) / ulp(want))) if want.size else 0.0


def tie_distance(x64):
  """min over the values of |x - tie| / (distance between x's two fp32 neighbours), the tie being their midpoint."""
  x = np.asarray(x64, dtype=np.float64).ravel()
  x = x[x != 0.0]
  f = x.astype(np.float32)
  below = np.where(f.astype(np.float64) <= x, f, np.nextafter(f, np.float32(-np.inf)))
  above = np.nextafter(below, np.float32(np.inf))
  lo, hi = below.astype(np.float64), above.astype(np.float64)
  return float(np.min(np.abs(x - 0.5 * (lo + hi)) / (hi - lo))) if x.size else 1.0


# ---- the cases ------------------------------------------------------------------------------------------------------
def rot(axis, angle):
  a = np.asarray(axis, dtype=np.float64)
  a = a / np.linalg.norm(a)
  K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
  return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def template(npts):
  """A face-like, non-coplanar template in the pixels range (npts = 68), or the minimal four points."""
  if npts == 4:
    return np.array([[100, 100, 0], [160, 105, 3], [120, 150, -8], [125, 120, 40]], dtype=np.float32)
  assert npts == 68
  rng = np.random.RandomState(68)
  t = np.stack([rng.uniform(-70, 70, 68), rng.uniform(-60, 90, 68), rng.uniform(-20, 20, 68)], axis=1)
  ang = np.linspace(0, 2 * np.pi, 6, endpoint=False)
  for lo, cx in ((36, -31.0), (42, 31.0)):           # the eye contours
    t[lo:lo + 6] = np.stack([cx + 13 * np.cos(ang), -30 + 5 * np.sin(ang), 2 - 7 * np.abs(np.cos(ang))], axis=1)
  ang = np.linspace(0, 2 * np.pi, 20, endpoint=False)
  t[48:68] = np.stack([25 * np.cos(ang), 45 + 10 * np.sin(ang), 12 - 6 * np.abs(np.cos(ang))], axis=1)
  t[27:31] = [[0, -30, 10], [0, -20, 16], [0, -10, 22], [0, 0, 30]]     # the nose bridge stands out of the face
  t[33] = [0, 10, 18]
  t += rng.uniform(-1, 1, t.shape)                    # nothing is exactly symmetric
  return (t + [100, 100, 0]).astype(np.float32)


def make_clips(npts, lens=LENS, seed=0, mirrored=False):
  """lmk f32 [rows][npts][3], offsets i64, lens i64: the template with noise on all points, a larger 'mouth' motion on
  points 48..67 (npts = 4: on the one point that is not rigid), one rigid motion and scale per clip and a small drift
  of the head from frame to frame.  mirrored: the face itself is mirrored, so the best ORTHOGONAL fit is a reflection."""
  rng = np.random.RandomState(1000 * seed + npts + (7 if mirrored else 0))
  tm = template(npts).astype(np.float64)
  centre = tm.mean(axis=0)
  clips = []
  for n in lens:
    R0 = rot(rng.randn(3), rng.uniform(0.2, 0.6))
    s0 = rng.uniform(0.75, 1.3)
    t0 = centre + rng.uniform(-30, 30, 3)
    drift_a = np.cumsum(rng.randn(n) * 0.03)
    drift_t = np.cumsum(rng.randn(n, 3) * 1.5, axis=0)
    axis = rng.randn(3)
    clip = np.zeros((n, npts, 3))
    for i in range(n):
      face = tm - centre + rng.randn(npts, 3) * 0.4
      if npts == 68:
        face[48:68] += rng.randn(20, 3) * 2.5
      else:
        face[2] += rng.randn(3) * 2.5
      if mirrored:
        face[:, 0] = -face[:, 0]
      clip[i] = s0 * (face @ (rot(axis, drift_a[i]) @ R0).T) + t0 + drift_t[i]
    clips.append(clip)
  lens = np.array(lens, dtype=np.int64)
  offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  return np.concatenate(clips).astype(np.float32), offsets, lens


def nudge_off_ties(lmk, rigid):
  """The centroid of a few fp32 values is a rational number of fp32 steps (a multiple of a ninth, or a third, of the
  finest step among them), so it lands EXACTLY on a rounding tie every few dozen values.  Where it does, one rigid
  coordinate of that row moves by one fp32 step."""
  lmk = np.array(lmk, dtype=np.float32)
  idx = list(rigid)
  for n in range(len(lmk)):
    for c in range(3):
      for _ in range(8):
        if tie_distance([lmk[n, idx, c].astype(np.float64).mean()]) >= 1e-3:
          break
        lmk[n, idx[0], c] = np.nextafter(lmk[n, idx[0], c], np.float32(np.inf))
      else:
        raise AssertionError("row %d keeps its centroid on a rounding tie" % n)
  return lmk


SHAPES = [(68, RIGID_68), (4, RIGID_4)]
RADII = (0, 2, 32)
T_MAXES = (9, 12)
_cache = {}


def case(npts, rigid, radius, scale, t_max, mirrored=False):
  """One parity case, computed once and shared (read only): a dict with the inputs and the restatement's answer.  The
  generator's two asserts run here."""
  key = (npts, tuple(rigid), radius, bool(scale), t_max, bool(mirrored))
  if key not in _cache:
    lmk, offsets, lens = make_clips(npts, mirrored=mirrored)
    lmk = nudge_off_ties(lmk, rigid)
    tmpl = template(npts)
    out, pose, status, out64, gaps = pose_batch(lmk, offsets, lens, None, t_max, tmpl, rigid, radius, scale)
    assert (status == OK).all()
    assert np.nanmin(gaps) >= MIN_GAP, "a window's Horn matrix has a relative gap of %g" % np.nanmin(gaps)
    pose64 = np.concatenate([poses(lmk, offsets, lens, tmpl, rigid, radius, scale)[i].reshape(len(lmk), -1)
                             for i in (1, 2)], axis=1)
    tie = min(tie_distance(out64), tie_distance(pose64))
    assert tie >= TIE_MARGIN, "an expected value lies %g of an fp32 step from a rounding tie" % tie
    for a in (lmk, offsets, lens, tmpl, out, pose, status, out64, gaps):
      a.setflags(write=False)
    _cache[key] = dict(lmk=lmk, offsets=offsets, lens=lens, tmpl=tmpl, rigid=tuple(rigid), radius=radius, scale=scale,
                       t_max=t_max, out=out, pose=pose, status=status, out64=out64, gaps=gaps)
  return _cache[key]


def all_cases(mirrored=(False, True)):
  for npts, rigid in SHAPES:
    for radius in RADII:
      for scale in (True, False):
        for t_max in T_MAXES:
          for mir in mirrored:
            yield case(npts, rigid, radius, scale, t_max, mirrored=mir)


def exact_clip(npts, n=6, seed=3):
  """A clip on a 1/64 grid with |coordinate| < 128: signed axis permutations, scales of 1/2 and 2 and integer
  translations of it are exact in fp32."""
  lmk, _, _ = make_clips(npts, lens=(n,), seed=seed)
  return (np.round(lmk.astype(np.float64) * 0.5 * 64) / 64).astype(np.float32)
