"""Training-time clip augmentation: the policy and its draws.  Host only — numpy, no GPU, no torch.

The host draws, the kernel applies (DESIGN.md "Clip augmentation"): a worker thread of loader.HostStage calls
`AugmentSpec.draw` once per batch and packs the result into the batch's slot; lr_lip_crop_collate_aug_u8 /
lr_collate_pad_aug_f32 apply it inside the collate launch.  No random number is made on the device.

  clip[b] = (dx, dy, zoom, flip)   one record per CLIP (the mouth must not jump between frames): the crop window is
                                   moved by (dx, dy) of its un-zoomed side, its side is scaled by zoom, and the output
                                   is mirrored left-right when flip is 1
  tmap[offsets[b] + t]             the source frame, within sample b, of output frame t, or -1 for a masked frame:
                                   temporal jitter (frames dropped or doubled) re-indexes a clip onto its OWN length,
                                   so frame_lens, label lengths and batch shapes are those of the un-augmented loader

A record depends on (seed, pass number, dataset index, clip length) and on nothing else: not on the batch it is drawn
in, its size, the prefetch depth or the worker that packs it.  The draws are therefore stateless: a counter-based hash
(the splitmix64 finaliser, chained over the four keys and a slot number) evaluated in numpy uint64 over the whole
batch.  No numpy Generator is built per sample — workers hold the GIL while they draw.

`LandmarkAugmentSpec` (below) is the landmark regime's policy, drawn the same way over a stream of its own: one 3x3
matrix, a shift and a noise key per clip, applied by lr_lmk_augment_f32 to the collated batch.
"""
import numpy as np

MAX_MASKS = 8

_U = np.uint64
_GOLDEN = _U(0x9E3779B97F4A7C15)
_M1, _M2 = _U(0xBF58476D1CE4E5B9), _U(0x94D049BB133111EB)
_S30, _S27, _S31, _S11 = _U(30), _U(27), _U(31), _U(11)

# slot numbers of a clip's draws; per-frame draws start at _SLOT_FRAME
_SLOT_DX, _SLOT_DY, _SLOT_ZOOM, _SLOT_FLIP, _SLOT_MASK, _SLOT_FRAME = 0, 1, 2, 3, 4, 4 + 2 * MAX_MASKS


def _mix(z):
  """splitmix64's finaliser over a uint64 array (wrapping multiplies)."""
  z = (z ^ (z >> _S30)) * _M1
  z = (z ^ (z >> _S27)) * _M2
  return z ^ (z >> _S31)


def _absorb(h, key):
  return _mix(h + _GOLDEN + np.asarray(key).astype(np.uint64))


def _uniform(h, slot):
  """float64 in [0, 1): 53 bits of the hash of (h, slot)."""
  return (_absorb(h, slot) >> _S11).astype(np.float64) * (1.0 / (1 << 53))


def _f32_inside(lo, hi):
  """The float32 interval inside [lo, hi] (the float32 nearest to a bound may lie outside it)."""
  a, b = np.float32(lo), np.float32(hi)
  if float(a) < lo:
    a = np.nextafter(a, np.float32(np.inf))
  if float(b) > hi:
    b = np.nextafter(b, np.float32(-np.inf))
  return a, b


class AugmentSpec(object):
  """flip: probability of a left-right mirror; shift: the window moves by up to +-shift of its side in x and in y;
  zoom: its side is scaled by a factor in [1 - zoom, 1 + zoom]; tjitter: every source frame is dropped with
  probability tjitter / 2 and doubled with probability tjitter / 2; tmask = (N, W): N spans of up to W frames are
  zeroed (never more than half a clip); seed: the stream of draws."""

  FIELDS = ("flip", "shift", "zoom", "tjitter", "tmask")

  def __init__(self, flip=0.0, shift=0.0, zoom=0.0, tjitter=0.0, tmask=(0, 0), seed=0):
    self.flip, self.shift, self.zoom, self.tjitter = float(flip), float(shift), float(zoom), float(tjitter)
    try:
      n, w = tmask
      self.tmask = (int(n), int(w))
      exact = self.tmask[0] == n and self.tmask[1] == w
    except (TypeError, ValueError):
      raise ValueError("tmask must be (N, W) or 'NxW', got %r" % (tmask,))
    self.seed = int(seed)
    if not 0.0 <= self.flip <= 1.0:
      raise ValueError("flip must be in [0, 1], got %r" % (flip,))
    for name in ("shift", "zoom", "tjitter"):
      if not 0.0 <= getattr(self, name) <= 0.5:
        raise ValueError("%s must be in [0, 0.5], got %r" % (name, getattr(self, name)))
    if not exact or not 0 <= self.tmask[0] <= MAX_MASKS or self.tmask[1] < 0:
      raise ValueError("tmask = NxW needs integers 0 <= N <= %d and W >= 0, got %r" % (MAX_MASKS, tmask))

  @classmethod
  def parse(cls, text, seed=0):
    """'flip=0.5,shift=0.08,zoom=0.1,tjitter=0.05,tmask=2x10' -> AugmentSpec; '' -> None."""
    text = (text or "").strip()
    if not text:
      return None
    args = {}
    for item in text.split(","):
      key, eq, value = item.strip().partition("=")
      key, value = key.strip(), value.strip()
      if key not in cls.FIELDS or not eq:
        raise ValueError("unknown augmentation %r (known: %s)" % (item.strip(), ", ".join(cls.FIELDS)))
      if key in args:
        raise ValueError("augmentation %r is given twice" % key)
      try:
        if key == "tmask":
          n, x, w = value.lower().partition("x")
          if not x:
            raise ValueError(value)
          args[key] = (int(n), int(w))
        else:
          args[key] = float(value)
      except ValueError:
        raise ValueError("cannot read %r as a value of %s" % (value, key))
    return cls(seed=seed, **args)

  def __str__(self):
    return "flip=%r,shift=%r,zoom=%r,tjitter=%r,tmask=%dx%d" % ((self.flip, self.shift, self.zoom, self.tjitter) +
                                                                 self.tmask)

  def __repr__(self):
    return "AugmentSpec(%s, seed=%d)" % (str(self).replace(",", ", "), self.seed)

  def _key(self):
    return (self.flip, self.shift, self.zoom, self.tjitter, self.tmask, self.seed)

  def __eq__(self, other):
    return isinstance(other, AugmentSpec) and self._key() == other._key()

  def __ne__(self, other):
    return not self == other

  def __hash__(self):
    return hash(self._key())

  @property
  def spatial(self):
    return self.flip > 0.0 or self.shift > 0.0 or self.zoom > 0.0

  @property
  def temporal(self):
    return self.tjitter > 0.0 or (self.tmask[0] > 0 and self.tmask[1] > 0)

  def draw(self, pass_no, indices, lens):
    """The records of one batch: (clip float32 [B][4], tmap int32 [sum(lens)]).  indices: the samples' dataset
    indices; lens: their frame counts.  Vectorised over the batch; sample b's record is a function of
    (seed, pass_no, indices[b], lens[b]) alone."""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    assert idx.shape == lens.shape and (lens > 0).all()
    B, rows = len(lens), int(lens.sum())
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    clip_of = np.repeat(np.arange(B), lens)                 # the sample of every frame
    t_of = np.arange(rows, dtype=np.int64) - offsets[clip_of]   # and the frame's position in it
    clip = np.zeros((B, 4), np.float32)
    clip[:, 2] = 1.0
    tmap = t_of.astype(np.int32)
    if not (self.spatial or self.temporal):
      return clip, tmap
    with np.errstate(over="ignore"):
      h = _mix(np.full(B, self.seed, dtype=np.int64).astype(np.uint64) ^ _GOLDEN)
      for key in (np.full(B, int(pass_no), dtype=np.int64), idx, lens):
        h = _absorb(h, key)
      if self.shift > 0.0:
        lo, hi = _f32_inside(-self.shift, self.shift)
        for col, slot in ((0, _SLOT_DX), (1, _SLOT_DY)):
          clip[:, col] = np.clip(((2.0 * _uniform(h, slot) - 1.0) * self.shift).astype(np.float32), lo, hi)
      if self.zoom > 0.0:
        lo, hi = _f32_inside(1.0 - self.zoom, 1.0 + self.zoom)
        clip[:, 2] = np.clip((1.0 + (2.0 * _uniform(h, _SLOT_ZOOM) - 1.0) * self.zoom).astype(np.float32), lo, hi)
      if self.flip > 0.0:
        clip[:, 3] = _uniform(h, _SLOT_FLIP) < self.flip
      if self.tjitter > 0.0:
        # walk the source frames: dropped, doubled or kept; the list is cut to len, or its last element repeated
        u = _uniform(h[clip_of], _SLOT_FRAME + t_of)
        counts = np.where(u < 0.5 * self.tjitter, 0, np.where(u < self.tjitter, 2, 1)).astype(np.int64)
        emitted = np.repeat(t_of, counts)                   # source frames in emission order, all clips back to back
        per_clip = np.add.reduceat(counts, offsets)         # (lens > 0: no empty segment)
        first = np.cumsum(per_clip) - per_clip
        pos = first[clip_of] + np.minimum(t_of, per_clip[clip_of] - 1)
        some = per_clip[clip_of] > 0
        tmap = np.where(some, emitted[np.where(some, pos, 0)] if len(emitted) else 0, 0).astype(np.int32)
      n_masks, width = self.tmask
      if n_masks > 0 and width > 0:
        w_most = np.minimum(width, lens // (2 * n_masks))   # N spans of at most len // (2N): at most half a clip
        for j in range(n_masks):
          w = np.floor(_uniform(h, _SLOT_MASK + 2 * j) * (w_most + 1)).astype(np.int64)
          w = np.minimum(w, w_most)
          start = np.floor(_uniform(h, _SLOT_MASK + 2 * j + 1) * (lens - w + 1)).astype(np.int64)
          start = np.minimum(start, lens - w)
          tmap[(t_of >= start[clip_of]) & (t_of < (start + w)[clip_of])] = -1
    return clip, tmap


# ---- landmark-space augmentation (include/lipreading_hip.h, "Landmark augmentation") ------------------
LMK_REC_WORDS = 16                            # eight-byte words of a clip's record
_LMK_DOMAIN = _U(0x6C6D6B5F61756721)          # the landmark stream's own domain constant: not AugmentSpec's draws
(_LSLOT_YAW, _LSLOT_PITCH, _LSLOT_ROLL, _LSLOT_SCALE, _LSLOT_EX, _LSLOT_EY, _LSLOT_SHIFT, _LSLOT_MIRROR,
 _LSLOT_KEY) = 0, 1, 2, 3, 4, 5, 6, 9, 10     # the three shifts are slots 6, 7, 8


class LandmarkAugmentSpec(object):
  """The landmark regime's policy: one 3x3 matrix, a shift and noise per CLIP, applied by lr_lmk_augment_f32 about the
  clip's centre c and in units of its RMS radius r.  mirror: probability of a left-right mirror; rot = (yaw, pitch,
  roll): the head turns by up to +-each, in degrees; scale: the face is scaled by a factor in [1 - scale, 1 + scale];
  stretch: x and y are stretched by factors in [1 - stretch, 1 + stretch] of their own; shift: the clip moves by up to
  +-shift * r along every axis; jitter: every output coordinate receives noise of standard deviation jitter * r; seed:
  the stream of draws."""

  FIELDS = ("mirror", "rot", "scale", "stretch", "shift", "jitter")
  LIMITS = {"mirror": 1.0, "scale": 0.5, "stretch": 0.25, "shift": 0.5, "jitter": 0.1}
  MAX_ROT = 45.0

  def __init__(self, mirror=0.0, rot=(0.0, 0.0, 0.0), scale=0.0, stretch=0.0, shift=0.0, jitter=0.0, seed=0):
    try:
      yaw, pitch, roll = rot
      self.rot = (float(yaw), float(pitch), float(roll))
    except (TypeError, ValueError):
      raise ValueError("rot must be (yaw, pitch, roll) or 'yaw/pitch/roll' in degrees, got %r" % (rot,))
    self.mirror, self.scale, self.stretch = float(mirror), float(scale), float(stretch)
    self.shift, self.jitter, self.seed = float(shift), float(jitter), int(seed)
    for name in ("mirror", "scale", "stretch", "shift", "jitter"):
      if not 0.0 <= getattr(self, name) <= self.LIMITS[name]:
        raise ValueError("%s must be in [0, %g], got %r" % (name, self.LIMITS[name], getattr(self, name)))
    if not all(0.0 <= a <= self.MAX_ROT for a in self.rot):
      raise ValueError("every angle of rot must be in [0, %g] degrees, got %r" % (self.MAX_ROT, rot))

  @classmethod
  def parse(cls, text, seed=0):
    """'mirror=0.5,rot=10/10/15,scale=0.1,stretch=0.05,shift=0.05,jitter=0.01' -> LandmarkAugmentSpec; '' -> None."""
    text = (text or "").strip()
    if not text:
      return None
    args = {}
    for item in text.split(","):
      key, eq, value = item.strip().partition("=")
      key, value = key.strip(), value.strip()
      if key not in cls.FIELDS or not eq:
        raise ValueError("unknown landmark augmentation %r (known: %s)" % (item.strip(), ", ".join(cls.FIELDS)))
      if key in args:
        raise ValueError("landmark augmentation %r is given twice" % key)
      try:
        if key == "rot":
          angles = tuple(float(a) for a in value.split("/"))
          if len(angles) != 3:
            raise ValueError(value)
          args[key] = angles
        else:
          args[key] = float(value)
      except ValueError:
        raise ValueError("cannot read %r as a value of %s" % (value, key))
    return cls(seed=seed, **args)

  def __str__(self):
    return "mirror=%r,rot=%r/%r/%r,scale=%r,stretch=%r,shift=%r,jitter=%r" % (
        (self.mirror,) + self.rot + (self.scale, self.stretch, self.shift, self.jitter))

  def __repr__(self):
    return "LandmarkAugmentSpec(%s, seed=%d)" % (str(self).replace(",", ", "), self.seed)

  def _key(self):
    return (self.mirror, self.rot, self.scale, self.stretch, self.shift, self.jitter, self.seed)

  def __eq__(self, other):
    return isinstance(other, LandmarkAugmentSpec) and self._key() == other._key()

  def __ne__(self, other):
    return not self == other

  def __hash__(self):
    return hash(self._key())

  @property
  def identity(self):
    return not (self.mirror > 0.0 or any(a > 0.0 for a in self.rot) or self.scale > 0.0 or self.stretch > 0.0 or
                self.shift > 0.0 or self.jitter > 0.0)

  def draw(self, pass_no, indices, lens):
    """The records of one batch: uint64 [B][16] — words 0-8 A row-major, 9-11 shift, 12 jitter, 13 mirror (float64
    bits), 14 the noise key, 15 zero.  A = s Rz(roll) Ry(yaw) Rx(pitch) diag(1 + e_x, 1 + e_y, 1) diag(-1 if mirrored
    else 1, 1, 1): the host folds everything linear into it.  Vectorised over the batch; sample b's record is a function
    of (seed, pass_no, indices[b], lens[b]) alone."""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    assert idx.shape == lens.shape
    B = len(lens)
    rec = np.zeros((B, LMK_REC_WORDS), np.float64)
    rec[:, [0, 4, 8]] = 1.0
    if self.identity:
      return rec.view(np.uint64)
    with np.errstate(over="ignore"):
      h = _mix(np.full(B, self.seed, dtype=np.int64).astype(np.uint64) ^ _LMK_DOMAIN)
      for key in (np.full(B, int(pass_no), dtype=np.int64), idx, lens):
        h = _absorb(h, key)

      def sym(slot, limit):                   # uniform in +-limit (exactly 0 for a limit of 0)
        return (2.0 * _uniform(h, slot) - 1.0) * limit if limit > 0.0 else np.zeros(B)

      yaw, pitch, roll = (np.deg2rad(sym(slot, limit)) for slot, limit in
                          zip((_LSLOT_YAW, _LSLOT_PITCH, _LSLOT_ROLL), self.rot))
      s = 1.0 + sym(_LSLOT_SCALE, self.scale)
      ex, ey = 1.0 + sym(_LSLOT_EX, self.stretch), 1.0 + sym(_LSLOT_EY, self.stretch)
      mirrored = _uniform(h, _LSLOT_MIRROR) < self.mirror if self.mirror > 0.0 else np.zeros(B, dtype=bool)
      shift = np.stack([sym(_LSLOT_SHIFT + k, self.shift) for k in range(3)], axis=1)
      key = _absorb(h, _LSLOT_KEY)
    one, zero = np.ones(B), np.zeros(B)

    def mat(*rows):
      return np.stack([np.stack(r, axis=1) for r in rows], axis=1)      # (B, 3, 3)

    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = mat((cr, -sr, zero), (sr, cr, zero), (zero, zero, one))
    Ry = mat((cy, zero, sy), (zero, one, zero), (-sy, zero, cy))
    Rx = mat((one, zero, zero), (zero, cp, -sp), (zero, sp, cp))
    diag = np.stack([ex * np.where(mirrored, -1.0, 1.0), ey, one], axis=1)
    A = s[:, None, None] * (Rz @ Ry @ Rx) * diag[:, None, :] + 0.0       # (+ 0.0: no negative zero)
    rec[:, :9] = A.reshape(B, 9)
    rec[:, 9:12] = shift
    rec[:, 12] = self.jitter
    rec[:, 13] = mirrored
    out = rec.view(np.uint64)
    out[:, 14] = key
    return out
