"""Prefetching batch loader: batch k+1 is gathered, uploaded and collated while the GPU runs step k.

`PrefetchLoader` yields what `BatchLoader(dataset, batch_size, make_collate_fn(device))` (or the pixel collate)
yields — the same batches in the same order, bit for bit — but takes the work in front of the step off the step's
stream and off the step's critical path:

  host stage    worker threads gather the samples of the next `depth` batches straight into a ring of `depth + 1`
                PINNED host slots (one contiguous slot per batch: frames or landmark rows, landmarks, offsets, lens),
                each sample copied once (numpy's copy releases the GIL), and build the padded chars and the lengths;
  device stage  the thread that iterates the loader uploads a ready slot with ONE asynchronous copy on the loader's
                own stream, collates it there in ONE launch (lr_lip_crop_collate_u8 / lr_collate_pad_f32) and records
                an event; the consumer's stream waits on that event (no host synchronisation).

With `crop="stable"` the pixel launch is lr_lip_stable_collate_u8 (the stabilised, roll-corrected window of
landmarks.lip_crop_stable), augmented or not; its workspace lies behind the slot's device bytes.

With `pose=PoseSpec(...)` (landmarks.py) the landmark launch is lr_lmk_pose_collate_f32 — every frame aligned to the
spec's canonical face — with the batch's frame map when the batch is augmented; its workspace and status words lie behind
the slot's device bytes as well.  A loader built without it issues the calls it always issued.

With `lmk_augment=LandmarkAugmentSpec(...)` (augment.py) the landmark regime's batches are also mirrored, turned, scaled,
stretched, shifted and jittered: lr_lmk_augment_f32, in place on the padded batch, behind whichever landmark collate ran.

With `augment=AugmentSpec(...)` (augment.py) a worker also draws the batch's augmentation records into the slot — they
ride the same upload — and the one launch is lr_lip_crop_collate_aug_u8 / lr_collate_pad_aug_f32, which applies them.
Lengths, labels, batch order and batch shapes are those of the un-augmented loader; `plain()` iterates the same
dataset, ring and stream with augmentation off (DESIGN.md "Clip augmentation").

Rules (DESIGN.md "Prefetching loader"):
  * no HIP call on a worker thread — workers touch host memory only; every enqueue, event record and event query is
    issued by the iterating thread between two steps, never while a step is being captured into a hipGraph;
  * a padded batch is an ordinary tensor of torch's allocator and stays valid for as long as the caller holds it; only
    the pinned slots and the ragged device staging are recycled, a slot only after the event behind its upload has
    completed;
  * a worker's exception is re-raised at the batch it belongs to; abandoning an iteration joins the workers; every
    blocking host wait has a time limit.

The host stage (`HostStage`) needs no GPU: it takes the buffer factory as a parameter.
"""
import queue
import threading
import time

import numpy as np
import torch

from . import _C

MAX_WORKERS = 8         # a GPU job may use 16 CPUs; never sized by os.cpu_count()
WAIT_SECONDS = 120.0    # upper bound of every blocking wait on the host
_ALIGN = 256            # every region of a slot starts on a 256-byte boundary (vector loads, int64 offsets)
LMK_REC_BYTES = 128     # a clip's landmark-augmentation record: 16 eight-byte words (augment.LMK_REC_WORDS)
DRAW_AHEAD = 16         # batches whose augmentation records ONE call of AugmentSpec.draw covers: a draw is some fifty
                        # numpy calls, each of which hands the GIL over and takes it back from the thread that launches
                        # the step, so the workers draw for many batches at once (DESIGN.md "Clip augmentation")


def _align(n):
  return (int(n) + _ALIGN - 1) // _ALIGN * _ALIGN


def batch_plan(n, batch_size):
  """Index ranges [(lo, hi)] of `BatchLoader`'s batches: consecutive, un-shuffled, a ragged last one."""
  assert batch_size > 0
  return [(lo, min(lo + batch_size, n)) for lo in range(0, n, batch_size)]


class PackedBatch(object):
  """What the host stage leaves in a slot: the byte offsets of its regions and the host half of the batch.

  pixels:    frames u8 [rows][3][H][W] | lmk f32 [rows][68][3] | offsets i64 [B] | lens i32 [B]
  landmarks: rows f32 [rows][feat]                             | offsets i64 [B] | lens i32 [B]
  augmented: ... | aug f32 [B][4] (pixels only) | tmap i32 [rows]     (AugmentSpec.draw's records)
  landmark-augmented: ... | lmk_aug u64 [B][16], the last region      (LandmarkAugmentSpec.draw's records)
  frame_lens / chars / char_lens: int64 numpy arrays, the values the plain collate functions return."""

  def __init__(self):
    self.index = self.slot = None
    self.pixels = False
    self.B = self.t_max = self.rows = self.nbytes = 0
    self.frames_off = self.lmk_off = self.offsets_off = self.lens_off = 0
    self.augmented = False
    self.aug_off = self.tmap_off = 0
    self.lmk_augmented = False
    self.lmk_aug_off = 0
    self.H = self.W = self.feat = 0
    self.tail = ()
    self.frame_lens = self.chars = self.char_lens = None

  def region(self, buf, name):
    """A numpy view of one region of `buf` (the uint8 array the batch was packed into)."""
    B, rows = self.B, self.rows
    if name == "frames":
      if self.pixels:
        return buf[self.frames_off:self.frames_off + rows * 3 * self.H * self.W].reshape(rows, 3, self.H, self.W)
      return buf[self.frames_off:self.frames_off + rows * self.feat * 4].view(np.float32).reshape(rows, self.feat)
    if name == "lmk":
      assert self.pixels
      return buf[self.lmk_off:self.lmk_off + rows * 68 * 3 * 4].view(np.float32).reshape(rows, 68, 3)
    if name == "offsets":
      return buf[self.offsets_off:self.offsets_off + B * 8].view(np.int64)
    if name == "lens":
      return buf[self.lens_off:self.lens_off + B * 4].view(np.int32)
    if name == "aug":
      assert self.augmented and self.pixels
      return buf[self.aug_off:self.aug_off + B * 16].view(np.float32).reshape(B, 4)
    if name == "tmap":
      assert self.augmented
      return buf[self.tmap_off:self.tmap_off + rows * 4].view(np.int32)
    if name == "lmk_aug":
      assert self.lmk_augmented
      return buf[self.lmk_aug_off:self.lmk_aug_off + B * LMK_REC_BYTES].view(np.uint64).reshape(B, LMK_REC_BYTES // 8)
    raise KeyError(name)


def _pad_chars(captions):
  """The host half of data.make_collate_fn: chars int64 (B, Cmax) PAD=0 and their lengths."""
  caps = [np.asarray(c, dtype=np.int64) for c in captions]
  char_lens = np.array([len(c) for c in caps], dtype=np.int64)
  chars = np.zeros((len(caps), int(char_lens.max())), dtype=np.int64)
  for i, c in enumerate(caps):
    chars[i, :len(c)] = c
  return chars, char_lens


def _aug_bytes(B, rows, pixels):
  """Bytes of the augmentation regions behind `lens`."""
  return (_align(B * 16) if pixels else 0) + _align(rows * 4)


def pack_batch(samples, pixels, buf, augment=None, pass_no=0, indices=None, records=None, lmk_augment=None,
               lmk_records=None):
  """Gather one batch into `buf` (1-D uint8 numpy array, a slot of the ring).  Host memory only.  Raises what the
  plain collate raises for a malformed batch (AssertionError), before anything is written.  augment: an AugmentSpec,
  whose draw for (pass_no, indices = the samples' dataset indices) follows `lens`; None: today's bytes.  records: that
  draw's (clip, tmap) if the caller has it already (a record depends on seed, pass, index and length only).
  lmk_augment: a LandmarkAugmentSpec, whose draw (lmk_records, if the caller has it already) lies in a region of its own
  behind all the others; None: no such region."""
  pb = PackedBatch()
  pb.pixels = bool(pixels)
  assert len(samples) > 0
  if pixels:
    assert all(len(x) == 2 and len(x[0]) == 2 for x in samples)          # data.make_pixel_collate_fn
    pairs, captions = zip(*samples)
    pix = [np.asarray(p[0]) for p in pairs]
    lmk = [np.asarray(p[1]) for p in pairs]
    H, W = pix[0].shape[2], pix[0].shape[3]
    assert all(p.dtype == np.uint8 and p.shape[1:] == (3, H, W) for p in pix)
    assert all(l.shape[0] == p.shape[0] and l.shape[1:] == (68, 3) for l, p in zip(lmk, pix))
    lens = np.array([len(p) for p in pix], dtype=np.int64)
    rows = int(lens.sum())
    pb.H, pb.W = int(H), int(W)
    pb.frames_off = 0
    pb.lmk_off = _align(rows * 3 * H * W)
    pb.offsets_off = pb.lmk_off + _align(rows * 68 * 3 * 4)
  else:
    assert all(len(x) == 2 for x in samples)                              # data.make_collate_fn
    seqs, captions = zip(*samples)
    pix = [np.asarray(s) for s in seqs]
    tail = pix[0].shape[1:]
    assert all(a.shape[1:] == tail for a in pix)                          # data.pad_frames
    lens = np.array([len(a) for a in pix], dtype=np.int64)
    rows = int(lens.sum())
    pb.tail = tuple(int(d) for d in tail)
    pb.feat = int(np.prod(tail)) if tail else 1
    pb.frames_off = 0
    pb.offsets_off = _align(rows * pb.feat * 4)
  pb.B, pb.rows, pb.t_max = len(samples), rows, int(lens.max())
  pb.lens_off = pb.offsets_off + _align(pb.B * 8)
  pb.nbytes = pb.lens_off + _align(pb.B * 4)
  if augment is not None:
    assert indices is not None and len(indices) == len(samples), "an augmented batch needs its dataset indices"
    pb.augmented = True
    pb.aug_off = pb.nbytes
    pb.tmap_off = pb.aug_off + (_align(pb.B * 16) if pixels else 0)
    pb.nbytes = pb.aug_off + _aug_bytes(pb.B, rows, pixels)
  if lmk_augment is not None:
    assert not pixels, "landmark augmentation belongs to the landmark regime"
    assert indices is not None and len(indices) == len(samples), "an augmented batch needs its dataset indices"
    pb.lmk_augmented = True
    pb.lmk_aug_off = pb.nbytes
    pb.nbytes = pb.lmk_aug_off + _align(pb.B * LMK_REC_BYTES)
  assert pb.nbytes <= buf.shape[0], "slot of %d bytes is too small for a batch of %d" % (buf.shape[0], pb.nbytes)
  offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
  frames = pb.region(buf, "frames")
  lmk_rows = pb.region(buf, "lmk") if pixels else None
  for b in range(pb.B):                      # every sample is copied (and converted) once, straight into the slot
    lo, n = int(offsets[b]), int(lens[b])
    if pixels:
      np.copyto(frames[lo:lo + n], pix[b])
      np.copyto(lmk_rows[lo:lo + n], lmk[b], casting="unsafe")             # as np.asarray(.., dtype=float32)
    else:
      np.copyto(frames[lo:lo + n], pix[b].reshape(n, pb.feat), casting="unsafe")
  pb.region(buf, "offsets")[:] = offsets
  pb.region(buf, "lens")[:] = lens
  if augment is not None:
    clip, tmap = augment.draw(pass_no, indices, lens) if records is None else records
    assert clip.shape == (pb.B, 4) and tmap.shape == (rows,)
    if pixels:
      pb.region(buf, "aug")[...] = clip       # (the landmark regime has no window to move: the map alone applies)
    pb.region(buf, "tmap")[:] = tmap
  if lmk_augment is not None:
    rec = lmk_augment.draw(pass_no, indices, lens) if lmk_records is None else lmk_records
    assert rec.shape == (pb.B, LMK_REC_BYTES // 8) and rec.dtype == np.uint64
    pb.region(buf, "lmk_aug")[...] = rec
  pb.frame_lens = lens
  pb.chars, pb.char_lens = _pad_chars(captions)
  return pb


def _slot_bytes(dataset, plan, pixels, augment=False, lmk_augment=False):
  """Bytes of the largest batch (the dataset is in memory): sizes only, the shape checks belong to pack_batch."""
  most = _ALIGN
  for lo, hi in plan:
    a = b = rows = 0
    for i in range(lo, hi):
      try:
        x = dataset[i][0]
        if pixels:
          a += int(np.asarray(x[0]).nbytes)
          b += int(np.asarray(x[1]).size) * 4
          rows += len(x[0])
        else:
          a += int(np.asarray(x).size) * 4
          rows += len(x)
      except Exception:     # a malformed sample: its batch raises when it is packed
        continue
    most = max(most, _align(a) + _align(b) + _align((hi - lo) * 8) + _align((hi - lo) * 4) +
               (_aug_bytes(hi - lo, rows, pixels) if augment else 0) +
               (_align((hi - lo) * LMK_REC_BYTES) if lmk_augment else 0))
  return most


def _max_rows(dataset, plan, pixels=True):
  """Frames of the largest batch (sizes only, as _slot_bytes)."""
  most = 1
  for lo, hi in plan:
    rows = 0
    for i in range(lo, hi):
      try:
        rows += len(dataset[i][0][0]) if pixels else len(dataset[i][0])
      except Exception:     # a malformed sample: its batch raises when it is packed
        continue
    most = max(most, rows)
  return most


def _plain_alloc(nbytes):
  return torch.empty(int(nbytes), dtype=torch.uint8)


def _pinned_alloc(nbytes):
  return torch.empty(int(nbytes), dtype=torch.uint8, pin_memory=True)


class _HostEpoch(object):
  """The workers of one pass over the dataset.  submit(slot) hands the next batch of the plan to a worker together
  with the slot it may fill; get(k) returns batch k's PackedBatch or re-raises its worker's exception."""

  def __init__(self, stage, augment=None, pass_no=0, lmk_augment=None):
    self._dataset, self._plan, self._pixels = stage.dataset, stage.plan, stage.pixels
    self._augment, self._lmk_augment, self._pass_no = augment, lmk_augment, int(pass_no)
    self._draw_lock = threading.Lock()
    self._drawn = {}                 # chunk of DRAW_AHEAD batches -> (first index, row starts, clip, tmap, lmk records)
    self._bufs = stage._np
    self._tasks = queue.Queue()
    self._cv = threading.Condition()
    self._results = {}
    self._stop = threading.Event()
    self.submitted = 0
    self.threads = [threading.Thread(target=self._work, name="lipreading-prefetch-%d" % i, daemon=True)
                    for i in range(stage.workers)]
    for t in self.threads:
      t.start()

  def _work(self):
    while True:
      task = self._tasks.get()
      if task is None or self._stop.is_set():
        return
      k, slot = task
      try:
        lo, hi = self._plan[k]
        drawn = self._augment is not None or self._lmk_augment is not None
        records, lmk_records = self._records(k) if drawn else (None, None)
        res = pack_batch([self._dataset[i] for i in range(lo, hi)], self._pixels, self._bufs[slot],
                         augment=self._augment, pass_no=self._pass_no, indices=range(lo, hi), records=records,
                         lmk_augment=self._lmk_augment, lmk_records=lmk_records)
        res.index, res.slot = k, slot
      except BaseException as exc:   # handed to the consumer, which raises it at batch k
        res = exc
      with self._cv:
        self._results[k] = res
        self._cv.notify_all()

  def _records(self, k):
    """Batch k's ((clip, tmap), landmark records), cut out of ONE draw of each policy for its chunk of DRAW_AHEAD
    batches (made by the worker that needs it first); None for a policy that is off.  (None, None) if the chunk cannot
    be drawn (a malformed sample somewhere in it): the batch then draws for itself, and the malformed batch raises when
    IT is packed."""
    c = k // DRAW_AHEAD
    with self._draw_lock:
      got = self._drawn.get(c, False)
      if got is False:
        try:
          b0, b1 = c * DRAW_AHEAD, min((c + 1) * DRAW_AHEAD, len(self._plan))
          lo, hi = self._plan[b0][0], self._plan[b1 - 1][1]
          lens = np.array([len(self._dataset[i][0][0]) if self._pixels else len(self._dataset[i][0])
                           for i in range(lo, hi)], dtype=np.int64)
          clip, tmap = (self._augment.draw(self._pass_no, range(lo, hi), lens) if self._augment is not None
                        else (None, None))
          rec = (self._lmk_augment.draw(self._pass_no, range(lo, hi), lens) if self._lmk_augment is not None
                 else None)
          got = (lo, np.concatenate([[0], np.cumsum(lens)]), clip, tmap, rec)
        except Exception:
          got = None
        self._drawn = {c2: v for c2, v in self._drawn.items() if c2 >= c - 1}   # workers are a few batches apart
        self._drawn[c] = got
    if got is None:
      return None, None
    first, starts, clip, tmap, rec = got
    lo, hi = self._plan[k]
    return ((clip[lo - first:hi - first], tmap[starts[lo - first]:starts[hi - first]]) if clip is not None else None,
            rec[lo - first:hi - first] if rec is not None else None)

  def submit(self, slot):
    if self._stop.is_set() or self.submitted >= len(self._plan):
      return False
    self._tasks.put((self.submitted, slot))
    self.submitted += 1
    return True

  def ready(self, k):
    with self._cv:
      return k in self._results

  def get(self, k, timeout=WAIT_SECONDS):
    assert k < self.submitted, "batch %d was never handed to a worker" % k
    with self._cv:
      if not self._cv.wait_for(lambda: k in self._results, timeout):
        raise TimeoutError("batch %d was not packed within %.0f s" % (k, timeout))
      res = self._results.pop(k)
    if isinstance(res, BaseException):
      raise res
    return res

  def close(self, timeout=WAIT_SECONDS):
    """Stop and join the workers (a worker finishes the sample copy it is in, nothing more)."""
    if self._stop.is_set() and not any(t.is_alive() for t in self.threads):
      return
    self._stop.set()
    for _ in self.threads:
      self._tasks.put(None)
    deadline = time.monotonic() + timeout
    for t in self.threads:
      t.join(max(0.0, deadline - time.monotonic()))
    alive = [t.name for t in self.threads if t.is_alive()]
    if alive:
      raise RuntimeError("prefetch workers did not stop within %.0f s: %s" % (timeout, ", ".join(alive)))


class HostStage(object):
  """Batch plan, ring of host slots and worker threads; no GPU needed.

  alloc(nbytes) -> 1-D uint8 CPU tensor: pinned for the GPU path, plain `torch.empty` for host-only use.  Iterating
  the stage yields the PackedBatch of every batch in order; a batch's slot goes back to the workers when the consumer
  asks for the next batch (PrefetchLoader drives the same workers but returns a slot only after its upload).

  augment: an AugmentSpec; every augmented pass draws with the next pass number (0, 1, ...; `set_pass` pins it), so two
  passes differ and a resumed run can repeat one.  A pass takes its number when it starts, completed or abandoned.
  lmk_augment: a LandmarkAugmentSpec (landmark regime); its records are drawn beside `augment`'s, with the same pass
  number."""

  def __init__(self, dataset, batch_size, pixels=False, depth=2, workers=2, alloc=None, augment=None,
               lmk_augment=None):
    assert depth >= 1 and workers >= 1
    self.dataset, self.batch_size, self.pixels = dataset, int(batch_size), bool(pixels)
    self.depth, self.workers = int(depth), min(int(workers), MAX_WORKERS)
    self.augment, self.lmk_augment, self.pass_no = augment, lmk_augment, 0
    self.plan = batch_plan(len(dataset), self.batch_size)
    self.slot_bytes = _slot_bytes(dataset, self.plan, self.pixels, augment is not None, lmk_augment is not None)
    alloc = alloc or _plain_alloc
    self.slots = [alloc(self.slot_bytes) for _ in range(self.depth + 1)]
    assert all(s.dtype == torch.uint8 and s.dim() == 1 and s.numel() >= self.slot_bytes and not s.is_cuda
               for s in self.slots)
    self._np = [s.numpy() for s in self.slots]
    self._epoch = None

  def __len__(self):
    return len(self.plan)

  def set_pass(self, n):
    """The number the next augmented pass draws with (resumption, tests)."""
    self.pass_no = int(n)

  def open(self, augmented=True):
    """Start the workers of a new pass (the previous pass, if it was abandoned, is shut down first).  augmented=False:
    a pass with augmentation off, which leaves the pass number alone."""
    self.close()
    if augmented and (self.augment is not None or self.lmk_augment is not None):
      self._epoch = _HostEpoch(self, self.augment, self.pass_no, self.lmk_augment)
      self.pass_no += 1
    else:
      self._epoch = _HostEpoch(self)
    return self._epoch

  def close(self):
    ep, self._epoch = self._epoch, None
    if ep is not None:
      ep.close()

  def threads_alive(self):
    ep = self._epoch
    return 0 if ep is None else sum(t.is_alive() for t in ep.threads)

  def __iter__(self):
    ep = self.open()
    try:
      for slot in range(len(self.slots)):
        ep.submit(slot)
      for k in range(len(self.plan)):
        pb = ep.get(k)
        yield pb
        ep.submit(pb.slot)
    finally:
      ep.close()
      if self._epoch is ep:
        self._epoch = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass


def _host_tensors(pb, pinned):
  """frame_lens, chars, char_lens as fresh int64 host tensors (pinned: the caller's .to(device, non_blocking=True) is
  then asynchronous) — views of ONE allocation that the batch owns; it is not part of the recycled slot."""
  B, C = pb.chars.shape
  t = torch.empty(B * (C + 2), dtype=torch.int64, pin_memory=pinned)
  a = t.numpy()
  a[:B] = pb.frame_lens
  a[B:2 * B] = pb.char_lens
  a[2 * B:].reshape(B, C)[...] = pb.chars
  return t[:B], t[2 * B:].view(B, C), t[B:2 * B]


class PrefetchLoader(object):
  """Drop-in for `BatchLoader(dataset, batch_size, make_collate_fn(device))` — with pixels=True for
  `make_pixel_collate_fn(device, size, margin)` — that prepares up to `depth` batches ahead of the consumer.

  Yields (frames f32 (B,Tmax,68,3) or clips u8 (B,Tmax,3,size,size) on `device`, frame_lens i64, chars i64 (B,Cmax)
  PAD=0, char_lens i64), the last three on the host (pinned).  Re-iterable; one pass at a time."""

  def __init__(self, dataset, batch_size, device, pixels=False, size=96, margin=0.3, depth=2, workers=2, alloc=None,
               augment=None, crop="box", extent=1.25, radius=2, pose=None, lmk_augment=None, mirror_perm=None):
    from .data import check_crop
    check_crop(crop)
    if pose is not None and pixels:
      raise ValueError("pose=%r normalises the landmark regime's batches; pixels=True has none (use crop=\"stable\")"
                       % (pose,))
    if lmk_augment is not None and pixels:
      raise ValueError("lmk_augment=%r augments the landmark regime's batches; pixels=True has none (use augment=)"
                       % (lmk_augment,))
    dev = torch.device(device)
    if dev.type != "cuda":
      raise _C.LipReadingHipError("collation runs on the MI355X only (no CPU fallback)")
    if dev.index is None:
      dev = torch.device("cuda", torch.cuda.current_device())
    self.dataset, self.batch_size, self.device = dataset, int(batch_size), dev
    self.pixels, self.size, self.margin = bool(pixels), int(size), float(margin)
    self.crop, self.extent, self.radius = crop, float(extent), int(radius)
    self.depth = int(depth)
    self._pinned = alloc is None
    self.augment, self.pose, self.lmk_augment = augment, pose, lmk_augment
    self._perm = None
    if lmk_augment is not None:
      from .landmarks import MIRROR_68, check_mirror_perm
      perm = MIRROR_68 if mirror_perm is None else mirror_perm
      self._perm = check_mirror_perm(perm, len(perm))
    self.host = HostStage(dataset, batch_size, pixels=pixels, depth=depth, workers=workers,
                          alloc=alloc or _pinned_alloc, augment=augment, lmk_augment=lmk_augment)
    with torch.cuda.device(dev):
      self._copy = torch.cuda.Stream(dev)
      # ragged device staging, one per slot: rewritten only by a later upload on the same stream
      # crop="stable": the poses' workspace lies behind the slot's bytes, so no batch allocates one
      self._work_bytes = 0
      if self.pixels and crop == "stable":
        self._work_bytes = int(_C.lib().lr_lip_stable_workspace_bytes(_max_rows(dataset, self.host.plan), self.radius))
        if not self._work_bytes:
          raise _C.LipReadingHipError("lr_lip_stable_workspace_bytes rejects radius=%r" % (radius,))
      # pose=: the rows' statistics and, behind them, the rows' status words
      self._status_off = 0
      if pose is not None:
        most = _max_rows(dataset, self.host.plan, pixels=False)
        self._status_off = _align(pose.workspace_bytes(most))
        if not self._status_off:
          raise _C.LipReadingHipError("lr_lmk_pose_workspace_bytes rejects %r" % (pose,))
        self._work_bytes = self._status_off + _align(most * 4)
      # lmk_augment=: the clips' statistics, behind pose's bytes; the permutation is uploaded here, once
      self._lmk_work_off = self._lmk_work_bytes = 0
      if lmk_augment is not None:
        from .landmarks import mirror_perm_on
        self._perm_dev = mirror_perm_on(self._perm, dev)
        self._lmk_work_off = self._work_bytes
        self._lmk_work_bytes = int(_C.lib().lr_lmk_augment_workspace_bytes(self.host.batch_size))
        if not self._lmk_work_bytes:
          raise _C.LipReadingHipError("lr_lmk_augment_workspace_bytes rejects B=%r" % (batch_size,))
        self._work_bytes += _align(self._lmk_work_bytes)
      self._stage = [torch.empty(self.host.slot_bytes + self._work_bytes, dtype=torch.uint8, device=dev)
                     for _ in self.host.slots]
    self._pending = [None] * len(self.host.slots)    # the event behind the last upload out of each slot
    from .landmarks import _eyes, _mouth
    self._mouth, self._eyes = _mouth, _eyes

  def __len__(self):
    return len(self.host)

  def close(self):
    self.host.close()

  @property
  def pass_no(self):
    return self.host.pass_no

  def set_pass(self, n):
    self.host.set_pass(n)

  def plain(self):
    """An iterable over the same dataset, ring and stream with augmentation off (scoring the training set on clean
    clips).  One pass at a time, as for the loader itself; it does not advance the pass number."""
    return _PlainPasses(self)

  def _enqueue(self, pb):
    """Upload slot -> staging, collate into a fresh padded batch, record the event.  Iterating thread only."""
    L = _C.lib()
    dev, slot = self.device, pb.slot
    with torch.cuda.device(dev), torch.cuda.stream(self._copy):
      stage = self._stage[slot]
      stage[:pb.nbytes].copy_(self.host.slots[slot][:pb.nbytes], non_blocking=True)    # the batch's ONE upload
      base, s = stage.data_ptr(), self._copy.cuda_stream
      if self.pixels and self.crop == "stable":
        out = torch.empty((pb.B, pb.t_max, 3, self.size, self.size), dtype=torch.uint8, device=dev)
        aug = (base + pb.aug_off, base + pb.tmap_off) if pb.augmented else (None, None)
        (ea, eb), work = self._eyes, self.host.slot_bytes     # slot_bytes is a multiple of 256
        _C.check(L.lr_lip_stable_collate_u8(base + pb.frames_off, base + pb.lmk_off, base + pb.offsets_off,
                                            base + pb.lens_off, aug[0], aug[1], out.data_ptr(), None, base + work,
                                            self._work_bytes, pb.B, pb.rows, pb.t_max, pb.H, pb.W, self.size, 68,
                                            self._mouth.start, self._mouth.stop, ea.start, ea.stop, eb.start, eb.stop,
                                            self.extent, self.radius, s), "lr_lip_stable_collate_u8")
      elif self.pixels and pb.augmented:
        out = torch.empty((pb.B, pb.t_max, 3, self.size, self.size), dtype=torch.uint8, device=dev)
        _C.check(L.lr_lip_crop_collate_aug_u8(base + pb.frames_off, base + pb.lmk_off, base + pb.offsets_off,
                                              base + pb.lens_off, base + pb.aug_off, base + pb.tmap_off, out.data_ptr(),
                                              pb.B, pb.t_max, pb.H, pb.W, self.size, 68, self._mouth.start,
                                              self._mouth.stop, self.margin, s), "lr_lip_crop_collate_aug_u8")
      elif self.pixels:
        out = torch.empty((pb.B, pb.t_max, 3, self.size, self.size), dtype=torch.uint8, device=dev)
        _C.check(L.lr_lip_crop_collate_u8(base + pb.frames_off, base + pb.lmk_off, base + pb.offsets_off,
                                          base + pb.lens_off, out.data_ptr(), pb.B, pb.t_max, pb.H, pb.W, self.size,
                                          68, self._mouth.start, self._mouth.stop, self.margin, s), "lr_lip_crop_collate_u8")
      elif self.pose is not None:
        spec, work = self.pose, self.host.slot_bytes          # slot_bytes is a multiple of 256
        if pb.tail != (spec.npts, 3):
          raise ValueError("pose normalisation takes (len, %d, 3) landmarks, got (len,) + %r" % (spec.npts, pb.tail))
        out = torch.empty((pb.B, pb.t_max) + pb.tail, dtype=torch.float32, device=dev)
        _C.check(L.lr_lmk_pose_collate_f32(base + pb.frames_off, base + pb.offsets_off, base + pb.lens_off,
                                           base + pb.tmap_off if pb.augmented else None,
                                           spec.template_on(dev).data_ptr(), spec.rigid_ptr, len(spec.rigid),
                                           out.data_ptr(), None, base + work + self._status_off, base + work,
                                           self._status_off, pb.B, pb.rows, pb.t_max, spec.npts, spec.radius, spec.flags,
                                           s), "lr_lmk_pose_collate_f32")
      else:
        out = torch.empty((pb.B, pb.t_max, pb.feat), dtype=torch.float32, device=dev)
        if pb.augmented:
          _C.check(L.lr_collate_pad_aug_f32(base + pb.frames_off, base + pb.offsets_off, base + pb.lens_off,
                                            base + pb.tmap_off, out.data_ptr(), pb.B, pb.t_max, pb.feat, s),
                   "lr_collate_pad_aug_f32")
        else:
          _C.check(L.lr_collate_pad_f32(base + pb.frames_off, base + pb.offsets_off, base + pb.lens_off,
                                        out.data_ptr(), pb.B, pb.t_max, pb.feat, s), "lr_collate_pad_f32")
        out = out.reshape((pb.B, pb.t_max) + pb.tail)
      if pb.lmk_augmented:                                    # in place, behind whichever landmark collate ran
        if pb.tail != (len(self._perm), 3):
          raise ValueError("landmark augmentation takes (len, %d, 3) landmarks, got (len,) + %r"
                           % (len(self._perm), pb.tail))
        work = base + self.host.slot_bytes + self._lmk_work_off
        _C.check(L.lr_lmk_augment_f32(out.data_ptr(), base + pb.lens_off, base + pb.lmk_aug_off,
                                      self._perm_dev.data_ptr(), out.data_ptr(), None, work, self._lmk_work_bytes, pb.B,
                                      pb.t_max, len(self._perm), s), "lr_lmk_augment_f32")
      event = torch.cuda.Event()
      event.record(self._copy)
    self._pending[slot] = event
    return out, event, _host_tensors(pb, self._pinned)

  def _recycle(self, ep, busy, block=False):
    """Slots whose upload (and collate) has completed go back to the workers.  block: wait, with a time limit, until
    at least one has."""
    deadline = time.monotonic() + WAIT_SECONDS
    while True:
      recycled = 0
      for slot in list(busy):
        ev = self._pending[slot]
        if ev is None or ev.query():
          self._pending[slot] = None
          busy.remove(slot)
          ep.submit(slot)
          recycled += 1
      if not block or recycled:
        return
      assert busy, "no slot is being uploaded and none is with a worker"
      if time.monotonic() > deadline:
        raise TimeoutError("no upload of the prefetch ring completed within %.0f s" % WAIT_SECONDS)
      time.sleep(1e-4)

  def __iter__(self):
    return self._passes(True)

  def _passes(self, augmented):
    ep = self.host.open(augmented)
    try:
      nb = len(self.host.plan)
      busy = list(range(len(self._pending)))     # slots not with a worker (an abandoned pass may have left events)
      inflight = {}
      enq = 0                                    # next batch to enqueue on the device
      failed = None                              # the exception of a batch ahead of the consumer
      for k in range(nb):
        self._recycle(ep, busy)
        while ep.submitted <= k:                 # every slot is still being uploaded: wait for one
          self._recycle(ep, busy, block=True)
        # batch k itself (the first call of a pass primes the pipe), then whatever is ready of the batches behind it
        while enq < nb and (enq <= k or (failed is None and enq <= k + self.depth and enq < ep.submitted
                                         and ep.ready(enq))):
          try:
            if failed is not None:
              raise failed
            pb = ep.get(enq)
          except BaseException as exc:           # a worker's exception belongs to ITS batch: raised when k gets there
            if enq <= k:
              raise
            failed = exc
            break
          inflight[enq] = self._enqueue(pb)
          busy.append(pb.slot)
          enq += 1
        out, event, (frame_lens, chars, char_lens) = inflight.pop(k)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(event)                    # device-side wait only
        out.record_stream(cur)                   # allocated under the copy stream, consumed on this one
        yield out, frame_lens, chars, char_lens
    finally:
      ep.close()
      if self.host._epoch is ep:
        self.host._epoch = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass


class _PlainPasses(object):
  """PrefetchLoader.plain(): the loader's batches with augmentation off."""

  def __init__(self, loader):
    self.loader = loader

  def __len__(self):
    return len(self.loader)

  def __iter__(self):
    return self.loader._passes(False)
