"""Train / eval loops — the caller contract of `src/train/train_better_model.py` (train :7,
eval :89) on the MI355X path.

`train(encoder, decoding_step, data_loader, opt, device, char2idx, teacher_forcing_ratio,
grad_norm)` keeps the reference's argument meaning.  Differences, all about not stalling the
GPU: the framing asserts (:26-33) run on the host copies the loader hands over; the CTC loss
uses the device-side status flag instead of a `None` return, so a skipped batch costs no
device->host round trip (the optimiser kernel honours the flag); losses are accumulated on the
device and read once per epoch.  `decoding_step=None` runs the encoder+CTC path alone — the
path BASELINE.json's north_star names; with a `CharDecodingStep` the attention decoder loop
(:56-65) runs as one fused enqueue per batch (lipreading_amd/attention_decoder.py).
"""
import contextlib
import os

import torch

from .encoder import VideoEncoder as _VideoEncoder

from . import _C
from .ctc import ctc_loss_prepared, ctc_loss_with_status, prepare_ctc_inputs
from .data import BOS, EOS, PAD, host_max_len
from .optim import FusedAdam


def _check_framing(chars, char_lens, frame_lens, char2idx, use_ctc, in_eval=False):
  """train_better_model.py:26-33.  The loader hands chars / lengths over on the HOST (data.py's
  collate, as the reference's does), so the asserts cost no device round trip; a caller that passes
  device tensors pays one copy here.  The ascending-length requirement is ctc_loss.py:39's, so it is
  only checked when the CTC loss will run."""
  if chars.is_cuda or char_lens.is_cuda or frame_lens.is_cuda:
    chars, char_lens, frame_lens = chars.cpu(), char_lens.cpu(), frame_lens.cpu()
  assert (chars[:, 0].squeeze() == char2idx[BOS]).all()
  assert (chars.gather(1, (char_lens - 1).unsqueeze(dim=1)).squeeze() == char2idx[EOS]).all()
  if use_ctc and not in_eval:
    # (the reference's eval does not assert this, train_better_model.py:100-106: a caption longer than its clip makes
    # ctc_loss skip the sample there, and does so here)
    assert (frame_lens >= char_lens).all()  # otherwise ctc loss will produce inf
  labels = chars[:, 1:]
  label_lens = char_lens - 1
  assert (labels != char2idx[PAD]).sum() == label_lens.sum()
  if use_ctc:
    assert (frame_lens[1:] - frame_lens[:-1] >= 0).all()  # ctc_loss.py:39


class _NLLMeanFunction(torch.autograd.Function):
  """train_better_model.py:62,65 in two launches: sum over the decoder steps of nll_loss(ignore_index=PAD,
  reduction='sum') divided by (labels != PAD).sum().  log_probs (B, L, V); labels = a view of chars[:, 1:]
  whose first L columns are the steps' labels (int64, any row stride)."""

  @staticmethod
  def forward(ctx, log_probs, labels, pad):
    B, L, V = log_probs.shape
    lp = log_probs.contiguous()
    assert labels.dtype == torch.int64 and labels.stride(1) == 1 and labels.shape[0] == B and labels.shape[1] >= L
    out2 = torch.empty(2, dtype=torch.float32, device=lp.device)
    _C.check(_C.lib().lr_nll_mean_forward(lp.data_ptr(), labels.data_ptr(), labels.stride(0), L, int(pad),
                                          out2.data_ptr(), B * L, V, _C.stream_handle()), "lr_nll_mean_forward")
    ctx.save_for_backward(labels, out2)
    ctx.cfg = (B, L, V, int(pad))
    return out2[0]

  @staticmethod
  def backward(ctx, g):
    labels, out2 = ctx.saved_tensors
    B, L, V, pad = ctx.cfg
    g = g.reshape(1).to(torch.float32).contiguous()
    d_lp = torch.empty((B, L, V), dtype=torch.float32, device=out2.device)
    _C.check(_C.lib().lr_nll_mean_backward(labels.data_ptr(), labels.stride(0), L, pad, out2.data_ptr(), g.data_ptr(),
                                           d_lp.data_ptr(), B * L, V, _C.stream_handle()), "lr_nll_mean_backward")
    return d_lp, None, None


def decoder_nll(log_probs, labels, pad):
  """decoder_loss of train_better_model.py:62-65 from the (B, L, V) log-probs of the loop (any V)."""
  return _NLLMeanFunction.apply(log_probs, labels, pad)


def decoder_nll_sum(log_probs, labels, pad):
  """(sum of -log_probs[label] over the non-PAD steps, their count): eval adds the sums over the batches and divides
  once (train_better_model.py:127,138).  No gradient."""
  B, L, V = log_probs.shape
  lp = log_probs.contiguous()
  assert labels.dtype == torch.int64 and labels.stride(1) == 1 and labels.shape[0] == B and labels.shape[1] >= L
  out3 = torch.empty(3, dtype=torch.float32, device=lp.device)
  _C.check(_C.lib().lr_nll_forward3(lp.data_ptr(), labels.data_ptr(), labels.stride(0), L, int(pad), out3.data_ptr(),
                                    B * L, V, _C.stream_handle()), "lr_nll_forward3")
  return out3[2], out3[1]


class _Held(object):
  """`with _Held(syncs):` = every GradSync in `syncs` on hold(): gradients that become ready inside launch no
  collective (a collective is never captured into a hipGraph, and a replay fires no hooks at all); the buckets
  go out when the sync is called after the step."""

  def __init__(self, syncs):
    self._cms = [s.hold() for s in syncs if s is not None and hasattr(s, "hold")]

  def __enter__(self):
    for cm in self._cms:
      cm.__enter__()

  def __exit__(self, *exc):
    for cm in reversed(self._cms):
      cm.__exit__(*exc)
    return False


# what the last train() epoch skipped: {"batches", "skipped", "recurrence_faults"} (None before the first epoch)
last_epoch_stats = None

_ONES = {}


def _one(device):
  """A cached scalar 1 on `device`: the root gradient of loss.backward() (autograd otherwise fills a fresh
  ones_like tensor every step — one more launch)."""
  key = (device.type, device.index)
  t = _ONES.get(key)
  if t is None:
    t = _ONES[key] = torch.ones((), dtype=torch.float32, device=device)
  return t


class StepGraphs(object):
  """hipGraph capture of the optimisation step, cached per batch shape.

  A step is a few hundred short launches whose shapes depend only on (B, Tmax, Lmax): the collate
  function already pads every batch to those, so the launch sequence of a shape is recorded ONCE and
  replayed for every later batch of that shape (inputs are copied into the graph's static buffers; the
  loss / status tensors a replay returns are the graph's static outputs — consume them, e.g. `sum +=
  loss`, before the next step of the same shape).  The first `warmup` steps of a shape run eagerly on a
  side stream (allocator warm-up, as capture requires), the next one is captured, the rest replay.
  Same kernels in the same order on the same data: results are bit-identical to eager launches.

  What is captured: zero_grad -> forward -> loss(es) -> backward, plus clip + Adam when no gradient
  exchange sits between them (a collective is never captured: with `grad_sync` the exchange and the
  optimiser run eagerly after the replay).  Steps whose launch sequence depends on host randomness (a
  decoder loop with sampled inputs, teacher_forcing_ratio < 1) are not graphed."""

  def __init__(self, max_entries=16, warmup=2, enabled=True):
    self.max_entries, self.warmup, self.enabled = max_entries, warmup, enabled
    self._entries = {}     # key -> dict(static=..., count=int, graph=CUDAGraph|None, out=...)
    self._failed = set()   # shapes whose capture failed once: eager launches from then on, no retry
    self.replays = 0
    self.captures = 0

  def reset(self):
    """Drop every captured graph (their launch sequences are stale: e.g. after the recurrence fell back to the step
    kernels); shapes are captured again on their next steps."""
    self._entries.clear()
    self._failed.clear()

  def staging_buffers(self):
    """The static input tensors of the most recently used shape (None before its first step): a loader can write
    the next batch of that shape straight into them (same stream) and hand THEM to the step, which then skips
    its device-to-device staging copy of every input."""
    if not self._entries:
      return None
    return next(reversed(self._entries.values()))["static"]

  def run(self, key, inputs, body, capturable=True):
    """inputs: tuple of device tensors; body(*static_inputs) -> tuple of tensors.  Returns body's
    result for these inputs (from a replay when a graph for `key` exists)."""
    if not (self.enabled and capturable) or key in self._failed:
      return body(*inputs)
    e = self._entries.pop(key, None)
    if e is None:
      if self.max_entries <= 0:
        return body(*inputs)
      while len(self._entries) >= self.max_entries:   # least recently used shape goes (its pool is freed)
        self._entries.pop(next(iter(self._entries)))
      e = dict(static=tuple(torch.empty_like(t) for t in inputs), count=0, graph=None, out=None)
    self._entries[key] = e                            # most recently used = last
    for dst, src in zip(e["static"], inputs):
      # a caller that stages its batches straight into the graph's buffers (staging_buffers) passes them back:
      # nothing to copy
      if dst.data_ptr() != src.data_ptr():
        dst.copy_(src, non_blocking=True)
    if e["graph"] is not None:
      e["graph"].replay()
      self.replays += 1
      return e["out"]
    e["count"] += 1
    if e["count"] <= self.warmup:
      side = torch.cuda.Stream()
      side.wait_stream(torch.cuda.current_stream())
      with torch.cuda.stream(side):
        out = body(*e["static"])
      torch.cuda.current_stream().wait_stream(side)
      return out
    try:
      torch.cuda.synchronize()
      graph = torch.cuda.CUDAGraph()
      # thread_local: another thread (RCCL's watchdog) may touch the runtime while this one captures
      with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out = body(*e["static"])
    except Exception as exc:       # keep training: this shape stays on eager launches
      torch.cuda.synchronize()
      self._entries.pop(key, None)
      self._failed.add(key)
      print("note: hipGraph capture failed for step shape %r (%s: %s); eager launches" % (key, type(exc).__name__, exc))
      return body(*inputs)
    graph.replay()                 # capture records, it does not run
    e["graph"], e["out"] = graph, out
    self.captures += 1
    return out


class RecurrenceWatch(object):
  """Keeps a run alive when the one-launch recurrences cannot run on this device.

  A pair / cluster recurrence needs all of its workgroups resident together (one per compute unit); when they are not
  — compute units held by another process or by a long foreign kernel — its members time out, the device-side fault
  word makes the step a skipped one (include/lipreading_hip.h), and the NEXT step would do the same, a few tenths
  of a second each: a run that skips every batch.  The reference's contract is skip a bad batch and keep training
  (src/train/train_better_model.py:49-50), so after `limit` consecutive faulted steps this switches every recurrence
  to the per-step kernels for the rest of the process (lr_rnn_one_launch_enable(0)), says so once, and drops the
  captured hipGraphs (`graphs`), whose launch sequences are stale.

  No host round trip in the step: after a step, the step's fault flag is exported on the stream and copied to pinned
  memory asynchronously; the copy is looked at once it has landed, a step or two later.  Only when the host has run
  more than `lag` steps ahead of an unobserved flag does it wait for it (the device still has those steps queued, so
  nothing idles: this bounds the host's run-ahead, as a healthy loop's own `.item()` reads would)."""

  def __init__(self, device, limit=3, lag=2):
    self.limit, self.run, self.tripped, self.lag = int(limit), 0, False, int(lag)
    n = self.lag + 2
    self._dev = torch.zeros(n, 2, dtype=torch.int32, device=device)
    self._host = torch.zeros(n, 2, dtype=torch.int32).pin_memory()
    self._pending = []          # (slot, event) of the steps not yet observed, oldest first
    self._step = 0

  def _observe(self, graphs):
    slot, _ = self._pending.pop(0)
    self.run = self.run + 1 if int(self._host[slot, 1]) < 0 else 0
    if self.run < self.limit:
      return False
    self.tripped = True
    del self._pending[:]
    torch.cuda.synchronize()
    _C.lib().lr_rnn_one_launch_enable(0)
    if graphs is not None:
      graphs.reset()
    import warnings
    warnings.warn("lipreading_amd: the one-launch recurrence timed out in %d consecutive steps (its workgroups were "
                  "not resident together: are this GPU's compute units shared?); every recurrence runs on the "
                  "per-step kernels from here on (slower, same results)" % self.run)
    return True

  def after_step(self, graphs=None):
    """Call once per optimisation step, after it was enqueued.  Returns True when the fall-back was just taken."""
    if self.tripped or not _C.lib().lr_rnn_one_launch_enabled():
      return False
    while self._pending:
      _, ev = self._pending[0]
      if not ev.query():
        if len(self._pending) <= self.lag:
          break                 # not landed yet, and the host is not far ahead: look again after the next step
        ev.synchronize()
      if self._observe(graphs):
        return True
    slot = self._step % self._dev.shape[0]
    self._step += 1
    _C.check(_C.lib().lr_fault_export(None, self._dev[slot].data_ptr(), _C.stream_handle()), "lr_fault_export")
    self._host[slot].copy_(self._dev[slot], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    self._pending.append((slot, ev))
    return False


def _roll_faults(device):
  """Outside a training step (eval, greedy decoding) nothing rolls the fault words: do it here, so that a time-out of
  an earlier batch does not mark every later one (lr_step_begin with an empty gradient buffer)."""
  _C.check(_C.lib().lr_step_begin(None, 0, None, _C.stream_handle()), "lr_step_begin")


def _fault_keep(flag2):
  """1 if no one-launch recurrence has timed out since the last roll, else 0 — a device scalar, no host read."""
  _C.check(_C.lib().lr_fault_export(None, flag2.data_ptr(), _C.stream_handle()), "lr_fault_export")
  return (flag2[1] == 0)


def ctc_step(encoder, opt, frames, frame_lens, chars, char_lens, grad_norm=None, max_len=None,
             grad_sync=None, graphs=None):
  """One encoder+CTC optimisation step with no host synchronisation.

  labels = chars[:,1:], label_lens = char_lens-1 (:31-32); encoder (:46); ctc_loss 'mean' (:48);
  zero_grad + backward (:67,:74); clip (:78); opt.step (:80).  `opt` is a FusedAdam; `grad_sync`
  (optional) is called between backward and the optimiser — the data-parallel all-reduce.
  Returns (loss, status) device tensors; status == 1 marks a batch the reference skips."""
  whole = grad_sync is None      # nothing between backward and the optimiser: one graph for the step

  def body(frames, frame_lens, chars, char_lens):
    # labels = chars[:, 1:] + 1, label_lens = char_lens - 1 and the int32 lengths in one launch; the encoder takes
    # the int32 frame lengths as they are
    fused_prep = (chars.dtype == torch.int64 and frame_lens.dtype == torch.int64 and char_lens.dtype == torch.int64
                  and chars.dim() == 2 and chars.stride(1) == 1)
    if fused_prep:   # ... and in the SAME launch as zero_grad (lr_step_begin_ctc)
      labels_p1, frame_lens32, label_lens32 = opt.zero_grad_and_prepare_ctc(chars, frame_lens, char_lens)
    else:
      opt.zero_grad()
    # (the CTC-only step never reads the encoder's final states: they are not extracted)
    log_probs, _, _ = encoder(frames, frame_lens32 if fused_prep else frame_lens, max_len=max_len,
                              need_final_state=False)
    if fused_prep:
      loss, status, _ = ctc_loss_prepared(log_probs, labels_p1, frame_lens32, label_lens32, 'mean')
    else:
      loss, status, _ = ctc_loss_with_status(log_probs, chars[:, 1:], frame_lens, char_lens - 1, 'mean')
    if grad_sync is not None and hasattr(grad_sync, "set_status"):
      grad_sync.set_status(status)   # (the bucket that carries the skip / fault words may leave during backward)
    loss.backward(_one(loss.device))
    if whole:
      opt.step(grad_norm=grad_norm, grad_scale=1.0, skip=status)
    return loss.detach(), status

  dev = frames.device
  inputs = (frames, frame_lens.to(dev), chars.to(dev), char_lens.to(dev))
  if graphs is None:
    loss, status = body(*inputs)
  else:
    # a graph bakes max_len in: it must be the padded length itself
    ml = frames.shape[1] if max_len is None else int(max_len)
    # (the learning rate is a by-value kernel argument: part of what a graph bakes in)
    key = ("ctc", id(encoder), id(opt), opt.lr, tuple(frames.shape), str(frames.dtype), tuple(chars.shape), ml,
           grad_norm, whole)
    with _Held((grad_sync,)):   # (an overlapping GradSync must not exchange from inside a capture)
      loss, status = graphs.run(key, inputs, body, capturable=(ml == frames.shape[1]))
  if not whole:
    scale = grad_sync(status)
    opt.step(grad_norm=grad_norm, grad_scale=scale, skip=status, dist_words=getattr(grad_sync, "dist_words", None),
             world=getattr(grad_sync, "world", 1))
  return loss, status


def mwer_step(encoder, opt, mwer, frames, frame_lens, chars, char_lens, grad_norm=None, max_len=None, ctc_weight=0.01,
              grad_sync=None):
  """One encoder+CTC optimisation step on the N-best expected risk, anchored by the CTC likelihood:
  loss = mwer(log_probs) + ctc_weight * ctc_loss('mean') (lipreading_amd/mwer.py).  `mwer` is an
  mwer.MWERLoss over ctc_labels(char2idx); the references are the CTC labels themselves (chars[:, 1:] + 1).

  Eager, and without a host read: search -> score -> loss -> backward -> Adam are all enqueued; Adam is skipped on the
  device when either loss reports a batch to skip (the OR of the two status words) or a recurrence timed out (the
  fault word, inside FusedAdam.step as in ctc_step).  Returns (expected risk, ctc loss, status, info): device tensors,
  `info` the MWERLoss's dict plus the step's `log_probs` (detached)."""
  if grad_sync is not None:
    raise NotImplementedError("data-parallel MWER is not built: the N-best lists differ from rank to rank and the "
                              "step has no exchange for its skip word; run mwer_step in a single process")
  dev = frames.device
  frame_lens, chars, char_lens = frame_lens.to(dev), chars.to(dev), char_lens.to(dev)
  if (chars.dtype == torch.int64 and frame_lens.dtype == torch.int64 and char_lens.dtype == torch.int64
      and chars.dim() == 2 and chars.stride(1) == 1):
    labels_p1, frame_lens32, label_lens32 = opt.zero_grad_and_prepare_ctc(chars, frame_lens, char_lens)
  else:
    opt.zero_grad()
    labels_p1 = (chars[:, 1:] + 1).to(torch.int32).contiguous()
    frame_lens32, label_lens32 = frame_lens.to(torch.int32), (char_lens - 1).to(torch.int32)
  log_probs, _, _ = encoder(frames, frame_lens32, max_len=max_len, need_final_state=False)
  ctc, ctc_status, _ = ctc_loss_prepared(log_probs, labels_p1, frame_lens32, label_lens32, 'mean')
  risk, mwer_status, info = mwer(log_probs, frame_lens32, labels_p1, label_lens32)
  status = ctc_status | mwer_status
  info["log_probs"] = log_probs.detach().clone()   # (a copy: the encoder may reuse the buffer in its backward)
  (risk + ctc_weight * ctc).backward(_one(dev))
  opt.step(grad_norm=grad_norm, grad_scale=1.0, skip=status)
  return risk.detach(), ctc.detach(), status, info


def train_mwer(encoder, data_loader, opt, device, char2idx, mwer, grad_norm=None, ctc_weight=0.01):
  """An epoch of mwer_step over `data_loader`: the encoder+CTC branch of train() with the N-best expected risk as the
  objective.  Prints and returns (mean expected risk, mean CTC loss) over len(data_loader); a skipped batch adds 0 to
  both, as in train()."""
  assert encoder.enable_ctc, "MWER trains the CTC head: the encoder must have enable_ctc=True"
  assert isinstance(opt, FusedAdam), "opt must be lipreading_amd.optim.FusedAdam"
  device = torch.device(device)
  encoder.train()
  risk_sum = torch.zeros((), dtype=torch.float32, device=device)
  ctc_sum = torch.zeros((), dtype=torch.float32, device=device)
  skipped_before = opt.skipped_steps()
  watch = RecurrenceWatch(device)
  for frames, frame_lens, chars, char_lens in data_loader:
    _check_framing(chars, char_lens, frame_lens, char2idx, True)
    max_len = host_max_len(frame_lens)
    frames, chars = frames.to(device, non_blocking=True), chars.to(device, non_blocking=True)
    frame_lens_d, char_lens_d = frame_lens.to(device, non_blocking=True), char_lens.to(device, non_blocking=True)
    risk, ctc, status, _ = mwer_step(encoder, opt, mwer, frames, frame_lens_d, chars, char_lens_d, grad_norm=grad_norm,
                                     max_len=max_len, ctc_weight=ctc_weight)
    keep = status.reshape(()) == 0
    risk_sum += torch.where(keep, risk, torch.zeros_like(risk))
    ctc_sum += torch.where(keep, ctc, torch.zeros_like(ctc))
    watch.after_step(None)
  avg_risk = (risk_sum / len(data_loader)).item()
  avg_ctc = (ctc_sum / len(data_loader)).item()
  global last_epoch_stats
  faults = int(_C.lib().lr_rnn_pair_errors())
  last_epoch_stats = {"batches": len(data_loader), "skipped": opt.skipped_steps() - skipped_before,
                      "recurrence_faults": faults}
  if last_epoch_stats["skipped"] or faults:
    print("\tSkipped batches: %(skipped)d of %(batches)d (recurrence time-outs: %(recurrence_faults)d)"
          % last_epoch_stats)
  print(f'\tTraining expected risk: {avg_risk}')
  print(f'\tTraining ctc_loss: {avg_ctc}')
  return avg_risk, avg_ctc


def transducer_step(encoder, head, opts, frames, frame_lens, chars, char_lens, grad_norm=None, max_len=None,
                    ctc_weight=0.3, grad_sync=None):
  """One optimisation step of an encoder and its transducer.TransducerHead:
  loss = rnnt + ctc_weight * ctc_loss('mean') when the encoder has a CTC head and ctc_weight > 0, else the transducer
  loss alone.  The labels are the CTC labels (chars[:, 1:] + 1).  opts = (the encoder's FusedAdam, the head's).

  Eager, and without a host read: both Adams are skipped on the device when either loss reports a batch to skip (the
  OR of the status words) or a recurrence timed out.  Returns (transducer loss, ctc loss or None, status, info):
  device tensors, `info` the head's dict (nll, sample_status)."""
  if grad_sync is not None:
    raise NotImplementedError("data-parallel transducer steps are not built: the step has no exchange for its skip "
                              "word; run transducer_step in a single process")
  dev = frames.device
  frame_lens, chars, char_lens = frame_lens.to(dev), chars.to(dev), char_lens.to(dev)
  if (chars.dtype == torch.int64 and frame_lens.dtype == torch.int64 and char_lens.dtype == torch.int64
      and chars.dim() == 2 and chars.stride(1) == 1):
    labels_p1, frame_lens32, label_lens32 = opts[0].zero_grad_and_prepare_ctc(chars, frame_lens, char_lens)
  else:
    opts[0].zero_grad()
    labels_p1 = (chars[:, 1:] + 1).to(torch.int32).contiguous()
    frame_lens32, label_lens32 = frame_lens.to(torch.int32), (char_lens - 1).to(torch.int32)
  opts[1].zero_grad()
  out = encoder(frames, frame_lens32, max_len=max_len, need_final_state=False)
  has_ctc = bool(getattr(encoder, "enable_ctc", False))
  hidden = out[1] if has_ctc else out[0]
  rnnt, status, info = head.loss(hidden, frame_lens32, labels_p1, label_lens32, 'mean')
  total, ctc = rnnt, None
  if has_ctc and ctc_weight > 0:
    ctc, ctc_status, _ = ctc_loss_prepared(out[0], labels_p1, frame_lens32, label_lens32, 'mean')
    status = status | ctc_status
    total = rnnt + ctc_weight * ctc
  total.backward(_one(dev))
  _step_all(opts, grad_norm, status)
  return rnnt.detach(), None if ctc is None else ctc.detach(), status, info


def train_transducer(encoder, head, data_loader, opts, device, char2idx, grad_norm=None, ctc_weight=0.3):
  """An epoch of transducer_step over `data_loader`.  Prints and returns (mean transducer loss, mean CTC loss) over
  len(data_loader); a skipped batch adds 0 to both, as in train()."""
  assert all(isinstance(o, FusedAdam) for o in opts) and len(opts) == 2, "opts: the encoder's FusedAdam and the head's"
  device = torch.device(device)
  encoder.train()
  head.train()
  use_ctc = bool(getattr(encoder, "enable_ctc", False)) and ctc_weight > 0
  rnnt_sum = torch.zeros((), dtype=torch.float32, device=device)
  ctc_sum = torch.zeros((), dtype=torch.float32, device=device)
  skipped_before = opts[0].skipped_steps()
  watch = RecurrenceWatch(device)
  for frames, frame_lens, chars, char_lens in data_loader:
    _check_framing(chars, char_lens, frame_lens, char2idx, use_ctc)
    max_len = host_max_len(frame_lens)
    frames, chars = frames.to(device, non_blocking=True), chars.to(device, non_blocking=True)
    frame_lens_d, char_lens_d = frame_lens.to(device, non_blocking=True), char_lens.to(device, non_blocking=True)
    rnnt, ctc, status, _ = transducer_step(encoder, head, opts, frames, frame_lens_d, chars, char_lens_d,
                                           grad_norm=grad_norm, max_len=max_len, ctc_weight=ctc_weight)
    keep = status.reshape(()) == 0
    rnnt_sum += torch.where(keep, rnnt, torch.zeros_like(rnnt))
    if ctc is not None:
      ctc_sum += torch.where(keep, ctc, torch.zeros_like(ctc))
    watch.after_step(None)
  avg_rnnt = (rnnt_sum / len(data_loader)).item()
  avg_ctc = (ctc_sum / len(data_loader)).item()
  global last_epoch_stats
  faults = int(_C.lib().lr_rnn_pair_errors())
  last_epoch_stats = {"batches": len(data_loader), "skipped": opts[0].skipped_steps() - skipped_before,
                      "recurrence_faults": faults}
  if last_epoch_stats["skipped"] or faults:
    print("\tSkipped batches: %(skipped)d of %(batches)d (recurrence time-outs: %(recurrence_faults)d)"
          % last_epoch_stats)
  print(f'\tTraining transducer_loss: {avg_rnnt}')
  print(f'\tTraining ctc_loss: {avg_ctc}')
  return avg_rnnt, avg_ctc


def transducer_cer(encoder, head, data_loader, device, char2idx, max_symbols=5, beam_width=0):
  """The host CER loop (_host_cer, time-out re-decode included) over the head's greedy transcripts, or over the top
  hypotheses of its beam search at a positive beam_width."""
  head.eval()

  def hypotheses(frames, frame_lens):
    lens_d = frame_lens.to(device)
    out = encoder(frames.to(device), lens_d, max_len=host_max_len(frame_lens), need_final_state=False)
    hidden = out[1] if getattr(encoder, "enable_ctc", False) else out[0]
    return head.decode_strings(hidden, lens_d, max_symbols=max_symbols, beam_width=beam_width)

  return _host_cer(encoder, data_loader, device, char2idx, hypotheses)


# test hook / switch: False keeps the CTC branch of a decoder step on the step's own stream
overlap_ctc_branch = True
_ctc_side = None


def _ctc_stream(device):
  global _ctc_side
  if _ctc_side is None or _ctc_side.device != device:
    _ctc_side = torch.cuda.Stream(device=device)
  return _ctc_side


def _step_all(opts, grad_norm, status):
  """The per-module clip + Adam of train_better_model.py:77-80 for opts = (encoder's, decoder's).  When the decoder
  loop's weight half ran on the side stream (attention_decoder.overlap_weight_half), its gradients were complete long
  before the encoder's: the decoder's optimiser goes to that stream as well — sum of squares + Adam are HBM-bound and run
  beside the encoder's weight-gradient products — and the streams are joined behind the encoder's optimiser."""
  from . import attention_decoder as _dec
  from . import encoder as _enc
  side_ok = len(opts) == 2 and _dec.take_split_flag() and _dec.side_stream() is not None
  if not side_ok:
    for o in opts:
      o.step(grad_norm=grad_norm, grad_scale=1.0, skip=status)
    return
  main = torch.cuda.current_stream()
  side = _dec.side_stream()
  with torch.cuda.stream(side):     # (the side stream already holds everything the decoder's gradients depend on)
    opts[1].step(grad_norm=grad_norm, grad_scale=1.0, skip=status)
  opts[0].step(grad_norm=grad_norm, grad_scale=1.0, skip=status)
  main.wait_stream(side)


def decoder_step(encoder, decoding_step, opts, frames, frame_lens, chars, char_lens, flags, seed, pad,
                 grad_norm=None, max_len=None, grad_sync=(None, None), graphs=None):
  """The reference's WHOLE step (train_better_model.py:46-80) for one batch, all on the device:
  encoder (:46) -> CTC 'mean' when the encoder has it (:48) -> decoder loop over len(flags) steps with
  the given teacher-forcing pattern (:54-63) -> NLL / non-PAD count (:65) -> one backward of the sum
  (:69,:74) -> per-module clip + Adam (:77-80).  opts = (encoder FusedAdam, decoder FusedAdam);
  grad_sync = (encoder GradSync | None, decoder GradSync | None).
  Returns (decoder_loss, ctc_loss | None, status | None) device tensors."""
  syncs = tuple(grad_sync)
  use_ctc = encoder.enable_ctc
  L = len(flags)
  whole = syncs[0] is None and syncs[1] is None

  def body(frames, frame_lens_d, chars, char_lens_d):
    labels = chars[:, 1:]
    status, total, ctc = None, 0, None
    # labels + 1, label_lens = char_lens - 1 and the int32 lengths in one launch (as ctc_step does) instead of four
    # ATen conversions — the launch that clears the encoder's gradients
    fused_prep = (use_ctc and chars.dtype == torch.int64 and frame_lens_d.dtype == torch.int64
                  and char_lens_d.dtype == torch.int64 and chars.dim() == 2 and chars.stride(1) == 1)
    if fused_prep:
      labels_p1, frame_lens32, label_lens32 = opts[0].zero_grad_and_prepare_ctc(chars, frame_lens_d, char_lens_d)
    for o in (opts[1:] if fused_prep else opts):
      o.zero_grad()
    ctc_side = None
    if use_ctc:
      # The CTC branch (head, loss — and, because autograd runs a node's backward on the stream of its forward, their
      # backward) on a stream of its own beside the decoder loop: both only read the encoder's states.
      if whole and overlap_ctc_branch and isinstance(encoder, _VideoEncoder):
        ctc_side = _ctc_stream(frames.device)
      log_probs, hidden, state = (encoder(frames, frame_lens32 if fused_prep else frame_lens_d, max_len=max_len,
                                          head_stream=ctc_side) if ctc_side is not None else
                                  encoder(frames, frame_lens32 if fused_prep else frame_lens_d, max_len=max_len))
      with (torch.cuda.stream(ctc_side) if ctc_side is not None else contextlib.nullcontext()):
        if fused_prep:
          ctc, status, _ = ctc_loss_prepared(log_probs, labels_p1, frame_lens32, label_lens32, 'mean')
        else:
          ctc, status, _ = ctc_loss_with_status(log_probs, labels, frame_lens_d, char_lens_d - 1, 'mean')
      total = ctc
    else:
      hidden, state = encoder(frames, frame_lens_d, max_len=max_len)
    log_probs_d, _, _ = decoding_step.decode_sequence(chars[:, :L], state, frame_lens32 if fused_prep else frame_lens_d, hidden,
                                                      teacher_forced=flags, seed=seed)
    decoder_loss = decoder_nll(log_probs_d, labels, pad)
    # one traversal from BOTH roots (the reference's two backward calls, train_better_model.py:70,74, add up to this);
    # no `decoder_loss + ctc` tensor: that sum was an elementwise launch of its own
    for sy in syncs:
      if sy is not None and hasattr(sy, "set_status"):
        sy.set_status(status)
    one = _one(decoder_loss.device)
    if ctc_side is not None:
      torch.cuda.current_stream().wait_stream(ctc_side)     # the loss and the status exist
    if use_ctc:
      torch.autograd.backward([decoder_loss, total], [one, one])
    else:
      decoder_loss.backward(one)
    if ctc_side is not None:
      # (the head's parameter gradients are written in place by its backward, on that stream: no AccumulateGrad node
      # that would make the engine join it)
      torch.cuda.current_stream().wait_stream(ctc_side)
    if whole:
      _step_all(opts, grad_norm, status)
    out = (decoder_loss.detach(),)
    return out + ((ctc.detach(), status) if use_ctc else ())

  dev = frames.device
  inputs = (frames, frame_lens.to(dev), chars.to(dev), char_lens.to(dev))
  if graphs is None:
    out = body(*inputs)
  else:
    ml = frames.shape[1] if max_len is None else int(max_len)
    key = ("dec", id(encoder), id(decoding_step), tuple((id(o), o.lr) for o in opts), tuple(frames.shape),
           str(frames.dtype), tuple(chars.shape), ml, L, grad_norm, whole, use_ctc)
    # only the all-teacher-forced loop has a launch sequence that does not depend on the coins; its
    # sampled tokens are not used by train(), so replaying the captured seed changes nothing
    with _Held(syncs):
      out = graphs.run(key, inputs, body, capturable=(all(flags) and ml == frames.shape[1]))
  decoder_loss = out[0]
  ctc, status = (out[1], out[2]) if use_ctc else (None, None)
  if not whole:
    # per-module clip (:77-79) on the all-reduced gradients; a batch the reference skips (:49-50)
    # updates nothing (with several ranks: only if every rank skipped, GradSync's MIN over ranks)
    for o, sync in zip(opts, syncs):
      scale = sync(status) if sync is not None else 1.0
      o.step(grad_norm=grad_norm, grad_scale=scale, skip=status, dist_words=getattr(sync, "dist_words", None),
             world=getattr(sync, "world", 1))
  return decoder_loss, ctc, status


def _decoder_losses(decoding_step, chars, labels, label_lens_host, frame_lens, hidden, state,
                    teacher_forcing_ratio, pad):
  """train_better_model.py:54-65: the decoder loop and its summed NLL.  The teacher-forcing coin
  of every step (:57) is drawn up front from the same host generator (torch.rand(1) per step), so
  all L steps go out as one enqueue; prev_output's multinomial (:63) is drawn on the device."""
  L = int(label_lens_host.max())
  flags = [bool(torch.rand(1) < teacher_forcing_ratio) for _ in range(L)]
  log_probs, sampled, _ = decoding_step.decode_sequence(chars[:, :L], state, frame_lens, hidden,
                                                        teacher_forced=flags)
  nll, _ = decoder_nll_sum(log_probs, labels, pad)
  return nll, sampled, L


def train(encoder, decoding_step, data_loader, opt, device, char2idx,
          teacher_forcing_ratio=1, grad_norm=None, grad_sync=None, graphs=None):
  """Assumes sequences begin with BOS and end with EOS; data_loader yields
  (frames f32, frame_lens i64, chars i64, char_lens i64) — train_better_model.py:7-86.

  decoding_step=None: encoder+CTC alone, `opt` a FusedAdam over the encoder (`grad_sync`: one
  distributed.GradSync or None).  With a CharDecodingStep `opt` is (encoder FusedAdam, decoder
  FusedAdam) and `grad_sync`, if given, (encoder GradSync, decoder GradSync): the reference clips the two
  modules separately (:77-79) and one Adam over both is the same update as two Adams.  The
  reference runs decoder_loss.backward(retain_graph) and then ctc_loss.backward() (:70,:74): two
  traversals of the encoder graph whose gradients add; here the two losses are summed and the
  encoder is traversed once — the same gradients up to fp32 addition order.

  `graphs` (optional, a StepGraphs): replay each batch shape's step as one hipGraph."""
  use_ctc = encoder.enable_ctc
  pad = char2idx[PAD]
  device = torch.device(device)
  if decoding_step is None:
    assert use_ctc, "without a decoding step the encoder must have enable_ctc=True"
    assert isinstance(opt, FusedAdam), "opt must be lipreading_amd.optim.FusedAdam"
    opts = (opt,)
  else:
    # data parallel: grad_sync = (encoder GradSync, decoder GradSync), one per flat buffer
    syncs = (None, None) if grad_sync is None else tuple(grad_sync)
    assert len(syncs) == 2, "with a decoding step grad_sync is (encoder GradSync, decoder GradSync)"
    opts = tuple(opt)
    assert len(opts) == 2 and all(isinstance(o, FusedAdam) for o in opts), \
        "opt must be (encoder FusedAdam, decoder FusedAdam)"
    decoding_step.train()
  encoder.train()
  ctc_sum = torch.zeros((), dtype=torch.float32, device=device)
  dec_sum = torch.zeros((), dtype=torch.float32, device=device)
  skipped_before = opts[0].skipped_steps() if device.type == "cuda" else 0
  watch = RecurrenceWatch(device) if device.type == "cuda" else None
  flag2 = torch.zeros(2, dtype=torch.int32, device=device) if device.type == "cuda" else None
  for frames, frame_lens, chars, char_lens in data_loader:
    _check_framing(chars, char_lens, frame_lens, char2idx, use_ctc)
    max_len = host_max_len(frame_lens)
    label_lens_host = (char_lens - 1).cpu()
    frames, chars = frames.to(device, non_blocking=True), chars.to(device, non_blocking=True)
    frame_lens_d, char_lens_d = frame_lens.to(device, non_blocking=True), char_lens.to(device, non_blocking=True)
    if decoding_step is None:
      loss, _ = ctc_step(encoder, opt, frames, frame_lens_d, chars, char_lens_d, grad_norm=grad_norm,
                         max_len=max_len, grad_sync=grad_sync, graphs=graphs)
      ctc_sum += loss  # a skipped batch contributes 0, as `continue` does at :49-50
      if watch is not None:
        watch.after_step(graphs)
      continue
    # the teacher-forcing coins (:57) and the sampler seed (:63) come from the host generator; drawn here,
    # outside anything that may be captured
    L = int(label_lens_host.max())
    flags = tuple(bool(torch.rand(1) < teacher_forcing_ratio) for _ in range(L))
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    decoder_loss, ctc, status = decoder_step(encoder, decoding_step, opts, frames, frame_lens_d, chars, char_lens_d,
                                             flags, seed, pad, grad_norm=grad_norm, max_len=max_len, grad_sync=syncs,
                                             graphs=graphs)
    # a recurrence time-out anywhere in the step (the decoder loop's included, which runs AFTER the CTC status was
    # written) leaves garbage in decoder_loss: the fault word masks it, with or without a CTC status
    keep = _fault_keep(flag2) if flag2 is not None else 1
    if status is None:
      dec_sum += torch.where(keep, decoder_loss, torch.zeros_like(decoder_loss)) if flag2 is not None else decoder_loss
    else:
      ok = (status.reshape(()) == 0) & keep if flag2 is not None else (status.reshape(()) == 0)
      dec_sum += torch.where(ok, decoder_loss, torch.zeros_like(decoder_loss))
      ctc_sum += ctc
    if watch is not None:
      watch.after_step(graphs)
  avg_ctc_loss = (ctc_sum / len(data_loader)).item()  # :84 divides by len(data_loader)
  avg_decoder_loss = (dec_sum / len(data_loader)).item()
  # batches that updated nothing this epoch — the reference's `continue` (:49-50) and, here, steps whose one-launch
  # recurrence timed out (the device-side fault word made CTC / Adam skip them) — read once per epoch
  global last_epoch_stats
  if device.type == "cuda":
    faults = int(_C.lib().lr_rnn_pair_errors())
    last_epoch_stats = {"batches": len(data_loader), "skipped": opts[0].skipped_steps() - skipped_before,
                        "recurrence_faults": faults}
    if last_epoch_stats["skipped"] or faults:
      print("\tSkipped batches: %(skipped)d of %(batches)d (recurrence time-outs: %(recurrence_faults)d)"
            % last_epoch_stats)
  if decoding_step is not None:
    print(f'\tTraining decoder_loss: {avg_decoder_loss}')
  if use_ctc:
    print(f'\tTraining ctc_loss: {avg_ctc_loss}')
  return avg_decoder_loss, avg_ctc_loss


def eval(encoder, decoding_step, data_loader, device, char2idx):
  """train_better_model.py:89-143: CTC 'sum' per batch (:116) averaged over len(data_loader)
  (:141); decoder loop teacher-forced on every step (:125), NLL summed and divided by the count of
  non-PAD labels (:138), `correct` counts multinomial samples equal to the label (:129-133).
  Returns (decoder_loss, correct, count, ctc_loss) — the reference's tuple plus the CTC average
  it computes and drops."""
  pad = char2idx[PAD]
  use_ctc = encoder.enable_ctc
  encoder.eval()
  if decoding_step is not None:
    decoding_step.eval()
  ctc_sum = torch.zeros((), dtype=torch.float32, device=device)
  dec_sum = torch.zeros((), dtype=torch.float32, device=device)
  correct = torch.zeros((), dtype=torch.int64, device=device)
  count = torch.zeros((), dtype=torch.float32, device=device)
  on_gpu = torch.device(device).type == "cuda"
  flag2 = torch.zeros(2, dtype=torch.int32, device=device) if on_gpu else None
  faulted = torch.zeros((), dtype=torch.int32, device=device)
  with torch.no_grad():
    for frames, frame_lens, chars, char_lens in data_loader:
      _check_framing(chars, char_lens, frame_lens, char2idx, use_ctc, in_eval=True)
      if on_gpu:
        _roll_faults(device)   # a time-out in an earlier batch must not mark this one
      max_len = host_max_len(frame_lens)
      label_lens_host = (char_lens - 1).cpu()
      frames, chars = frames.to(device), chars.to(device)
      frame_lens_d = frame_lens.to(device)
      labels = chars[:, 1:]
      keep = 1
      if use_ctc:
        log_probs, hidden, state = encoder(frames, frame_lens_d, max_len=max_len)
        loss, status, _ = ctc_loss_with_status(log_probs, labels, frame_lens_d,
                                               (char_lens - 1).to(device), 'sum')
        ctc_sum += loss
        keep = (status.reshape(()) == 0)  # :117-118 `continue`s past the decoder on a skipped batch
      else:
        hidden, state = encoder(frames, frame_lens_d, max_len=max_len)
      if decoding_step is None:
        if on_gpu:
          faulted += (~_fault_keep(flag2)).int()
        continue
      nll, sampled, L = _decoder_losses(decoding_step, chars, labels, label_lens_host, frame_lens_d,
                                        hidden, state, 2.0, pad)
      mask = labels[:, :L] != pad
      if on_gpu:
        # (a one-launch recurrence that timed out — the encoder's or the decoder loop's — left garbage: the batch counts
        # like one the reference `continue`s past, and is reported below)
        fk = _fault_keep(flag2)
        faulted += (~fk).int()
        keep = keep * fk
      dec_sum += torch.where(keep.bool(), nll, torch.zeros_like(nll)) if torch.is_tensor(keep) else nll
      correct += ((sampled.long() == labels[:, :L]) & mask).sum() * keep
      count += mask.sum().float() * keep
  if on_gpu:
    _roll_faults(device)
    nf = int(faulted.item())
    if nf:
      print("\tEvaluation batches dropped after a recurrence time-out: %d of %d" % (nf, len(data_loader)))
  ctc_avg = (ctc_sum / len(data_loader)).item()
  if decoding_step is None:
    return 0.0, 0, 0, ctc_avg
  count_h = count.item()
  return (dec_sum / count).item() if count_h else float('nan'), int(correct.item()), count_h, ctc_avg


@contextlib.contextmanager
def _step_kernels(encoder):
  """Inside the block the encoder's recurrences run on the per-step kernels (recurrence='f32'), which cannot time out;
  the saved mode comes back on the way out, also when the block raises.  Yields whether there was anything to switch:
  an encoder without a `recurrence` attribute (TransformerVideoEncoder) is left untouched."""
  inner = getattr(encoder, "encoder", encoder)   # (PixelLipReader wraps the VideoEncoder)
  if not hasattr(inner, "recurrence"):
    yield False
    return
  saved = inner.recurrence
  inner.recurrence = 'f32'
  try:
    yield True
  finally:
    inner.recurrence = saved


def _retried(encoder, flag2, run):
  """run()'s result for one batch of an evaluation loop — the encoder and whatever consumes its output, ending in a
  host read —, from the per-step kernels if a one-launch recurrence timed out under it.  `flag2` is the loop's
  two-word export buffer on the device, None on a CPU device (nothing to roll or read there).

  The fault words are rolled per batch, as eval() does: only THIS batch's time-out counts.  (Round 4 read
  lr_rnn_pair_errors() here — pending + total, cleared by the read —, so one timed-out TRAINING step of the epoch
  made the first validation batch look faulted and took the epoch's count away from whoever reads it next.)  The
  word is read once, after run() has synchronised, so the read costs no wait of its own; when it is set, run()'s
  output is garbage — and val_cer drives save_best_model and the annealing — so the batch is run again instead of
  being scored, and the word is not read a second time."""
  if flag2 is None:
    return run()
  _roll_faults(flag2.device)
  out = run()
  if not bool(_fault_keep(flag2)):
    with _step_kernels(encoder) as switched:
      if switched:
        out = run()
  return out


def _host_cer(encoder, data_loader, device, char2idx, hypotheses):
  """The host CER loop: sum of space-free edit distances / sum of space-free reference lengths over the loader.
  hypotheses(frames, frame_lens) returns the batch's transcripts as strings without EOS, having read them back from
  the device; it is called through _retried, so a batch whose recurrence timed out is transcribed again."""
  from .decoder import _edit_distance
  inv = {v: k for k, v in char2idx.items()}
  encoder.eval()
  dist, total = 0, 0
  flag2 = torch.zeros(2, dtype=torch.int32, device=device) if torch.device(device).type == "cuda" else None
  with torch.no_grad():
    for frames, frame_lens, chars, char_lens in data_loader:
      hyps = _retried(encoder, flag2, lambda: hypotheses(frames, frame_lens))
      for b, hyp in enumerate(hyps):
        ref = ''.join(inv[int(c)] for c in chars[b, 1:int(char_lens[b]) - 1]).replace(' ', '')  # strip BOS/EOS
        dist += _edit_distance(hyp.replace(' ', ''), ref)
        total += len(ref)
  return dist / max(total, 1)


def greedy_cer(encoder, data_loader, device, char2idx):
  """Character error rate of the CTC greedy path (decoder.py:64-73 on decoder.py:182-197
  output): sum of edit distances / sum of reference lengths.  The reference composes these
  only in its dead archived script (archive/train_model.py:351-357)."""
  from .decoder import GreedyDecoder, ctc_labels
  return ctc_cer(encoder, data_loader, device, char2idx, GreedyDecoder(ctc_labels(char2idx), blank_index=0))


def ctc_cer(encoder, data_loader, device, char2idx, decoder):
  """The host CER loop (_host_cer, time-out re-decode included) with any CTC decoder whose decode() returns the
  reference's (strings, offsets) — e.g. decoder.BeamCTCDecoder(ctc_labels(char2idx), log_probs_input=True, ...); the
  best hypothesis strings[b][0] is scored.  The encoder's output is log-probabilities: a BeamCTCDecoder here needs
  log_probs_input=True."""
  def hypotheses(frames, frame_lens):
    lens_d = frame_lens.to(device)
    log_probs = encoder(frames.to(device), lens_d, max_len=host_max_len(frame_lens))[0]
    return [s[0].replace(EOS, '') for s in decoder.decode(log_probs, lens_d)[0]]

  return _host_cer(encoder, data_loader, device, char2idx, hypotheses)


def attention_cer(encoder, decoding_step, data_loader, device, char2idx, beam_width=10, max_label_len=100,
                  ctc_weight=0.0, pre_beam=None, lm=None):
  """CER of the attention decoder's own transcripts: the best hypothesis of CharDecodingStep.beam_search (the
  reference's analysis.inference, with this build's deterministic rule) with EOS stripped, scored as greedy_cer
  scores the CTC head (sum of space-free edit distances / sum of space-free reference lengths).  A batch whose
  encoder recurrence timed out is encoded and searched again with recurrence='f32' (_retried).  ctc_weight > 0 runs
  the joint CTC/attention search on the CTC head of the same encoder pass (re-encoded with it); `lm`
  (a lm.WordLM over decoder.ctc_labels(char2idx)) adds the word language model to the search."""
  from .analysis import best_ids, encode_for_beam, need_ctc_head
  if ctc_weight > 0:
    need_ctc_head(encoder)
  inv = {v: k for k, v in char2idx.items()}
  eos = char2idx[EOS]
  decoding_step.eval()

  def hypotheses(frames, frame_lens):
    hidden, lens_d, state, y = encode_for_beam(encoder, frames, frame_lens, device, with_ctc=ctc_weight > 0)
    best = best_ids(decoding_step, hidden, lens_d, state, beam_width, max_label_len, ctc_log_probs=y,
                    ctc_weight=ctc_weight, pre_beam=pre_beam, lm=lm)
    return [''.join(inv[int(i)] for i in h if i != eos) for h in best]

  return _host_cer(encoder, data_loader, device, char2idx, hypotheses)


def _two_pass(encoder, decoding_step, ctc_decoder, frames, frame_lens, device, nbest, ctc_weight, length_bonus,
              frame_lens_d=None):
  """One batch of two-pass decoding, all enqueued: one encoder pass for log-probs, hidden states and
  final state, the CTC search's N-best (ctc_decoder.decode_ids), then CharDecodingStep.rescore through
  analysis.rescored_best -> (ids (B, W) int32 decoder tokens, lens (B,) int32) of the hypothesis ranked first.  Only
  decode_ids of the CTC decoder and __call__ of the encoder are used: decoder.ChunkedBeamDecoder and
  encoder_stream.ChunkedEncoder stand in for them unchanged.  A clip of more than 1024 frames is rescored on the first
  1024 classes of each hypothesis, the most rescore takes (a transcript has far fewer characters than frames)."""
  from .analysis import rescored_best
  lens_d = frame_lens.to(device) if frame_lens_d is None else frame_lens_d
  log_probs, hidden, state = encoder(frames.to(device), lens_d, max_len=host_max_len(frame_lens))
  ids, _, lens, scores = ctc_decoder.decode_ids(log_probs, lens_d)
  n = min(int(nbest), ids.shape[1])
  return rescored_best(decoding_step, hidden, lens_d, state, ids[:, :n, :1024], lens[:, :n], scores[:, :n],
                       ctc_weight=ctc_weight, length_bonus=length_bonus)


def _check_two_pass(encoder, ctc_decoder, nbest, char2idx):
  from .analysis import need_ctc_head
  from .decoder import ctc_labels
  need_ctc_head(encoder)
  if not hasattr(ctc_decoder, "decode_ids") or not hasattr(ctc_decoder, "beam_width"):
    raise TypeError("attention rescoring needs a CTC beam decoder with decode_ids() (BeamCTCDecoder)")
  if list(ctc_decoder.labels) != ctc_labels(char2idx):
    raise ValueError("the CTC decoder's labels are not ctc_labels(char2idx)")
  if isinstance(nbest, bool) or not isinstance(nbest, int) or not 1 <= nbest <= min(ctc_decoder.beam_width, 128):
    raise ValueError("nbest must be an int in [1, min(beam_width, 128)] = [1, %d], got %r"
                     % (min(ctc_decoder.beam_width, 128), nbest))


def rescored_cer(encoder, decoding_step, data_loader, device, char2idx, ctc_decoder, nbest=10, ctc_weight=0.5,
                 length_bonus=0.0):
  """CER of two-pass decoding: the CTC beam search's `nbest` best hypotheses rescored by the attention
  decoder (CharDecodingStep.rescore: (1 - ctc_weight) * attention - ctc_weight * first-pass score + length_bonus *
  tokens), the hypothesis ranked first cut at its first EOS and scored as attention_cer scores (the host CER loop, a
  batch whose recurrence timed out run again on the per-step kernels).  `ctc_decoder` is a BeamCTCDecoder over
  ctc_labels(char2idx) with log_probs_input=True, or decoder.ChunkedBeamDecoder around one; the encoder needs
  enable_ctc."""
  _check_two_pass(encoder, ctc_decoder, nbest, char2idx)
  inv = {v: k for k, v in char2idx.items()}
  decoding_step.eval()

  def hypotheses(frames, frame_lens):
    ids, lens = _two_pass(encoder, decoding_step, ctc_decoder, frames, frame_lens, device, nbest, ctc_weight,
                          length_bonus)
    ids, lens = ids.cpu(), lens.cpu()
    return [''.join(inv[int(i)] for i in ids[b, :int(lens[b])]) for b in range(ids.shape[0])]

  return _host_cer(encoder, data_loader, device, char2idx, hypotheses)


# ---- scoring on the device (lipreading_amd/scoring.py) -------------------------------------------------
# The three loops above copy the ids to the host every batch, join label strings and run decoder._edit_distance (a
# pure-Python O(n m) loop) per utterance, with the GPU idle.  device_scores keeps the ids on the device: per batch
# it enqueues encoder -> decode_ids / beam_search -> lr_edit_distance and reads nothing back.

last_device_score_stats = None   # {"batches", "gated", "rescored"} of the latest device_scores call
_SCORERS = {}                    # label tuple -> EditScorer (its tables are uploaded once per device)


def _fault_gate(flag2):
  """Exports the fault words into `flag2` on the stream and returns the int32 view whose first element is non-zero
  iff a one-launch recurrence has timed out since the last roll — lr_edit_distance's `gate`; no host read."""
  _C.check(_C.lib().lr_fault_export(None, flag2.data_ptr(), _C.stream_handle()), "lr_fault_export")
  return flag2[1:]


class _DeviceScoring(object):
  """What a device_scores call carries from batch to batch."""

  def __init__(self, encoder, device, char2idx, decoder, decoding_step, beam_width, max_label_len, ctc_weight, pre_beam,
               units, align, n_batches, lm=None, rescore_nbest=0, length_bonus=0.0):
    from .decoder import GreedyDecoder, ctc_labels
    from .scoring import EditScorer
    self.encoder, self.device, self.decoding_step = encoder, torch.device(device), decoding_step
    self.beam = (beam_width, max_label_len)
    self.rescore_nbest, self.length_bonus = int(rescore_nbest), length_bonus
    self.joint = decoding_step is not None and ctc_weight > 0 and not self.rescore_nbest
    self.ctc_weight, self.pre_beam, self.lm = ctc_weight, pre_beam, lm
    self.units, self.align = tuple(units), bool(align)
    inv = {v: k for k, v in char2idx.items()}
    if decoding_step is None:
      # CTC classes: character id + 1, blank at 0; the references are shifted the same way (as lr_ctc_prepare_i64 does)
      labels, self.shift = ctc_labels(char2idx), 1
      self.decoder = decoder if decoder is not None else GreedyDecoder(labels, blank_index=0)
      if not hasattr(self.decoder, "decode_ids"):
        raise TypeError("device scoring needs a decoder with decode_ids() (GreedyDecoder, BeamCTCDecoder)")
      if list(self.decoder.labels) != labels:
        raise ValueError("the decoder's labels are not ctc_labels(char2idx)")
    else:
      # (two-pass decoding keeps the CTC decoder for its first pass; its answer is in decoder tokens all the same)
      labels, self.shift, self.decoder = [inv[i] for i in range(len(inv))], 0, decoder if self.rescore_nbest else None
    key = tuple(labels)
    self.scorer = _SCORERS.get(key)
    if self.scorer is None:
      self.scorer = _SCORERS[key] = EditScorer(labels)
    self.scorer._state(self.device)   # the tables' upload (once per device) happens here, not in the first batch
    self.flag2 = torch.zeros(2, dtype=torch.int32, device=self.device)
    self.gated = torch.zeros(max(n_batches, 1), dtype=torch.int32, device=self.device)

  def hypotheses(self, frames, frame_lens, frame_lens_d):
    """One encoder pass and one search, all enqueued: (ids (B, W) int32 view, lens (B,) int32 view)."""
    if self.decoding_step is None:
      log_probs, _, _ = self.encoder(frames, frame_lens_d, max_len=host_max_len(frame_lens))
      got = self.decoder.decode_ids(log_probs, frame_lens_d)
      if len(got) == 3:
        return got[0], got[2]
      return got[0][:, 0], got[2][:, 0]       # the best hypothesis of (B, W, T) / (B, W)
    if self.rescore_nbest:
      return _two_pass(self.encoder, self.decoding_step, self.decoder, frames, frame_lens, self.device,
                       self.rescore_nbest, self.ctc_weight, self.length_bonus, frame_lens_d=frame_lens_d)
    from .analysis import best_beam, encode_for_beam
    hidden, lens_d, state, y = encode_for_beam(self.encoder, frames, frame_lens, self.device, with_ctc=self.joint)
    return best_beam(self.decoding_step, hidden, lens_d, state, *self.beam, ctc_log_probs=y, ctc_weight=self.ctc_weight,
                     pre_beam=self.pre_beam, lm=self.lm)


def _device_batch(ctx, k, frames, frame_lens, frame_lens_d, chars_d, char_lens_d, gated=True):
  """Batch k, after its upload: everything here is an enqueue.  With gated=False (the re-score pass) the fault word
  is not consulted."""
  _roll_faults(ctx.device)
  hyp, hyp_lens = ctx.hypotheses(frames, frame_lens, frame_lens_d)
  # BOS and EOS stripped as the host loops do: chars[b, 1:char_lens[b] - 1]
  ref = (chars_d + ctx.shift if ctx.shift else chars_d).to(torch.int32)[:, 1:]
  ref_lens = (char_lens_d - 2).clamp_(min=0).to(torch.int32)
  gate = None
  if gated:
    gate = _fault_gate(ctx.flag2)
    ctx.gated[k:k + 1].copy_(gate[:1])
  for unit in ctx.units:
    ctx.scorer.score(hyp, hyp_lens, ref, ref_lens, unit=unit, align=ctx.align and unit == 'char', gate=gate)


def _device_score_run(encoder, data_loader, device, char2idx, decoder=None, decoding_step=None, beam_width=10,
                      max_label_len=100, ctc_weight=0.0, pre_beam=None, units=('char', 'word'), align=False, lm=None,
                      rescore_nbest=0, length_bonus=0.0):
  global last_device_score_stats
  device = torch.device(device)
  if device.type != "cuda":
    raise _C.LipReadingHipError("device scoring runs on the MI355X only (no CPU fallback)")
  if rescore_nbest:
    if decoding_step is None:
      raise ValueError("rescore_nbest needs a decoding_step (the second pass) next to the CTC decoder")
    _check_two_pass(encoder, decoder, rescore_nbest, char2idx)
  elif decoding_step is not None and ctc_weight > 0:
    from .analysis import need_ctc_head
    need_ctc_head(encoder)
  ctx = _DeviceScoring(encoder, device, char2idx, decoder, decoding_step, beam_width, max_label_len, ctc_weight, pre_beam,
                       units, align, len(data_loader), lm=lm, rescore_nbest=rescore_nbest, length_bonus=length_bonus)
  ctx.scorer.reset()
  encoder.eval()
  if decoding_step is not None:
    decoding_step.eval()

  def upload(batch):
    frames, frame_lens, chars, char_lens = batch
    return (frames.to(device), frame_lens, frame_lens.to(device), chars.to(device), char_lens.to(device))

  with torch.no_grad():
    for k, batch in enumerate(data_loader):
      _device_batch(ctx, k, *upload(batch))
    # the one read: the totals and which batches the fault word kept out of them
    res, gated = ctx.scorer.read(extra=ctx.gated)
    again = set(i for i, g in enumerate(gated.tolist()) if g != 0)
    rescored = 0
    if again:
      # a one-launch recurrence timed out in those batches (see _retried): they were left out of the totals; encode
      # just them again on the per-step kernels and score them — the host loops' immediate re-decode, deferred
      with _step_kernels(encoder):
        for k, batch in enumerate(data_loader):
          if k in again:
            _device_batch(ctx, k, *upload(batch), gated=False)
            rescored += 1
      res = ctx.scorer.result()
  last_device_score_stats = {"batches": len(data_loader), "gated": len(again), "rescored": rescored}
  return res, ctx.scorer


def device_scores(encoder, data_loader, device, char2idx, decoder=None, decoding_step=None, beam_width=10,
                  max_label_len=100, ctc_weight=0.0, pre_beam=None, units=('char', 'word'), align=False, lm=None,
                  rescore_nbest=0, length_bonus=0.0):
  """greedy_cer / ctc_cer / attention_cer / rescored_cer's evaluation with the scoring on the device: the dict of
  scoring.EditScorer.result() — cer, wer, distance, ref_len, pairs, ... (hits / sub / ins / dele with align=True).

  decoder=None, decoding_step=None: the CTC head's greedy path (greedy_cer).  decoder = a BeamCTCDecoder over
  ctc_labels(char2idx): its best hypothesis (ctc_cer).  decoding_step: the attention decoder's beam search
  (attention_cer; beam_width, max_label_len, and ctc_weight > 0 with pre_beam for the joint search; `lm`, a
  lm.WordLM, adds the word language model to that search).  rescore_nbest > 0 with BOTH `decoder` (a BeamCTCDecoder)
  and `decoding_step`: two-pass decoding (rescored_cer) — the decoder's rescore_nbest best hypotheses
  rescored by the attention decoder at `ctc_weight` and `length_bonus`.

  Per batch nothing is read back.  A recurrence time-out is handled as in the host loops, but without their per-batch
  read: the device-side fault word gates the batch out of the totals (lr_edit_distance's `gate`), a device vector
  records which batches were gated, and after the last batch one read covers the totals and that vector; only if some
  batch was gated is the loader walked again and just those batches re-encoded with recurrence='f32' and scored."""
  return _device_score_run(encoder, data_loader, device, char2idx, decoder, decoding_step, beam_width, max_label_len,
                           ctc_weight, pre_beam, units, align, lm, rescore_nbest, length_bonus)[0]


def device_cer(encoder, data_loader, device, char2idx, decoder=None, decoding_step=None, beam_width=10,
               max_label_len=100, ctc_weight=0.0, pre_beam=None, lm=None, rescore_nbest=0, length_bonus=0.0):
  """The same float as greedy_cer (no decoder), ctc_cer (`decoder`), attention_cer (`decoding_step`) or rescored_cer
  (both, with rescore_nbest): sum of
  space-free edit distances / sum of space-free reference lengths, scored on the device (device_scores)."""
  return device_scores(encoder, data_loader, device, char2idx, decoder, decoding_step, beam_width, max_label_len,
                       ctc_weight, pre_beam, units=('char',), lm=lm, rescore_nbest=rescore_nbest,
                       length_bonus=length_bonus)["cer"]


# ---- forced alignment over a loader (lipreading_amd/align.py) -----------------------------------------

def align_loader(encoder, data_loader, device, char2idx, fps=29.97):
  """When is each character and word of every caption spoken, by the encoder's CTC head: a generator of one record per
  utterance, in the loader's order — align.CTCAligner.records' dict (status, total, chars, words; frames as ints)
  plus `index` (the running utterance number) and `frames` (the clip's length).

  Per batch: the encoder, then one lr_ctc_align launch against the TRAINING targets — ctc.prepare_ctc_inputs' labels,
  i.e. chars[:, 1:] with '<EOS>', which the head was trained to emit ('<EOS>' gets a span but belongs to no word) —
  and one read.  The fault words are rolled and read by _retried: a batch whose one-launch recurrence timed out is
  encoded again with recurrence='f32' before it is aligned."""
  from .align import CTCAligner
  from .analysis import need_ctc_head
  from .decoder import ctc_labels
  device = torch.device(device)
  if device.type != "cuda":
    raise _C.LipReadingHipError("forced alignment runs on the MI355X only (no CPU fallback)")
  need_ctc_head(encoder)
  aligner = CTCAligner(ctc_labels(char2idx), blank_index=0, fps=fps)
  encoder.eval()
  flag2 = torch.zeros(2, dtype=torch.int32, device=device)
  index = 0
  with torch.no_grad():
    for frames, frame_lens, chars, char_lens in data_loader:
      max_len = host_max_len(frame_lens)
      frames_d, lens_d = frames.to(device), frame_lens.to(device)
      labels_p1, lens32, label_lens32 = prepare_ctc_inputs(chars.to(device), lens_d, char_lens.to(device))

      def aligned():
        log_probs = encoder(frames_d, lens_d, max_len=max_len)[0]
        return aligner.records(aligner.align_ids(log_probs, lens32, labels_p1, label_lens32), labels_p1, label_lens32)

      n = frame_lens.tolist()
      for b, rec in enumerate(_retried(encoder, flag2, aligned)):
        rec["index"], rec["frames"] = index, int(n[b])
        index += 1
        yield rec


# ---- keyword spotting over a loader (lipreading_amd/spot.py) ------------------------------------------

def spot_batches(encoder, data_loader, device, char2idx, keywords, **spotter_kw):
  """spot_loader's walk, batch by batch: a generator of (the loader's batch, KeywordSpotter.spot's answer for it), so
  that a caller who also wants the captions (analysis.keyword_report) takes them from the same walk."""
  from .analysis import need_ctc_head
  from .decoder import ctc_labels
  from .spot import KeywordSpotter
  device = torch.device(device)
  if device.type != "cuda":
    raise _C.LipReadingHipError("keyword spotting runs on the MI355X only (no CPU fallback)")
  need_ctc_head(encoder)
  spotter = KeywordSpotter(ctc_labels(char2idx), keywords, blank_index=0, **spotter_kw)
  encoder.eval()
  flag2 = torch.zeros(2, dtype=torch.int32, device=device)
  with torch.no_grad():
    for batch in data_loader:
      frames, frame_lens = batch[0], batch[1]
      max_len = host_max_len(frame_lens)
      frames_d, lens_d = frames.to(device), frame_lens.to(device)

      def spotted():
        log_probs = encoder(frames_d, lens_d, max_len=max_len)[0]
        return spotter.spot(log_probs, lens_d)

      yield batch, _retried(encoder, flag2, spotted)


def spot_loader(encoder, data_loader, device, char2idx, keywords, **spotter_kw):
  """Where is each of `keywords` spoken in every utterance of `data_loader`, by the encoder's CTC head: a generator of
  one record per utterance, in the loader's order — dict(index (the running utterance number), frames (the clip's
  length), hits (spot.KeywordSpotter.records' list: keyword, index, start, end, score, confidence)).  `spotter_kw` goes
  to KeywordSpotter (fps, max_hits, min_confidence).

  Per batch: the encoder, then one lr_ctc_spot launch and one read, through _retried exactly as align_loader — a batch
  whose one-launch recurrence timed out is encoded again with recurrence='f32' before it is spotted."""
  index = 0
  for batch, spotted in spot_batches(encoder, data_loader, device, char2idx, keywords, **spotter_kw):
    n = batch[1].tolist()
    for b, found in enumerate(spotted):
      yield dict(index=index, frames=int(n[b]), hits=found)
      index += 1


# ---- CTC segmentation of whole videos (lipreading_amd/segment.py) -------------------------------------

def stream_position(offsets, frame):
  """(clip, frame in the clip) of a frame of the stream whose clips start at `offsets` (ascending, offsets[0] == 0)."""
  import bisect
  clip = bisect.bisect_right(offsets, frame) - 1
  return clip, frame - offsets[clip]


def segment_videos(encoder, vid_dirs, device, char2idx, batch_size, fps=29.97, collate_fn=None, pixels=False,
                   threshold=0.8):
  """Where does each caption of a whole video really start and end, by the encoder's CTC head: a generator of one
  record per video directory of `vid_dirs`, in their order.

  Per video: its kept clips in start-time order (dataset.VideoClips) are encoded batch by batch through `collate_fn`
  (default: data.make_collate_fn(device); pass the pixel regime's with pixels=True) — through _retried as align_loader
  does — and every clip's valid log-probability rows are joined into ONE stream on the device.  The stream is segmented
  (segment.CTCSegmenter, both ends free) against the whole caption track, every caption with its '<EOS>' — the training
  target of its clip — one utterance.  Stream frames map back to (clip, frame in the clip) and so to seconds,
  s_e[clip].start + frame / fps.

  The record: dict(video, status, frames, tokens, total, span, captions=[dict(index (the caption's row in the video's
  files), text, old_start_s, old_end_s, start, end (stream frames), start_clip, start_frame, end_clip, end_frame (of the
  caption's last frame), new_start_s, new_end_s, logp, frames, confidence, worst)]).  status: 0, the kernel's
  (segment.INFEASIBLE, ...), segment.TOO_LONG for a video past the kernel's limits and segment.NO_CLIPS for one that
  keeps no clip; with a non-zero status the captions carry their old times only."""
  from . import segment as SG
  from .analysis import need_ctc_head
  from .data import make_collate_fn
  from .dataset import BatchLoader, VideoClips
  from .decoder import ctc_labels
  device = torch.device(device)
  if device.type != "cuda":
    raise _C.LipReadingHipError("CTC segmentation runs on the MI355X only (no CPU fallback)")
  need_ctc_head(encoder)
  segmenter = SG.CTCSegmenter(ctc_labels(char2idx), blank_index=0, fps=fps)
  collate_fn = collate_fn if collate_fn is not None else make_collate_fn(device)
  encoder.eval()
  flag2 = torch.zeros(2, dtype=torch.int32, device=device)
  for vid in vid_dirs:
    clips = VideoClips(vid, char2idx, threshold=threshold, fps=fps, pixels=pixels)
    caps = [dict(index=clips.kept[i], text=clips.captions[i], old_start_s=clips.s_e[i][0], old_end_s=clips.s_e[i][1])
            for i in range(len(clips))]
    rec = dict(video=os.path.basename(os.path.normpath(vid)), status=SG.NO_CLIPS, frames=0, tokens=0, total=None,
               span=None, captions=caps)
    if len(clips) == 0:
      yield rec
      continue
    # the training targets: the caption's characters and '<EOS>' in the CTC head's class layout (chars[:, 1:] + 1)
    ids = [[int(c) + 1 for c in clips[i][1][1:]] for i in range(len(clips))]
    lens = [int(clips.frames[i].shape[0]) for i in range(len(clips))]
    offsets = [0]
    for n in lens[:-1]:
      offsets.append(offsets[-1] + n)
    rec["frames"], rec["tokens"] = sum(lens), sum(len(r) for r in ids)
    if not SG.within_limits(rec["frames"], rec["tokens"]):
      rec["status"] = SG.TOO_LONG
      yield rec
      continue
    rows = []
    with torch.no_grad():
      for frames, frame_lens, _, _ in BatchLoader(clips, batch_size, collate_fn):
        max_len = host_max_len(frame_lens)
        frames_d, lens_d = frames.to(device), frame_lens.to(device)
        n = [int(x) for x in frame_lens.tolist()]

        def valid_rows():
          log_probs = encoder(frames_d, lens_d, max_len=max_len)[0]
          return torch.cat([log_probs[b, :n[b]] for b in range(len(n))], dim=0)

        rows.append(_retried(encoder, flag2, valid_rows))
      stream = torch.cat(rows, dim=0).unsqueeze(0)
      assert stream.shape[1] == rec["frames"]
      tg = torch.tensor([[c for r in ids for c in r]], dtype=torch.int32, device=device)
      first = [0]
      for r in ids[:-1]:
        first.append(first[-1] + len(r))
      d = lambda rows_: torch.tensor([rows_], dtype=torch.int32, device=device)
      out = segmenter.segment_ids(stream, None, tg, d([tg.shape[1]])[0], d(first), d([len(r) for r in ids]),
                                  d([len(ids)])[0])
      got = segmenter.records(out, [clips.captions], tg)[0]
    if got["status"] == 0:
      rec.update(total=got["total"], span=list(got["span"]))
    rec["status"] = got["status"]
    if got["status"] == 0:
      for cap, u in zip(caps, got["utterances"]):
        sc, sf = stream_position(offsets, u["start"])
        ec, ef = stream_position(offsets, u["end"] - 1)
        cap.update(start=u["start"], end=u["end"], start_clip=sc, start_frame=sf, end_clip=ec, end_frame=ef,
                   new_start_s=clips.s_e[sc][0] + sf / fps, new_end_s=clips.s_e[ec][0] + (ef + 1) / fps,
                   logp=u["logp"], frames=u["frames"], confidence=u["confidence"], worst=u["worst"])
    yield rec
