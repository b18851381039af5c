"""GPU: lr_lmk_augment_f32, landmarks.augment_landmarks, PrefetchLoader(lmk_augment=) and the driver's --lmk_augment.
The yardstick is the float64 numpy restatement (tests/lmk_aug_cases.py, records built by hand) or existing code (today's
loaders), never the new code.  Everything is float64 with one rounding, so `y` must lie within ONE fp32 ulp of the
restatement's value (pose_cases.worst_ulps: the ulp taken at max(|want|, 2^-10)) and the clip statistics within 1e-12
relative; what the kernel promises about itself (zeros, determinism, batch = clips, in place = out of place, the
identity record, exact motions) is exact.  The host side is tests/test_lmk_aug_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lmk_aug_cases as AC

pytestmark = pytest.mark.gpu

GUARD = 1024                                       # elements either side of y and the statistics; bytes of the workspace
FULL = "mirror=0.5,rot=10/10/15,scale=0.1,stretch=0.05,shift=0.05,jitter=0.01"


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


def _guarded(dev, n, dtype, fill):
  raw = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
  return raw, raw[GUARD:GUARD + n]


def _intact(raw, n, fill):
  edge = torch.cat([raw[:GUARD], raw[GUARD + n:]])
  return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


def aug_call(dev, x, lens, rec, perm, in_place=False, want_stats=True):
  """One call of the C entry on numpy inputs -> (y [B][t_max][npts][3], stats [B][4]) as numpy.  y is pre-filled with
  NaN (out of place), so an unwritten element shows; y, the statistics and the workspace lie between guards, which every
  call checks.  in_place: x is copied into the guarded buffer and augmented there."""
  from lipreading_amd import _C
  L = _C.lib()
  x = np.array(x, dtype=np.float32, order="C")                  # (a copy: the shared cases are read-only)
  B, t_max, npts, _ = x.shape
  n = x.size
  x_d = torch.from_numpy(x).to(dev)
  lens_d = torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(dev)
  rec_d = torch.from_numpy(np.array(rec, dtype=np.uint64).view(np.int64).reshape(B, 16)).to(dev)
  perm_d = torch.from_numpy(np.asarray(perm, dtype=np.int32)).to(dev)
  assert perm_d.numel() == npts
  need = L.lr_lmk_augment_workspace_bytes(B)
  assert need >= B * 5 * 8
  raw_y, y = _guarded(dev, n, torch.float32, float("nan"))
  raw_s, stats = _guarded(dev, B * 4, torch.float64, float("nan"))
  raw_w, work = _guarded(dev, need, torch.uint8, 0xFF)
  assert work.data_ptr() % 16 == 0
  if in_place:
    y.copy_(x_d.view(-1))
  src = y if in_place else x_d
  _C.check(L.lr_lmk_augment_f32(src.data_ptr(), lens_d.data_ptr(), rec_d.data_ptr(), perm_d.data_ptr(), y.data_ptr(),
                                stats.data_ptr() if want_stats else None, work.data_ptr(), need, B, t_max, npts,
                                _C.stream_handle()), "lr_lmk_augment_f32")
  torch.cuda.synchronize()
  assert _intact(raw_y, n, float("nan")), "wrote outside y"
  assert _intact(raw_s, B * 4, float("nan")), "wrote outside clip_stats"
  assert _intact(raw_w, need, 0xFF), "wrote outside the workspace"
  y_h = y.view(B, t_max, npts, 3).cpu().numpy()
  assert not np.isnan(y_h).any(), "%d elements of y were not written (or are NaN)" % int(np.isnan(y_h).sum())
  stats_h = stats.view(B, 4).cpu().numpy()
  assert np.isnan(stats_h).all() if not want_stats else not np.isnan(stats_h).any()
  if not in_place:
    assert x_d.cpu().numpy().tobytes() == x.tobytes(), "the input was written"
  return y_h, stats_h


def check_against(got, want_y, want_stats, what):
  y, stats = got
  e = AC.worst_ulps(y, want_y)
  rel = float(np.max(np.abs(stats - want_stats) / np.maximum(np.abs(want_stats), 1e-300))) if want_stats.any() else 0.0
  print("%s: y %.3g ulp, clip statistics %.3g relative" % (what, e, rel))
  assert e <= 1.0 and rel <= 1e-12, (what, e, rel)
  return e


# ---- parity ---------------------------------------------------------------------------------------------------------
def test_parity_with_the_restatement(dev):
  worst = 0.0
  for c in AC.parity_cases():
    got = aug_call(dev, c["x"], c["lens"], c["rec"], c["perm"])
    worst = max(worst, check_against(got, c["y"], c["stats"], "npts %d t_max %d %s" % (c["npts"], c["t_max"], c["kind"])))
    for b, n in enumerate(c["lens"]):
      assert not got[0][b, int(n):].any()                      # padding frames are zeros
  print("worst over the parity cases: %.3g ulp" % worst)


@pytest.mark.parametrize("npts", [68, 4])
def test_the_identity_record_returns_the_inputs_bits(dev, npts):
  for t_max in AC.T_MAXES:
    c = AC.case(npts, t_max, "identity")
    y, _ = aug_call(dev, c["x"], c["lens"], c["rec"], c["perm"])
    live = AC.live_rows(c["x"], c["lens"])
    assert live.sum() == sum(AC.LENS)
    assert y[live].tobytes() == np.asarray(c["x"])[live].tobytes() and not y[~live].any()


def test_an_exact_motion_gives_the_integer_answer(dev):
  x, rec, want = AC.exact_case()
  for in_place in (False, True):
    y, stats = aug_call(dev, x, [4], rec, AC.perm_for(4), in_place=in_place)
    assert stats[0].tolist() == [10.0, 20.0, 5.0, 5.0]
    assert y.tobytes() == want.tobytes()


# ---- batch semantics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["identity", "full_jitter"])
def test_batch_semantics(dev, kind):
  for t_max in AC.T_MAXES:
    x, lens = AC.semantics_case(t_max)
    rec = AC.records(kind, 4)
    want_y, want_stats, _ = AC.augment(x, lens, rec, AC.perm_for(68))
    live = AC.live_rows(x, lens)
    got = aug_call(dev, x, lens, rec, AC.perm_for(68))
    check_against(got, want_y, want_stats, "semantics %s t_max %d" % (kind, t_max))
    y, stats = got
    assert not y[~live].any() and np.isfinite(y).all()          # garbage padding, the masked row, the NaN rows: zeros
    assert (y[live] != 0).any(axis=(1, 2)).all()
    assert live[3].sum() == t_max - 1 and live[0].sum() == 4    # lens[3] > t_max is clamped
    assert stats[2].tolist() == [0.0, 0.0, 0.0, 0.0] and not y[2].any()      # the clip without a LIVE row
    # the statistics are those of the LIVE rows alone: the same clip with its EMPTY rows zeroed has them bit for bit
    clean = np.where(live[:, :, None, None], x, np.float32(0))
    again = aug_call(dev, clean, lens, rec, AC.perm_for(68))
    assert again[1].tobytes() == stats.tobytes() and again[0].tobytes() == y.tobytes()


def test_no_value_of_mirror_perm_reads_outside_the_row(dev):
  c = AC.case(68, 9, "full_jitter")
  perm = list(c["perm"])
  perm[3], perm[40], perm[67] = -5, 10 ** 6, 68
  rec = np.array(c["rec"])
  rec.view(np.float64)[:, 13] = 1.0                            # every clip mirrors
  x = np.array(c["x"])
  want_y, want_stats, _ = AC.augment(x, c["lens"], rec, perm)  # (the restatement clamps the indices)
  y, stats = aug_call(dev, x, c["lens"], rec, perm)
  assert np.isfinite(y).all()
  check_against((y, stats), want_y, want_stats, "clamped mirror_perm")
  # one row on its own with NaN all around it on the device: a read outside the row would show in the output
  one = x[2:3, 4:5]
  from lipreading_amd import _C
  L = _C.lib()
  wide = torch.full((3, 68, 3), float("nan"), dtype=torch.float32, device=dev)
  wide[1] = torch.from_numpy(one[0, 0]).to(dev)
  out = torch.full((3, 68, 3), float("nan"), dtype=torch.float32, device=dev)
  lens_d = torch.ones(1, dtype=torch.int32, device=dev)
  rec_d = torch.from_numpy(rec[2:3].view(np.int64)).to(dev)
  perm_d = torch.tensor(perm, dtype=torch.int32, device=dev)
  need = L.lr_lmk_augment_workspace_bytes(1)
  work = torch.empty(need, dtype=torch.uint8, device=dev)
  _C.check(L.lr_lmk_augment_f32(wide[1].data_ptr(), lens_d.data_ptr(), rec_d.data_ptr(), perm_d.data_ptr(),
                                out[1].data_ptr(), None, work.data_ptr(), need, 1, 1, 68, _C.stream_handle()), "augment")
  torch.cuda.synchronize()
  got = out.cpu().numpy()
  assert np.isnan(got[0]).all() and np.isnan(got[2]).all() and np.isfinite(got[1]).all()
  want = AC.augment(one, [1], rec[2:3], perm)[0]
  assert AC.worst_ulps(got[1][None, None], want) <= 1.0


# ---- determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npts", [68, 4, 1])
def test_two_launches_in_place_and_per_clip_calls_give_the_same_bits(dev, npts):
  if npts == 68:
    x, lens = AC.semantics_case(12)
  else:
    lmk, offsets, n = AC.clips(npts)
    x, lens = AC.pad(lmk, offsets, n, 12, fill=-3.5), np.asarray(n, dtype=np.int32)
  B = len(lens)
  perm = AC.perm_for(npts)
  for kind in ("full", "full_jitter"):
    rec = AC.records(kind, B)
    a = aug_call(dev, x, lens, rec, perm)
    b = aug_call(dev, x, lens, rec, perm)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = aug_call(dev, x, lens, rec, perm, in_place=True)
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()
    d = aug_call(dev, x, lens, rec, perm, want_stats=False)
    assert d[0].tobytes() == a[0].tobytes()
    for s in range(B):
      one = aug_call(dev, x[s:s + 1], lens[s:s + 1], rec[s:s + 1], perm)
      assert one[0][0].tobytes() == a[0][s].tobytes() and one[1][0].tobytes() == a[1][s].tobytes(), (kind, s)
    want_y, want_stats, _ = AC.augment(x, lens, rec, perm)
    check_against(a, want_y, want_stats, "determinism input npts %d %s" % (npts, kind))


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_error_codes_and_the_workspace_query(dev):
  from lipreading_amd import _C
  L = _C.lib()
  B, t_max, npts = 2, 3, 4
  n = B * t_max * npts * 3
  x = torch.zeros(2 * n + 64, dtype=torch.float32, device=dev)   # room for a y that starts where x ends
  y = torch.zeros_like(x)
  lens = torch.ones(B, dtype=torch.int32, device=dev)
  rec = torch.from_numpy(AC.records("identity", B).view(np.int64)).to(dev)
  perm = torch.arange(npts, dtype=torch.int32, device=dev)
  need = L.lr_lmk_augment_workspace_bytes(B)
  work = torch.empty(need, dtype=torch.uint8, device=dev)
  good = dict(x=x.data_ptr(), lens=lens.data_ptr(), rec=rec.data_ptr(), perm=perm.data_ptr(), y=y.data_ptr(), stats=None,
              work=work.data_ptr(), work_bytes=need, B=B, t_max=t_max, npts=npts)

  def call(**change):
    a = dict(good, **change)
    return L.lr_lmk_augment_f32(a["x"], a["lens"], a["rec"], a["perm"], a["y"], a["stats"], a["work"], a["work_bytes"],
                                a["B"], a["t_max"], a["npts"], _C.stream_handle())

  assert call() == _C.LR_OK and call(y=good["x"]) == _C.LR_OK
  for change in (dict(npts=0), dict(npts=257), dict(npts=-1), dict(B=0), dict(B=-3), dict(t_max=0),
                 dict(B=65536, t_max=32768), dict(B=1 << 30, t_max=2)):
    assert call(**change) == _C.LR_ERR_UNSUPPORTED, change
  for name in ("x", "lens", "rec", "perm", "y", "work"):
    assert call(**{name: None}) == _C.LR_ERR_INVALID_ARG, name
  four = ctypes.sizeof(ctypes.c_float)
  for shift in (four, -four, (n - 1) * four, -(n - 1) * four):
    assert call(y=good["x"] + shift) == _C.LR_ERR_INVALID_ARG, shift     # overlapping without being equal
  assert call(y=good["x"] + n * four) == _C.LR_OK                        # back to back is no overlap
  assert call(work_bytes=need - 1) == _C.LR_ERR_WORKSPACE and call(work_bytes=0) == _C.LR_ERR_WORKSPACE
  torch.cuda.synchronize()
  # the query answers 0 exactly where the entry refuses the argument it is asked about
  for b in (-1, 0):
    assert L.lr_lmk_augment_workspace_bytes(b) == 0
  for b in (1, 2, 32, 33, 4096):
    got = L.lr_lmk_augment_workspace_bytes(b)
    assert got >= b * 5 * 8 and got % 16 == 0


# ---- Python, up to the loaders ----------------------------------------------------------------------------------------
def _caption(rng, n):
  return np.array([1] + list(rng.randint(4, 64, n)) + [2])


def _landmark_dataset(n, seed):
  rng = np.random.RandomState(seed)
  out = []
  for t in np.sort(rng.randint(6, 20, n)):
    clip = AC.clips(68, lens=(int(t),), seed=int(rng.randint(1 << 20)))[0]
    out.append((clip.astype(np.float64), _caption(rng, rng.randint(2, 5))))
  return out


def _same_batches(got, want, where):
  got, want = list(got), list(want)
  assert len(got) == len(want) > 0
  for k, (a, b) in enumerate(zip(got, want)):
    assert len(a) == len(b) == 4
    for i, (x, y) in enumerate(zip(a, b)):
      assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, (where, k, i)
      assert torch.equal(x, y), (where, k, i)
  return got


def test_augment_landmarks_is_the_c_entry(dev):
  from lipreading_amd import landmarks
  c = AC.case(68, 12, "full_jitter")
  want = aug_call(dev, c["x"], c["lens"], c["rec"], c["perm"])
  x_d = torch.from_numpy(np.array(c["x"])).to(dev)
  lens_d = torch.from_numpy(np.array(c["lens"])).to(dev)
  rec = np.array(c["rec"])
  y, stats = landmarks.augment_landmarks(x_d, lens_d, rec, return_stats=True)
  assert y.shape == x_d.shape and y.dtype == torch.float32 and stats.shape == (3, 4) and stats.dtype == torch.float64
  assert y.cpu().numpy().tobytes() == want[0].tobytes() and stats.cpu().numpy().tobytes() == want[1].tobytes()
  assert torch.equal(x_d.cpu(), torch.from_numpy(np.array(c["x"])))          # out of place: the input stays
  assert torch.equal(landmarks.augment_landmarks(x_d, lens_d.long(), torch.from_numpy(rec.view(np.int64)).to(dev)), y)
  z = x_d.clone()
  assert landmarks.augment_landmarks(z, lens_d, rec, out=z) is z and torch.equal(z, y)     # in place
  four = torch.from_numpy(np.array(AC.case(4, 9, "mirror")["x"])).to(dev)
  got = landmarks.augment_landmarks(four, lens_d, AC.records("mirror", 3), perm=(3, 2, 1, 0))
  assert AC.worst_ulps(got.cpu().numpy(), AC.case(4, 9, "mirror")["y"]) <= 1.0
  for bad in (dict(perm=(1, 2, 3, 0)), dict(perm=(0, 1, 2)), dict(perm=(0, 1, 2, 4))):
    with pytest.raises(ValueError):
      landmarks.augment_landmarks(four, lens_d, AC.records("mirror", 3), **bad)
  with pytest.raises(ValueError):
    landmarks.augment_landmarks(four, lens_d, AC.records("mirror", 2), perm=(3, 2, 1, 0))
  with pytest.raises(ValueError):
    landmarks.augment_landmarks(four.double(), lens_d, AC.records("mirror", 3), perm=(3, 2, 1, 0))
  with pytest.raises(ValueError):
    landmarks.augment_landmarks(four, lens_d[:2], AC.records("mirror", 3), perm=(3, 2, 1, 0))
  with pytest.raises(ValueError):
    landmarks.augment_landmarks(four, lens_d, AC.records("mirror", 3), perm=(3, 2, 1, 0), out=four[:, :5])


def test_loaders_yield_the_augmented_collates_batches(dev):
  from lipreading_amd import landmarks
  from lipreading_amd.augment import AugmentSpec, LandmarkAugmentSpec
  from lipreading_amd.data import make_collate_fn
  from lipreading_amd.dataset import make_loader
  ds = _landmark_dataset(11, seed=9)
  plan = ((0, 4), (4, 8), (8, 11))
  spec = LandmarkAugmentSpec.parse(FULL, seed=5)
  aug_spec = AugmentSpec.parse("tjitter=0.2,tmask=2x3", seed=5)
  pose = landmarks.PoseSpec(AC.PC.template(68), radius=2, scale=True)
  today = list(make_loader(ds, 4, make_collate_fn(dev)))
  kw = dict(prefetch=2, workers=2, device=dev)

  def expected(base, pass_no):
    out = []
    for (lo, hi), (x, frame_lens, chars, char_lens) in zip(plan, base):
      rec = spec.draw(pass_no, range(lo, hi), frame_lens.numpy())
      y = landmarks.augment_landmarks(x.clone(), frame_lens.to(dev), rec)
      out.append((y, frame_lens, chars, char_lens))
    return out

  # alone: the plain pad collate's batch, augmented; two passes draw with two pass numbers
  alone = make_loader(ds, 4, None, lmk_augment=spec, **kw)
  first = _same_batches(alone, expected(today, 0), "lmk_augment alone, pass 0")
  assert sum(not torch.equal(a[0], b[0]) for a, b in zip(first, today)) == 3      # it reached every batch
  for a, b in zip(first, today):                                # lengths, chars and shapes are unchanged
    assert a[0].shape == b[0].shape and all(torch.equal(p, q) for p, q in zip(a[1:], b[1:]))
    for s, n in enumerate(a[1]):
      assert not a[0][s, int(n):].any()
  _same_batches(alone.plain(), today, "plain pass of the landmark-augmented loader")
  assert alone.pass_no == 1
  _same_batches(alone, expected(today, 1), "lmk_augment alone, pass 1")
  # with the frame map: the temporally augmented loader's batch, augmented
  mapped = make_loader(ds, 4, None, augment=aug_spec, **kw)
  both = make_loader(ds, 4, None, augment=aug_spec, lmk_augment=spec, **kw)
  _same_batches(both, expected(list(mapped), 0), "with augment=")
  _same_batches(both.plain(), today, "plain pass with augment=")
  # with pose=, and with all three
  posed = list(make_loader(ds, 4, None, pose=pose, **kw))
  with_pose = make_loader(ds, 4, None, pose=pose, lmk_augment=spec, **kw)
  _same_batches(with_pose, expected(posed, 0), "with pose=")
  _same_batches(with_pose.plain(), posed, "plain pass with pose=")
  mapped_posed = make_loader(ds, 4, None, pose=pose, augment=aug_spec, **kw)
  three = make_loader(ds, 4, None, pose=pose, augment=aug_spec, lmk_augment=spec, **kw)
  _same_batches(three, expected(list(mapped_posed), 0), "with pose= and augment=")
  # a loader built without it yields today's batches
  _same_batches(make_loader(ds, 4, None, **kw), today, "default prefetch")
  _same_batches(make_loader(ds, 4, None, lmk_augment=None, **kw), today, "lmk_augment=None prefetch")
  # the identity policy issues the launch and changes nothing
  _same_batches(make_loader(ds, 4, None, lmk_augment=LandmarkAugmentSpec(), **kw), today, "identity policy")
  for x in (alone, mapped, both, with_pose, mapped_posed, three):
    x.close()


# ---- driver -----------------------------------------------------------------------------------------------------------
def test_driver_trains_on_augmented_landmarks(dev, tmp_path, capsys):
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synth/nano", n_videos=6, captions_per_video=3, seed=11)
  flags = ["--root=" + root, "--data=synth/nano", "--batch_size=4", "--enable_ctc=True", "--ctc_only=True",
           "--rnn_type=GRU", "--hidden_size=32", "--max_epochs=1", "--prefetch=2", "--lmk_augment=" + FULL]
  out = driver.run(**driver.parse_flags(flags))
  text = capsys.readouterr().out
  assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["ctc_loss"])
  assert "Augmenting the training landmarks: " + "mirror=0.5,rot=10.0/10.0/15.0" in text
  train, val, test = out["loaders"]
  assert train.lmk_augment is not None and train.lmk_augment.seed == driver.DEFAULTS["seed"]
  assert val.lmk_augment is None and test.lmk_augment is None and train.pass_no == 1
  for loader in out["loaders"]:
    loader.close()
