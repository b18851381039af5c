"""GPU: lr_rnnt_loss_forward / lr_rnnt_loss_backward / lr_rnnt_greedy_decode through lipreading_amd.transducer against
the float64 restatement of tests/transducer_cases.py, the contract's edge cases, TransducerHead end to end,
train.transducer_step and the driver's --transducer.

The tolerances are 8 x the float32 restatement's own error on the same case (tests/transducer_cases.py); the device's
measured errors are in DESIGN.md §33."""
import functools

import numpy as np
import pytest
import torch

from lipreading_amd import _C
from lipreading_amd import transducer as TR
from tests import transducer_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
  return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(name, reduction="mean"):
  """The float64 restatement of a case: computed once, shared, never modified."""
  return K.reference(name, reduction=reduction)


@functools.lru_cache(maxsize=None)
def greedy_reference(name):
  return K.greedy_reference(name)


def device_run(case, dev, reduction="mean", grad_out=None, transposed=False, preset=None):
  """rnnt_loss on a case's float32 tensors and autograd back to e, p, joint weight and bias."""
  e = case["e"].to(dev)
  if transposed:
    leaf_e = e.transpose(0, 1).contiguous().requires_grad_(True)   # (T, B, J)
    e_in = leaf_e.transpose(0, 1)
  else:
    leaf_e = e.requires_grad_(True)
    e_in = leaf_e
  p, W, b = (case[k].to(dev).requires_grad_(True) for k in ("p", "W", "b"))
  if preset is not None:
    W.grad, b.grad = preset[0].clone(), preset[1].clone()
  loss, status, info = TR.rnnt_loss(e_in, p, W, b, case["mask"].to(dev), case["labels"].to(dev),
                                    case["frame_lens"].to(dev), case["label_lens"].to(dev), reduction)
  loss.backward(grad_out)
  ge = leaf_e.grad.transpose(0, 1) if transposed else leaf_e.grad
  return dict(loss=loss.detach(), status=int(status.item()), nll=info["nll"], sample_status=info["sample_status"],
              grads=dict(e=ge, p=p.grad, W=W.grad, b=b.grad))


def errors(got, want):
  out = dict(loss=K.rel_err(got["loss"].cpu(), want["loss"]), nll=K.rel_err(got["nll"].cpu(), want["nll"]))
  out.update({k: K.rel_err(got["grads"][k].cpu(), want["grads"][k]) for k in ("e", "p", "W", "b")})
  return out


def same_bits(a, b):
  return all(torch.equal(a["grads"][k], b["grads"][k]) for k in ("e", "p", "W", "b")) and \
      torch.equal(a["nll"], b["nll"]) and torch.equal(a["loss"], b["loss"])


# ---- parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_loss_and_gradients_match_float64(dev, name):
  got = device_run(K.make_case(name, torch.float32), dev)
  want = reference(name)
  assert got["status"] == 0 and got["sample_status"].cpu().tolist() == want["sample_status"]
  err, tol = errors(got, want), K.tolerance(name)
  print("%s: " % name + "  ".join("%s %.3e (tol %.3e)" % (k, err[k], tol[k]) for k in err))
  for k in err:
    assert err[k] <= tol[k], (name, k, err[k], tol[k])


# ---- contract ----------------------------------------------------------------------------------------------------------
def test_sum_and_mean_agree(dev):
  case = K.make_case("ragged", torch.float32)
  s, m = device_run(case, dev, "sum"), device_run(case, dev, "mean")
  want = reference("ragged", "sum")
  err, tol = errors(s, want), K.tolerance("ragged")
  for k in err:
    assert err[k] <= tol[k], (k, err[k], tol[k])
  assert torch.equal(s["nll"], m["nll"])
  assert abs(float(s["loss"]) - 3 * float(m["loss"])) <= 1e-6 * abs(float(s["loss"]))
  assert K.rel_err(3 * m["grads"]["W"].cpu(), s["grads"]["W"].cpu().double()) <= 1e-6


def test_a_device_scalar_grad_out_scales_the_gradients(dev):
  case = K.make_case("odd", torch.float32)
  one = device_run(case, dev)
  two = device_run(case, dev, grad_out=torch.tensor(2.0, device=dev))       # a power of two: exact
  third = device_run(case, dev, grad_out=torch.tensor(0.37, device=dev))
  want, tol = reference("odd"), K.tolerance("odd")
  for k in ("e", "p", "W", "b"):
    assert torch.equal(two["grads"][k], 2 * one["grads"][k]), k
    assert K.rel_err(third["grads"][k].cpu(), 0.37 * want["grads"][k]) <= tol[k] + 2.0 ** -23, k


def test_a_transposed_view_of_e_is_accepted(dev):
  case = K.make_case("ragged", torch.float32)
  assert same_bits(device_run(case, dev), device_run(case, dev, transposed=True))


def test_bad_samples_contribute_nothing_and_leave_their_neighbours_alone(dev):
  clean = K.make_case("vocab", torch.float32)
  bad = K.make_case("vocab", torch.float32)
  bad["labels"][1, 1] = 0                # inside label_lens[1] = 3: a blank as a label
  bad["frame_lens"][2] = 18              # T + 1
  a, b = device_run(clean, dev, "sum"), device_run(bad, dev, "sum")
  assert b["sample_status"].cpu().tolist() == [0, K.BAD_ID, K.BAD_LENGTH, 0] and b["status"] == 0
  assert b["nll"][[1, 2]].cpu().tolist() == [0.0, 0.0]
  for k in ("e", "p"):
    assert not b["grads"][k][[1, 2]].any()
    assert torch.equal(a["grads"][k][[0, 3]], b["grads"][k][[0, 3]])
  assert torch.equal(a["nll"][[0, 3]], b["nll"][[0, 3]])
  assert torch.equal(b["loss"], b["nll"][0] + b["nll"][3])
  masked = K.make_case("vocab", torch.float32)
  masked["labels"][0, 0] = 2             # a masked class
  toolong = K.make_case("vocab", torch.float32)
  toolong["label_lens"][3] = 8           # U + 1
  assert device_run(masked, dev)["sample_status"].cpu().tolist() == [K.BAD_ID, 0, 0, 0]
  assert device_run(toolong, dev)["sample_status"].cpu().tolist() == [0, 0, 0, K.BAD_LENGTH]


def test_a_batch_without_a_usable_sample_sets_the_batch_status(dev):
  case = K.make_case("ragged", torch.float32)
  case["frame_lens"][:] = 0
  out = device_run(case, dev)
  assert out["status"] == 1 and float(out["loss"]) == 0.0
  assert out["sample_status"].cpu().tolist() == [K.BAD_LENGTH] * 3
  assert not any(bool(g.any()) for g in out["grads"].values())


def test_rejected_shapes(dev):
  L = _C.lib()
  assert L.lr_rnnt_workspace_bytes(2, 9, 5, 65, 256) > 0
  for args in ((2, 9, _C.LR_RNNT_MAX_U + 1, 65, 256), (2, 9, 5, _C.LR_RNNT_MAX_CLASSES + 1, 256),
               (2, 9, 5, 65, _C.LR_RNNT_MAX_JOINT + 1), (2, _C.LR_RNNT_MAX_T + 1, 5, 65, 256), (0, 9, 5, 65, 256),
               (2, 0, 5, 65, 256), (2, 9, -1, 65, 256), (2, 9, 5, 1, 256), (2, 9, 5, 65, 0)):
    assert L.lr_rnnt_workspace_bytes(*args) == 0, args
  J = _C.LR_RNNT_MAX_JOINT + 1
  z = lambda *s: torch.zeros(*s, device=dev)
  with pytest.raises(ValueError):
    TR.rnnt_loss(z(1, 2, J), z(1, 2, J), z(5, J), z(5), torch.ones(5, device=dev),
                 torch.ones((1, 1), dtype=torch.int32, device=dev), torch.tensor([2], device=dev),
                 torch.tensor([1], device=dev))
  with pytest.raises(_C.LipReadingHipError):
    TR.rnnt_loss(torch.zeros(1, 2, 8), z(1, 2, 8), z(5, 8), z(5), torch.ones(5, device=dev),
                 torch.ones((1, 1), dtype=torch.int32, device=dev), torch.tensor([2], device=dev),
                 torch.tensor([1], device=dev))


def test_two_runs_give_the_same_bits(dev):
  case = K.make_case("vocab", torch.float32)
  assert same_bits(device_run(case, dev), device_run(case, dev))


def test_accumulate_adds_onto_existing_weight_gradients(dev):
  case = K.make_case("odd", torch.float32)
  plain = device_run(case, dev)
  g = torch.Generator().manual_seed(5)
  preset = (torch.randn(case["W"].shape, generator=g).to(dev), torch.randn(case["b"].shape, generator=g).to(dev))
  acc = device_run(case, dev, preset=preset)
  assert torch.equal(acc["grads"]["W"], preset[0] + plain["grads"]["W"])
  assert torch.equal(acc["grads"]["b"], preset[1] + plain["grads"]["b"])
  assert torch.equal(acc["grads"]["e"], plain["grads"]["e"])


# ---- greedy ------------------------------------------------------------------------------------------------------------
def device_greedy(case, dev, chunk=None, max_symbols=5, max_out=None, sizes=None, **over):
  t = {k: (over[k] if k in over else case[k]).to(dev) for k in ("e", "tables", "W", "b", "mask")}
  sizes = (case["frame_lens"] if sizes is None else sizes).to(dev)
  T = t["e"].shape[1]
  width = T * max_symbols if max_out is None else max_out
  if chunk is None:
    return TR.rnnt_greedy(t["e"], sizes, t["tables"], t["W"], t["b"], t["mask"], max_symbols=max_symbols, max_out=width)
  out = None
  for t0 in range(0, T, chunk):
    out = TR.rnnt_greedy(t["e"][:, t0:t0 + chunk], (sizes - t0).clamp(0, chunk), t["tables"], t["W"], t["b"], t["mask"],
                         state=None if out is None else out["state"], max_symbols=max_symbols, max_out=width)
  return out


def as_lists(out):
  lens = out["lens"].cpu().tolist()
  width = out["ids"].shape[1]
  cut = lambda x: [x[b, :min(n, width)].cpu().tolist() for b, n in enumerate(lens)]
  return dict(ids=cut(out["ids"]), frames=cut(out["frames"]), logp=cut(out["logp"]), lens=lens,
              forced=out["forced"].cpu().tolist())


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_greedy_matches_float64(dev, name):
  want, margin, logit_err = greedy_reference(name)
  # the condition is on the oracle alone: every decision is clear of what float32 can blur
  assert margin >= K.MARGIN_FACTOR * max(logit_err, K.FP32_ERROR[name][6]), (name, margin, logit_err)
  got = as_lists(device_greedy(K.make_case(name, torch.float32), dev))
  assert got["ids"] == want["ids"] and got["lens"] == want["lens"]
  assert got["frames"] == want["frames"] and got["forced"] == want["forced"]
  flat = lambda rows: torch.tensor([v for r in rows for v in r], dtype=torch.float64)
  if sum(want["lens"]):
    err, tol = K.rel_err(flat(got["logp"]), flat(want["logp"])), K.tolerance(name)
    print("%s: greedy logp %.3e (tol %.3e), %d symbols, forced %s" % (name, err, max(tol["loss"], tol["nll"]),
                                                                     sum(want["lens"]), want["forced"]))
    assert err <= max(tol["loss"], tol["nll"]), (name, err)


@pytest.mark.parametrize("chunk", [1, 3, 5])
def test_chunked_greedy_gives_the_one_shot_bits(dev, chunk):
  for name in ("ragged", "vocab"):
    case = K.make_case(name, torch.float32)
    whole, parts = device_greedy(case, dev), device_greedy(case, dev, chunk=chunk)
    for k in ("ids", "frames", "logp", "lens", "forced"):
      assert torch.equal(whole[k], parts[k]), (name, k)
    assert torch.equal(whole["state"]["context"], parts["state"]["context"])
    assert torch.equal(parts["state"]["frame_base"], case["frame_lens"].to(dev).clamp(0, case["e"].shape[1]))


def test_greedy_caps_the_symbols_of_a_frame_and_counts_what_does_not_fit(dev):
  case = K.make_case("ragged", torch.float64)
  b = case["b"].clone()
  b[0] = -50.0                                     # the blank never wins: every frame is forced to end
  want = K.greedy(case["e"], case["frame_lens"], case["tables"], case["W"], b, case["mask"], max_symbols=3)
  c32 = K.make_case("ragged", torch.float32)
  got = as_lists(device_greedy(c32, dev, max_symbols=3, b=b.float()))
  sizes = case["frame_lens"].tolist()
  assert got["lens"] == [3 * n for n in sizes] == want["lens"] and got["forced"] == sizes == want["forced"]
  assert got["ids"] == want["ids"] and got["frames"] == want["frames"]
  small = device_greedy(c32, dev, max_symbols=3, max_out=4, b=b.float())
  assert small["lens"].cpu().tolist() == want["lens"] and tuple(small["ids"].shape) == (3, 4)
  assert small["ids"].cpu().tolist() == [(r + [0] * 4)[:4] for r in want["ids"]]


# ---- module and loop ---------------------------------------------------------------------------------------------------
def _replica(head, hidden, labels, flens, llens, dtype):
  """TransducerHead.loss restated on the CPU in `dtype`: (loss, gradients by parameter name + 'hidden')."""
  sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in head.named_parameters()}
  h = hidden.detach().cpu().to(dtype).requires_grad_(True)
  E, C = head.embed_dim, head.context
  e = h @ sd["enc_proj.weight"].t() + sd["enc_proj.bias"]
  tabs = [sd["embed.weight"] @ sd["pred_proj.weight"][:, k * E:(k + 1) * E].t() for k in range(C)]
  tabs[0] = tabs[0] + sd["pred_proj.bias"]
  lab = labels.cpu().long()
  y = torch.cat((lab.new_zeros((lab.shape[0], C)), lab), 1)
  U1 = lab.shape[1] + 1
  p = tabs[0][y[:, C - 1:C - 1 + U1]]
  if C == 2:
    p = p + tabs[1][y[:, 0:U1]]
  loss, _, _, _ = K.rnnt_loss(e, p, sd["joint.weight"], sd["joint.bias"], head.output_mask.cpu().to(dtype), labels.cpu(),
                              flens.cpu(), llens.cpu())
  loss.backward()
  grads = {k: v.grad for k, v in sd.items()}
  grads["hidden"] = h.grad
  return loss.detach(), grads


def test_head_loss_backward_matches_a_float64_replica(dev):
  from lipreading_amd.data import default_char2idx
  c2i = default_char2idx()
  torch.manual_seed(3)
  head = TR.TransducerHead(24, 64, c2i, joint_dim=256, embed_dim=16, context=2).to(dev)
  _, T, U, V1, _, flens, llens, _ = K.CASES["vocab"]
  allowed = torch.tensor([c for c in range(1, V1) if head.output_mask[c] != 0])
  labels = allowed[torch.randint(0, len(allowed), (4, U))].to(torch.int32).to(dev)
  hidden = torch.randn(4, T, 24, device=dev, requires_grad=True)
  fl, ll = torch.tensor(flens, dtype=torch.int32, device=dev), torch.tensor(llens, dtype=torch.int32, device=dev)
  loss, status, _ = head.loss(hidden, fl, labels, ll)
  loss.backward()
  assert int(status.item()) == 0
  l64, g64 = _replica(head, hidden, labels, fl, ll, torch.float64)
  l32, g32 = _replica(head, hidden, labels, fl, ll, torch.float32)
  # the rule of tests/transducer_cases.py on this case: 8 x the float32 replica's own error (its largest over the
  # tensors, each relative to its own maximum), no smaller than what a float32 word can hold
  e32 = max([K.rel_err(g32[k], g64[k]) for k in g64] + [K.rel_err(l32, l64), K.FP32_HALF_ULP])
  got = {k: v.grad for k, v in head.named_parameters()}
  got["hidden"] = hidden.grad
  assert K.rel_err(loss.detach().cpu(), l64) <= K.TOL_FACTOR * e32
  for k in g64:
    err = K.rel_err(got[k].cpu(), g64[k])
    print("head %s: %.3e (tol %.3e)" % (k, err, K.TOL_FACTOR * e32))
    assert err <= K.TOL_FACTOR * e32, (k, err, e32)


def _small_setup(dev, frames_per_clip=None, hidden=32, clips=4):
  from lipreading_amd.data import default_char2idx, make_collate_fn
  from lipreading_amd.encoder import VideoEncoder
  from lipreading_amd.optim import FlatParameters, FusedAdam
  c2i = default_char2idx()
  rng = np.random.RandomState(0)
  items = []
  for n in sorted(rng.randint(20, 40, clips)) if frames_per_clip is None else [frames_per_clip] * clips:
    items.append((rng.randn(n, 68, 3).astype(np.float32), np.r_[1, rng.randint(4, 64, 6), 2]))
  batch = make_collate_fn(dev)(items)
  torch.manual_seed(0)
  enc = VideoEncoder(204, hidden, rnn_type='GRU', bidirectional=True, enable_ctc=True, vocab_size=64, char2idx=c2i).to(dev)
  head = TR.TransducerHead(2 * hidden, 64, c2i, joint_dim=64, embed_dim=16, context=2).to(dev)
  opts = (FusedAdam(FlatParameters(enc), lr=3e-3), FusedAdam(FlatParameters(head), lr=3e-3))
  return enc.train(), head.train(), opts, batch


def test_transducer_step_moves_every_parameter(dev):
  from lipreading_amd import train as T
  enc, head, opts, (frames, frame_lens, chars, char_lens) = _small_setup(dev)
  before = {k: v.detach().clone() for m in (enc, head) for k, v in m.named_parameters()}
  for _ in range(2):
    rnnt, ctc, status, info = T.transducer_step(enc, head, opts, frames, frame_lens, chars, char_lens, grad_norm=50)
    assert int(status.item()) == 0 and np.isfinite(float(rnnt)) and np.isfinite(float(ctc))
  for m in (enc, head):
    for k, v in m.named_parameters():
      assert not torch.equal(before[k], v.detach()), k
  with pytest.raises(NotImplementedError):
    T.transducer_step(enc, head, opts, frames, frame_lens, chars, char_lens, grad_sync=lambda s: 1.0)


def test_transducer_step_moves_nothing_when_the_status_says_skip(dev):
  from lipreading_amd import train as T
  enc, head, opts, (frames, frame_lens, chars, char_lens) = _small_setup(dev, frames_per_clip=3)   # 7 labels, 3 frames
  before = {k: v.detach().clone() for m in (enc, head) for k, v in m.named_parameters()}
  _, _, status, _ = T.transducer_step(enc, head, opts, frames, frame_lens, chars, char_lens, grad_norm=50)
  assert int(status.item()) == 1 and opts[0].skipped_steps() == 1 and opts[1].skipped_steps() == 1
  for m in (enc, head):
    for k, v in m.named_parameters():
      assert torch.equal(before[k], v.detach()), k


def test_sixty_steps_on_two_clips_lower_the_loss(dev):
  from lipreading_amd import train as T
  enc, head, opts, (frames, frame_lens, chars, char_lens) = _small_setup(dev, hidden=64, clips=2)
  losses = [T.transducer_step(enc, head, opts, frames, frame_lens, chars, char_lens, grad_norm=50)[0] for _ in range(60)]
  first, last = float(losses[0]), float(losses[-1])
  print("transducer loss: step 1 %.4f, step 60 %.4f" % (first, last))
  assert np.isfinite(last) and last < first


@pytest.mark.parametrize("encoder", ["rnn", "transformer"])
def test_driver_trains_a_transducer(dev, tmp_path, capsys, encoder):
  import os
  from lipreading_amd import dataset as DS
  from lipreading_amd import driver
  root = str(tmp_path)
  DS.write_synthetic_dataview(root, "synthetic/nano", n_videos=6, captions_per_video=5, seed=11)
  flags = driver.parse_flags(["--data=synthetic/nano", "--batch_size=5", "--enable_ctc=True", "--ctc_only=True",
                              "--rnn_type=GRU", "--bidirectional=True", "--hidden_size=32", "--learning_rate=3e-4",
                              "--grad_norm=400", "--cuda=True", "--transducer=True", "--transducer_joint=64",
                              "--transducer_embed=16", "--encoder=" + encoder, "--num_layers=1", "--root=" + root,
                              "--max_epochs=1"])
  out = driver.run(**flags)
  text = capsys.readouterr().out
  h = out["history"]
  assert len(h) == 1 and np.isfinite(h[0]["transducer_loss"]) and h[0]["transducer_loss"] > 0
  # (an untrained head free-runs up to max_symbols characters per frame: its CER is far above 1, and only has to be a number)
  assert np.isfinite(h[0]["ctc_loss"]) and np.isfinite(h[0]["val_cer"]) and h[0]["val_cer"] >= 0.0
  assert "Transducer CER (val): " in text and "Training transducer_loss: " in text
  assert os.path.isfile(out["transducer_path"]) and out["transducer_path"].endswith("best_transducer.pth")
  assert "Restored " + out["transducer_path"] in text
  saved = torch.load(out["transducer_path"], map_location="cpu")
  assert sorted(saved) == sorted(out["transducer"].state_dict()) and "output_mask" not in saved
  for k, v in out["transducer"].state_dict().items():
    assert torch.equal(v.cpu(), saved[k]), k
