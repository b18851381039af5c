"""The yardstick of the N-best minimum error rate objective (include/lipreading_hip.h A6h): a torch-CPU
restatement of the specification, float64 by default, and the cases the CPU and GPU tests share.

The restatement starts from LEAF LOGITS: log_softmax, then F.ctc_loss(reduction='none') once per usable hypothesis, a
softmax over the hypotheses' likelihoods, the expected risk, and autograd back to the logits.  Every gradient row of the
objective sums to zero over the classes, so the gradient at the logits equals the gradient at the log-probabilities,
which is what the kernels return.  Hypotheses that are empty, rejected or infeasible never enter the graph: the `inf`
F.ctc_loss gives an infeasible one would turn the whole gradient into NaN.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

USED, EMPTY, REJECTED, INFEASIBLE = 0, 1, 2, 3

# ---- tolerances -------------------------------------------------------------------------------------------------------
# The rule: evaluate the restatement in float32 on the CPU as well; e32 = that evaluation's largest error against
# float64, relative to the case's largest float64 magnitude of the same quantity; take the maximum over PARITY_CASES.
# The device must agree with float64 within 8 x that (a different summation order and fused multiply-adds, nothing
# more).  The three e32 below are the maxima over parity_cases() as printed by `python -m tests.mwer_cases` on an
# x86-64 CPU (the run behind DESIGN.md §25: the gradient's maximum at T76_N16_C65, 2e-6 to 1.5e-5 at T = 17).
E32_GRAD = 9.57e-5
E32_LOSS = 2.90e-6
E32_LL = 4.09e-7
TOL_GRAD, TOL_LOSS, TOL_LL = 8 * E32_GRAD, 8 * E32_LOSS, 8 * E32_LL
# the posterior is exp(ll - logsumexp): an absolute error of ll becomes a relative one of p, and p <= 1
TOL_POST_ABS = 1e-4


def slot_status(ids, length, risk, frames, C, blank, max_hyp_len):
  """The status of one slot, by the specification's order: empty, rejected, infeasible, used."""
  if length < 0:
    return EMPTY
  if length > max_hyp_len or not math.isfinite(risk):
    return REJECTED
  y = [int(c) for c in ids[:length]]
  if any(c < 0 or c >= C or c == blank for c in y):
    return REJECTED
  repeats = sum(1 for i in range(1, length) if y[i] == y[i - 1])
  if frames == 0 or frames < length + repeats:
    return INFEASIBLE
  return USED


def oracle(logits, sizes, hyp_ids, hyp_lens, risk, blank=0, reduction='mean', dtype=torch.float64, grad_out=1.0):
  """logits (B, T, C) array; sizes (B,) or None; hyp_ids (B, N, W) ints; hyp_lens (B, N); risk (B, N).  Returns a dict
  of numpy arrays: loss, grad (B, T, C) at the logits, hyp_ll, posterior, status (B, N), utt_risk (B,), batch_status."""
  x = torch.as_tensor(np.asarray(logits)).to(dtype).clone().requires_grad_(True)
  B, T, C = x.shape
  hyp_ids, hyp_lens = np.asarray(hyp_ids), np.asarray(hyp_lens)
  risk = np.asarray(risk, dtype=np.float64)
  N, W = hyp_ids.shape[1], hyp_ids.shape[2]
  sizes = np.full(B, T) if sizes is None else np.clip(np.asarray(sizes), 0, T)
  lp = F.log_softmax(x, dim=-1)
  status = np.zeros((B, N), dtype=np.int32)
  hyp_ll = np.full((B, N), -np.inf)
  post = np.zeros((B, N))
  utt_risk = np.zeros(B)
  total, used = x.new_zeros(()), 0
  for b in range(B):
    n_b = int(sizes[b])
    lls, slots = [], []
    for n in range(N):
      L = int(hyp_lens[b, n])
      status[b, n] = slot_status(hyp_ids[b, n], L, float(risk[b, n]), n_b, C, blank, W)
      if status[b, n] != USED:
        continue
      tgt = torch.as_tensor(hyp_ids[b, n, :L].astype(np.int64)).reshape(1, L)
      nll = F.ctc_loss(lp[b, :n_b].unsqueeze(1), tgt, torch.tensor([n_b]), torch.tensor([L]), blank=blank,
                       reduction='none', zero_infinity=False)[0]
      if not bool(torch.isfinite(nll)):      # -inf log-probabilities emptied the lattice
        status[b, n] = INFEASIBLE
        continue
      lls.append(-nll)
      slots.append(n)
    if not slots:
      continue
    ll = torch.stack(lls)
    p = torch.softmax(ll, dim=0)
    R = (p * torch.as_tensor(risk[b, slots]).to(dtype)).sum()
    total = total + R
    used += 1
    hyp_ll[b, slots] = ll.detach().double().numpy()
    post[b, slots] = p.detach().double().numpy()
    utt_risk[b] = float(R.detach())
  loss = total / max(used, 1) if reduction == 'mean' else total
  if used:
    loss.backward(torch.as_tensor(grad_out, dtype=dtype))
  grad = np.zeros((B, T, C)) if x.grad is None else x.grad.double().numpy()
  return dict(loss=float(loss.detach()), grad=grad, hyp_ll=hyp_ll, posterior=post, status=status, utt_risk=utt_risk,
              batch_status=int(used == 0))


# ---- cases ------------------------------------------------------------------------------------------------------------
def make_case(seed, T, C, N, base_lens, sizes=None, blank=0, width=None, doubles=True):
  """One batch: utterance b's hypotheses are perturbations of one random base string of base_lens[b] characters — 0 to 3
  substitutions, every fifth hypothesis with a character deleted — over N(0, 1) logits.  Independent random strings
  would collapse the posterior to one-hot and test nothing.  The base strings carry doubled characters; ids past the
  lengths are junk (out-of-range values among them).  Risks are small integers, as edit distances are."""
  rng = np.random.RandomState(seed)
  B = len(base_lens)
  chars = [c for c in range(C) if c != blank]
  W = max(1, max(base_lens)) if width is None else width
  ids = rng.randint(-3, C + 40, size=(B, N, W)).astype(np.int32)          # junk everywhere, the strings go on top
  lens = np.zeros((B, N), dtype=np.int32)
  k = 0
  for b, L in enumerate(base_lens):
    base = []
    for _ in range(L):                                                    # no doubles by accident: they are planted
      base.append(chars[rng.randint(len(chars))] if len(chars) == 1 else
                  rng.choice([c for c in chars if not base or c != base[-1]]))
    if doubles and L >= 2:
      base[1] = base[0]                                                   # one doubled character, two from 33 up
      if L >= 33 and L < T - 2:
        base[L // 2] = base[L // 2 - 1]
    for n in range(N):
      y = list(base)
      for _ in range(rng.randint(0, 4) if n else 0):                      # slot 0 is the base itself
        if y and len(chars) > 1:
          i = rng.randint(len(y))
          y[i] = chars[(chars.index(y[i]) + 1 + rng.randint(len(chars) - 1)) % len(chars)]
      if k % 5 == 4 and y:
        del y[rng.randint(len(y))]
      k += 1
      ids[b, n, :len(y)] = y
      lens[b, n] = len(y)
  logits = rng.randn(B, T, C).astype(np.float32)
  risk = rng.randint(0, 6, size=(B, N)).astype(np.float32)
  if sizes is None:
    sizes = np.full(B, T, dtype=np.int32)
  return dict(logits=logits, sizes=np.asarray(sizes, dtype=np.int32), hyp_ids=ids, hyp_lens=lens, risk=risk,
              blank=blank, T=T, C=C, N=N, B=B)


# hypothesis lengths per padded length T: at 31/32 and 63/64 characters the 2L+1 states cross 64 and 128 lanes; 75
# characters with one doubled pair need 76 frames (infeasible at 75).  Two sets for the long T, crossed with N and C.
_LENS = {1: ([0, 1, 0, 1, 2, 1],), 2: ([0, 1, 2, 1, 2, 0],), 17: ([0, 1, 2, 7, 8, 16],),
         75: ([0, 1, 31, 32, 63, 75], [2, 33, 64, 1, 63, 32]), 76: ([0, 1, 31, 32, 63, 75], [2, 33, 64, 1, 75, 63])}


def _sizes(T, base_lens, rng):
  """Ragged: the first utterance is full, the first later one with at most one character has ONE frame, the others
  lie between what their base string needs and T."""
  sizes, one = [], False
  for b, L in enumerate(base_lens):
    need = L + (1 if L >= 2 else 0) + (1 if 33 <= L < T - 2 else 0)
    if b == 0:
      sizes.append(T)
    elif L <= 1 and not one:
      sizes.append(1)
      one = True
    else:
      lo = min(T, need + 7)     # (a substitution can double a character on both sides)
      sizes.append(int(rng.randint(lo, T + 1)))
  return sizes


def parity_cases():
  """(name, case) over T x N x C, B = 6 each."""
  out = []
  for ti, T in enumerate((1, 2, 17, 75, 76)):
    for ni, N in enumerate((1, 2, 3, 16)):
      for ci, C in enumerate((3, 65)):
        sets = _LENS[T]
        base_lens = sets[(ni + ci) % len(sets)]
        seed = 1000 * T + 10 * N + C
        sizes = _sizes(T, base_lens, np.random.RandomState(seed + 1))
        out.append(("T%d_N%d_C%d" % (T, N, C), make_case(seed, T, C, N, base_lens, sizes=sizes)))
  return out


def wide_case():
  """max_hyp_len at its limit: 513 states, two per thread of the lattice kernel."""
  return make_case(77, 260, 65, 3, [256, 130], sizes=[260, 259], width=256)


def second_posteriors(res):
  """Per utterance with at least two used slots, the second-largest posterior."""
  out = []
  for b in range(res["posterior"].shape[0]):
    p = np.sort(res["posterior"][b][res["status"][b] == USED])
    if len(p) >= 2:
      out.append(p[-2])
  return out


def assert_spread(res, N):
  """A fixed condition on the ORACLE alone: at least half of the utterances have a second-largest posterior >= 0.02
  (a one-hot posterior would make the gradient vanish and the comparison empty).  One slot has no second."""
  if N < 2:
    return
  B = res["posterior"].shape[0]
  assert sum(p >= 0.02 for p in second_posteriors(res)) * 2 >= B, second_posteriors(res)


def rel_errors(got, want):
  """(gradient, loss, hyp_ll) errors of `got` against `want`, each relative to the largest magnitude in `want`."""
  g = np.abs(got["grad"] - want["grad"]).max() / max(np.abs(want["grad"]).max(), 1e-300)
  l = abs(got["loss"] - want["loss"]) / max(abs(want["loss"]), 1e-300)
  used = want["status"] == USED
  ll = 0.0
  if used.any():
    ll = np.abs(got["hyp_ll"][used] - want["hyp_ll"][used]).max() / np.abs(want["hyp_ll"][used]).max()
  return g, l, ll


def run(case, dtype=torch.float64, **kw):
  return oracle(case["logits"], case["sizes"], case["hyp_ids"], case["hyp_lens"], case["risk"], blank=case["blank"],
                dtype=dtype, **kw)


if __name__ == "__main__":
  worst = [0.0, 0.0, 0.0]
  for name, case in parity_cases():
    r64, r32 = run(case), run(case, dtype=torch.float32)
    assert (r64["status"] == r32["status"]).all()
    assert_spread(r64, case["N"])
    e = rel_errors(r32, r64)
    worst = [max(a, b) for a, b in zip(worst, e)]
    print("%-14s e32 grad %.2e loss %.2e ll %.2e  |grad|max %.2e  second p %s" % (
        name, e[0], e[1], e[2], np.abs(r64["grad"]).max(), np.round(second_posteriors(r64), 3)))
  print("max e32: grad %.3e loss %.3e ll %.3e" % tuple(worst))
