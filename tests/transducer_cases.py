"""The transducer head restated in torch on the CPU (float64 the yardstick, float32 the measure of what fp32 can hold),
the named cases of tests/test_transducer_cpu.py and tests/test_gpu_transducer.py, and their tolerances.

Nothing here touches the package: the model, the lattice, the status rules and the greedy decoder are written out again
from include/lipreading_hip.h (A6i), the gradients come from autograd through the plain recursion.
"""
import itertools

import torch

BAD_ID, BAD_LENGTH = -1, -2
NEG = -1.0e30   # "impossible" inside the recursion: logaddexp(NEG, x) == x exactly and its gradient is 0, never NaN


# ---- the model ---------------------------------------------------------------------------------------------------------
def joint_log_probs(e, p, W, b, mask):
  """(B, T, U1, V1) masked log-softmax of W . tanh(e_t + p_u) + b."""
  z = torch.tanh(e[:, :, None, :] + p[:, None, :, :])
  logits = z @ W.t() + b
  logits = logits.masked_fill(mask == 0, float("-inf"))
  return torch.log_softmax(logits, dim=-1)


def sample_status(Tb, Ub, labels, T, U, V1, mask):
  if Tb < 1 or Tb > T or Ub < 0 or Ub > U:
    return BAD_LENGTH
  for y in labels[:Ub].tolist():
    if y <= 0 or y >= V1 or mask[y] == 0:
      return BAD_ID
  return 0


def lattice_nll(lp, labels, Tb, Ub):
  """-log P(y | x) of one sample: lp (T, U1, V1), the recursion vectorised over anti-diagonals."""
  blank = lp[:Tb, :Ub + 1, 0]
  idx = labels[:Ub].long()
  lab = lp[:Tb, :Ub, :].gather(2, idx[None, :, None].expand(Tb, Ub, 1))[:, :, 0] if Ub > 0 else lp.new_zeros((Tb, 0))
  us = torch.arange(Ub + 1)
  neg = lp.new_full((Ub + 1,), NEG)
  a = neg.clone()
  a[0] = 0.0
  for d in range(1, Tb + Ub):
    t = d - us
    valid = (t >= 0) & (t < Tb)
    from_blank = torch.where(valid & (t >= 1), a + blank[(t - 1).clamp(0, Tb - 1), us], neg)
    prev_u = torch.cat((neg[:1], a[:-1]))
    if Ub > 0:
      from_label = torch.where(valid & (us >= 1), prev_u + lab[t.clamp(0, Tb - 1), (us - 1).clamp(0, Ub - 1)], neg)
    else:
      from_label = neg
    a = torch.where(valid, torch.logaddexp(from_blank, from_label), neg)
  return -(a[Ub] + blank[Tb - 1, Ub])


def rnnt_loss(e, p, W, b, mask, labels, frame_lens, label_lens, reduction="mean"):
  """(loss, batch status, nll (B,), sample status list) as the entry point defines them."""
  B, T, _ = e.shape
  U, V1 = p.shape[1] - 1, W.shape[0]
  lp = joint_log_probs(e, p, W, b, mask)
  nll, stats = [], []
  for i in range(B):
    st = sample_status(int(frame_lens[i]), int(label_lens[i]), labels[i], T, U, V1, mask)
    stats.append(st)
    nll.append(lattice_nll(lp[i], labels[i], int(frame_lens[i]), int(label_lens[i])) if st == 0 else lp.new_zeros(()))
  nll = torch.stack(nll)
  used = sum(1 for s in stats if s == 0)
  loss = nll.sum() / (max(used, 1) if reduction == "mean" else 1)
  return loss, int(used == 0), nll, stats


def brute_force_nll(lp, labels, Tb, Ub):
  """The sum over every alignment, path by path (small lattices only)."""
  total = None
  for blanks in itertools.combinations(range(Tb - 1 + Ub), Tb - 1):
    t = u = 0
    s = lp.new_zeros(())
    for step in range(Tb - 1 + Ub):
      if step in blanks:
        s = s + lp[t, u, 0]
        t += 1
      else:
        s = s + lp[t, u, int(labels[u])]
        u += 1
    s = s + lp[Tb - 1, Ub, 0]
    total = s if total is None else torch.logaddexp(total, s)
  return -total


def occupancy_grad(lp, labels, Tb, Ub):
  """d nll / d logits (T, U1, V1) from alpha, beta and the occupancies, by plain loops."""
  T, U1, V1 = lp.shape
  al = torch.full((Tb, Ub + 1), NEG, dtype=lp.dtype)
  be = torch.full((Tb, Ub + 1), NEG, dtype=lp.dtype)
  for t in range(Tb):
    for u in range(Ub + 1):
      if t == 0 and u == 0:
        al[t, u] = 0.0
        continue
      x = al[t - 1, u] + lp[t - 1, u, 0] if t > 0 else torch.tensor(NEG, dtype=lp.dtype)
      y = al[t, u - 1] + lp[t, u - 1, int(labels[u - 1])] if u > 0 else torch.tensor(NEG, dtype=lp.dtype)
      al[t, u] = torch.logaddexp(x, y)
  for t in reversed(range(Tb)):
    for u in reversed(range(Ub + 1)):
      if t == Tb - 1 and u == Ub:
        be[t, u] = lp[t, u, 0]
        continue
      x = be[t + 1, u] + lp[t, u, 0] if t + 1 < Tb else torch.tensor(NEG, dtype=lp.dtype)
      y = be[t, u + 1] + lp[t, u, int(labels[u])] if u < Ub else torch.tensor(NEG, dtype=lp.dtype)
      be[t, u] = torch.logaddexp(x, y)
  logZ = be[0, 0]
  g = torch.zeros_like(lp)
  for t in range(Tb):
    for u in range(Ub + 1):
      if t + 1 < Tb:
        ob = torch.exp(al[t, u] + lp[t, u, 0] + be[t + 1, u] - logZ)
      else:
        ob = torch.exp(al[t, u] + lp[t, u, 0] - logZ) if u == Ub else lp.new_zeros(())
      ol = torch.exp(al[t, u] + lp[t, u, int(labels[u])] + be[t, u + 1] - logZ) if u < Ub else lp.new_zeros(())
      g[t, u] = (ob + ol) * torch.exp(lp[t, u])
      g[t, u, 0] -= ob
      if u < Ub:
        g[t, u, int(labels[u])] -= ol
  return g


# ---- the greedy decoder ------------------------------------------------------------------------------------------------
def new_state(B, context):
  return dict(context=[[0] * context for _ in range(B)], lens=[0] * B, forced=[0] * B, frame_base=[0] * B,
              ids=[[] for _ in range(B)], frames=[[] for _ in range(B)], logp=[[] for _ in range(B)])


def greedy(e, sizes, tables, W, b, mask, state=None, max_symbols=5, max_out=None, margins=None):
  """The decoder of lr_rnnt_greedy_decode on (B, T, J) `e`; `state` is continued in place.  Returns the state: ids,
  frames, logp as lists per sample (at most max_out entries), lens, forced.  margins: a list that receives
  (top-1 logit - top-2 logit, the logits) of every decision."""
  B, T, _ = e.shape
  context, V1 = tables.shape[0], tables.shape[1]
  st = new_state(B, context) if state is None else state
  width = T * max_symbols if max_out is None else max_out
  st.setdefault("max_out", width)
  for i in range(B):
    n = max(0, min(int(sizes[i]), T)) if sizes is not None else T
    ctx = st["context"][i]
    for t in range(n):
      for s in range(max_symbols):
        pre = e[i, t] + tables[0, ctx[0]]
        if context == 2:
          pre = pre + tables[1, ctx[1]]
        logits = (W @ torch.tanh(pre) + b).masked_fill(mask == 0, float("-inf"))
        top = float(logits.max())
        k = int((logits == top).nonzero()[0])   # ties: the lowest class
        if margins is not None:
          rest = torch.cat((logits[:k], logits[k + 1:]))
          margins.append((top - float(rest.max()), logits.clone()))
        if k == 0:
          break
        if st["lens"][i] < st["max_out"]:
          st["ids"][i].append(k)
          st["frames"][i].append(st["frame_base"][i] + t)
          st["logp"][i].append(float(torch.log_softmax(logits, 0)[k]))
        st["lens"][i] += 1
        ctx[:] = [k] + ctx[:-1]
        if s == max_symbols - 1:
          st["forced"][i] += 1
    st["frame_base"][i] += n
  return st


# ---- the named cases ---------------------------------------------------------------------------------------------------
# name: (B, T, U, V1, J, frame_lens, label_lens, context).  The kernel's tile is 32 nodes x 32 classes, the joint width is
# padded to 32: `odd` has a V1 (37) and a J (45) that are multiples of neither the tile nor a float4.
CASES = {
    "ragged": (3, 9, 5, 5, 8, [9, 1, 5], [5, 2, 0], 1),
    "vocab": (4, 17, 7, 65, 256, [17, 12, 9, 17], [7, 3, 5, 0], 2),
    "wide": (2, 5, 70, 65, 64, [5, 4], [70, 33], 2),
    "workload": (2, 75, 40, 65, 256, [75, 60], [40, 31], 2),
    "odd": (2, 6, 4, 37, 45, [6, 5], [4, 3], 2),
    "maxu": (2, 2, 256, 9, 16, [2, 2], [256, 200], 2),
}


def make_case(name, dtype=torch.float64):
  """The case's tensors in `dtype`, drawn in float64 from the name's own seed (the float32 ones are its roundings)."""
  B, T, U, V1, J, flens, llens, context = CASES[name]
  g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
  r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  mask = torch.ones(V1, dtype=torch.float64)
  for c in ((3,) if V1 < 9 else (2, 5)):   # stand-ins for PAD + 1 and BOS + 1
    mask[c] = 0
  allowed = torch.tensor([c for c in range(1, V1) if mask[c] != 0])
  labels = allowed[torch.randint(0, len(allowed), (B, max(U, 1)), generator=g)][:, :U].to(torch.int32)
  W = r(V1, J) * (3.0 / J ** 0.5)
  b = r(V1) * 0.1
  b[0] += 2.0   # a blank likely enough that the greedy path is a mix of frames and symbols
  out = dict(e=r(B, T, J), p=r(B, U + 1, J), W=W, b=b, mask=mask, tables=r(context, V1, J) * 0.7)
  out = {k: v.to(dtype) for k, v in out.items()}
  out.update(labels=labels, frame_lens=torch.tensor(flens, dtype=torch.int32),
             label_lens=torch.tensor(llens, dtype=torch.int32), context=context, name=name)
  return out


def reference(name, dtype=torch.float64, reduction="mean"):
  """loss, nll and the gradients (e, p, W, b) of the case in `dtype`."""
  c = make_case(name, dtype)
  leaves = [c[k].clone().requires_grad_(True) for k in ("e", "p", "W", "b")]
  loss, status, nll, stats = rnnt_loss(*leaves, c["mask"], c["labels"], c["frame_lens"], c["label_lens"], reduction)
  loss.backward()
  return dict(loss=loss.detach(), status=status, nll=nll.detach(), sample_status=stats,
              grads=dict(zip(("e", "p", "W", "b"), (l.grad for l in leaves))))


def rel_err(a, ref):
  """|a - ref| relative to |ref| for the losses; relative to the tensor's maximum for gradients (the caller's choice of
  `ref`'s scale: max |ref|)."""
  scale = float(ref.abs().max())
  return float((a.double() - ref.double()).abs().max()) / (scale if scale > 0 else 1.0)


# The float32 restatement's error against the float64 one, per case: (loss, nll, d_e, d_p, d_W, d_b, largest logit error
# on the greedy path).  MEASURED by `python tests/transducer_cases.py` (torch on the CPU, the run of this file's commit);
# a device result may differ from float64 by TOL = 8 x these.
FP32_ERROR = {
    "ragged": (3.83e-09, 3.22e-08, 9.81e-08, 3.18e-07, 1.9e-07, 1.69e-07, 4.4e-07),   # smallest greedy margin 1.03
    "vocab": (8.76e-08, 1.07e-07, 5.72e-07, 1.59e-07, 1.99e-07, 4.05e-08, 1.53e-06),   # smallest greedy margin 0.0144
    "wide": (1.18e-07, 1.05e-07, 1.33e-05, 1.45e-05, 7.69e-06, 4.54e-06, 1.19e-06),   # smallest greedy margin 0.00279
    "workload": (4.49e-09, 9.11e-08, 6.35e-06, 9.94e-07, 1.38e-06, 7.53e-08, 1.46e-06),   # smallest greedy margin 0.000847
    "odd": (5.32e-08, 3.84e-08, 2.7e-07, 3.56e-07, 3.54e-07, 4.67e-08, 1.17e-06),   # smallest greedy margin 0.0532
    "maxu": (3.87e-08, 7.3e-09, 1.61e-06, 1.48e-05, 1.6e-06, 5.24e-07, 5.99e-07),   # smallest greedy margin 0.264
}
TOL_FACTOR = 8.0
MARGIN_FACTOR = 64.0
# A float32 evaluation can land closer to float64 than float32 can express (3.8e-9 on `ragged`'s loss: luck, not
# precision).  The device returns float32 words, and storing the float64 answer itself in one costs up to half an ulp,
# 2^-24 relative: a measured error below that is taken as that.
FP32_HALF_ULP = 2.0 ** -24


def tolerance(name):
  loss, nll, de, dp, dw, db, _ = (max(v, FP32_HALF_ULP) for v in FP32_ERROR[name])
  return dict(loss=TOL_FACTOR * loss, nll=TOL_FACTOR * nll, e=TOL_FACTOR * de, p=TOL_FACTOR * dp, W=TOL_FACTOR * dw,
              b=TOL_FACTOR * db)


def greedy_reference(name, max_symbols=5):
  """The float64 greedy decode of the case, its smallest top-1 / top-2 margin and the float32 restatement's largest
  logit error along that path."""
  c = make_case(name)
  margins = []
  st = greedy(c["e"], c["frame_lens"], c["tables"], c["W"], c["b"], c["mask"], max_symbols=max_symbols, margins=margins)
  c32 = make_case(name, torch.float32)
  m32 = []
  greedy(c32["e"], c32["frame_lens"], c32["tables"], c32["W"], c32["b"], c32["mask"], max_symbols=max_symbols,
         margins=m32)
  err = 0.0
  for (_, l64), (_, l32) in zip(margins, m32):
    keep = torch.isfinite(l64)
    err = max(err, float((l32.double()[keep] - l64[keep]).abs().max()))
  return st, min(m for m, _ in margins), err


def measure():
  for name in CASES:
    r64, r32 = reference(name), reference(name, torch.float32)
    row = [rel_err(r32["loss"], r64["loss"]), rel_err(r32["nll"], r64["nll"])]
    row += [rel_err(r32["grads"][k], r64["grads"][k]) for k in ("e", "p", "W", "b")]
    _, margin, err = greedy_reference(name)
    row.append(err)
    print('    "%s": (%s),   # smallest greedy margin %.3g' % (name, ", ".join("%.3g" % v for v in row), margin))


if __name__ == "__main__":
  measure()
