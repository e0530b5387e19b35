"""Plain references for the dense-SNN training kernels (csrc/train_dense.hip); no GPU.

  gemm_chain / gemm_f64 / gemm_mag     C[i][j] = sum_r A[r][i] B[r][j]: the float32 fmaf chain the
                                       kernels promise, the float64 product and |A|^T |B|
  lif_save_ref                         float32 h, s of the multi_step_LIF scan, by the oracle
  lif_backward_ref32                   DESIGN.md section 10's recurrence in numpy float32
  lif_backward_ref64                   the same in float64, with an a-priori per-element bound
  TorchDenseSNN64                      the training forward of examples/tcja/models.py:191-255 in
                                       float64 torch; its backward is torch.autograd's
  scan_vjp / duq_vjp / hand_gradients  the hand-derived backward (a second derivation)
"""
import numpy as np
import torch

from oracle import snn_oracle as oracle

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24                       # unit roundoff of float32
SURROGATES = ("fast_sigmoid", "atan", "slayer", "smooth_step", "piecewise_linear")


# ---- the two products ---------------------------------------------------------------------------

def gemm_chain(a_ri, b_rj):
  """C[i][j] = fmaf chain over r ascending of A[r][i] B[r][j], from +0, float32."""
  a_ri, b_rj = np.asarray(a_ri, F32), np.asarray(b_rj, F32)
  assert a_ri.ndim == 2 and b_rj.ndim == 2 and a_ri.shape[0] == b_rj.shape[0]
  return oracle.fseq_matmul(np.ascontiguousarray(a_ri.T), b_rj)


def gemm_f64(a_ri, b_rj):
  return np.asarray(a_ri, F64).T @ np.asarray(b_rj, F64)


def gemm_mag(a_ri, b_rj):
  """sum_r |A[r][i]| |B[r][j]| in float64."""
  return np.abs(np.asarray(a_ri, F64)).T @ np.abs(np.asarray(b_rj, F64))


def gamma(n):
  """gamma_n = n u / (1 - n u): a chain of n fused multiply-adds is within gamma_n sum |a||b| of
  the exact sum (n roundings, one per fmaf; Higham, Accuracy and Stability, section 3.1)."""
  return n * U / (1.0 - n * U)


# ---- forward scan -------------------------------------------------------------------------------

def lif_save_ref(cur, tau, vth=1.0, vr=0.0):
  """float32 currents [T, ...] -> (h, s) float32 [T, ...] from a zero state: the pre-reset
  potential u + (x - (u - v_reset)) / tau and the spike of oracle.multi_step_lif, step by step."""
  cur = np.asarray(cur, F32)
  u = np.zeros(cur.shape[1:], F32)
  hs, ss = np.empty_like(cur), np.empty_like(cur)
  for t in range(cur.shape[0]):
    hs[t] = (u + (cur[t] - (u - F32(vr))) / F32(tau)).astype(F32)
    u, s = oracle.multi_step_lif(u, cur[t], tau=tau, v_threshold=vth, v_reset=vr)
    ss[t] = s
  return hs, ss


# ---- surrogate derivatives, spiking_learning.py:139-241 -----------------------------------------

def sg64(name, x):
  x = np.asarray(x, F64)
  if name == "fast_sigmoid":
    return 1.0 / (10.0 * np.abs(x) + 1.0) ** 2
  if name == "atan":
    return 1.0 / (1.0 + (np.pi * x) ** 2)
  if name == "slayer":
    return np.exp(-5.0 * np.abs(x))
  if name == "smooth_step":
    return ((x < 0.5) & (x >= -0.5)).astype(F64)
  if name == "piecewise_linear":
    return np.maximum(1.0 - 2.0 * np.abs(x), 0.0)
  raise ValueError(name)


def sg32(name, x):
  """The same in float32, one rounding per operation."""
  x = np.asarray(x, F32)
  one = F32(1)
  if name == "fast_sigmoid":
    d = F32(10) * np.abs(x) + one
    return one / (d * d)
  if name == "atan":
    p = F32(np.pi) * x
    return one / (one + p * p)
  if name == "slayer":
    return np.exp(F32(-5) * np.abs(x)).astype(F32)
  if name == "smooth_step":
    return ((x < F32(0.5)) & (x >= F32(-0.5))).astype(F32)
  if name == "piecewise_linear":
    return np.maximum(one - F32(2) * np.abs(x), F32(0))
  raise ValueError(name)


def sg_rel_err(name, x):
  """Bound on the relative error of a float32 sigma'(x) against sg64 at the same x, per element.

  smooth_step is exact.  piecewise_linear: 2|x| is exact, the subtraction rounds once: u.
  fast_sigmoid: d = fl(fl(10|x|) + 1) is within 2u, d d within 5u, the reciprocal 6u.  atan:
  float32 pi is 0.47u off, p = fl(pi x) within 1.47u, 1 + p p within 5u, the reciprocal 6u.
  Both are charged 8u.  slayer: fl(-5|x|) moves the argument by 5|x|u, which exp turns into a
  relative 5|x|u, and expf is charged 2 ulp = 4u (twice the device library's documented 1)."""
  x = np.abs(np.asarray(x, F64))
  if name == "smooth_step":
    return np.zeros_like(x)
  if name == "piecewise_linear":
    return np.full_like(x, U)
  if name in ("fast_sigmoid", "atan"):
    return np.full_like(x, 8 * U)
  if name == "slayer":
    return 5.0 * x * U * (1 + U) + 4 * U
  raise ValueError(name)


# ---- backward scan ------------------------------------------------------------------------------

def _is_pow2(x):
  m, _ = np.frexp(float(x))
  return m == 0.5


def lif_backward_ref32(h, gs, tau, vth, surrogate):
  """DESIGN.md section 10 in float32, t = T-1 .. 0 from gu_T = 0:
    gh = gs sigma'(h - vth) + gu (1 - s);  gI = gh / tau;  gu = gh (1 - 1/tau),  s = (h - vth >= 0).
  Every operation rounds once (numpy float32 arrays; nothing is fused)."""
  h, gs = np.asarray(h, F32), np.asarray(gs, F32)
  tau, vth, one = F32(tau), F32(vth), F32(1)
  keep = one - one / tau
  gI = np.empty_like(h)
  gu = np.zeros(h.shape[1:], F32)
  for t in range(h.shape[0] - 1, -1, -1):
    x = h[t] - vth
    s = (x >= 0).astype(F32)
    gh = gs[t] * sg32(surrogate, x) + gu * (one - s)
    gI[t] = gh / tau
    gu = gh * keep
  return gI


def lif_backward_ref64(h, gs, tau, vth, surrogate):
  """The recurrence in float64 at the float32 x = fl(h - vth), and a bound on what a float32
  evaluation (lif_backward_ref32's order of operations) may differ from it, per element.

  Beside the values run their magnitudes Gh = |gs| sigma' + Gu (1 - s), Gu = Gh keep, and the
  errors.  With e the surrogate's relative error (sg_rel_err), u = 2^-24 and one rounding for
  each product, sum and quotient:
    Eh = |gs| sigma' ((1 + e)(1 + u)^2 - 1) + (1 - s) (Eu (1 + u) + Gu u)       [(1 - s) is exact]
    EI = (Eh (1 + u) + Gh u) / tau
    Eu = Eh keep + (Gh + Eh) keep ((1 + ek)(1 + u) - 1)
  where ek is the relative error of float32 keep = fl(1 - fl(1 / tau)): 0 when tau is a power of
  two, else (inv / keep + 1) u (1 + u).  A few units of the smallest subnormal are added for
  results that underflow.  Returns (gI float64, EI float64)."""
  h, gs = np.asarray(h, F32), np.asarray(gs, F32)
  tau64, vth32 = float(F32(tau)), F32(vth)
  inv = 1.0 / tau64
  keep = 1.0 - inv
  ek = 0.0 if _is_pow2(tau64) else (inv / keep + 1.0) * U * (1 + U)
  tiny = 4 * 2.0 ** -149
  gI, EI = np.empty(h.shape, F64), np.empty(h.shape, F64)
  gu = np.zeros(h.shape[1:], F64)
  Gu, Eu = np.zeros_like(gu), np.zeros_like(gu)
  for t in range(h.shape[0] - 1, -1, -1):
    x = (h[t] - vth32).astype(F64)
    ns = 1.0 - (x >= 0)
    sg, e = sg64(surrogate, x), sg_rel_err(surrogate, x)
    g = gs[t].astype(F64)
    gh = g * sg + gu * ns
    Gh = np.abs(g) * sg + Gu * ns
    Eh = np.abs(g) * sg * ((1 + e) * (1 + U) ** 2 - 1) + ns * (Eu * (1 + U) + Gu * U) + tiny
    gI[t] = gh / tau64
    EI[t] = (Eh * (1 + U) + Gh * U) / tau64 + tiny
    gu = gh * keep
    Eu = Eh * keep + (Gh + Eh) * keep * ((1 + ek) * (1 + U) - 1) + tiny
    Gu = Gh * keep
  return gI, EI


def planted_h(rng, shape, vth, shift=0.0):
  """Random float32 potentials around vth + shift whose first entries put x = fl(h - vth) on the
  surrogates' edges.  Returns (h, reached): the edge values e of {-0.5, 0.0, 0.5, 0.25, -0.25}
  for which some float32 h has x == e exactly.  x is monotonic in h, so a search of the
  neighbours of fl(vth + e) is exhaustive: with vth = 1 every edge is reached, while float32 0.7
  is an odd multiple of 2^-24 and h near 1.2 an even one, so no h gives x == 0.5 there.  Beside
  each +-0.5 go the nearest h on either side whose x is strictly beyond the edge (the finest
  step x can take there; several h may round to the edge itself).  x == -0.0 cannot occur: h == vth subtracts to +0.0."""
  vth = F32(vth)
  h = (vth + F32(shift) + rng.standard_normal(shape) * 0.6).astype(F32)
  vals, reached = [], set()
  for e in (-0.5, 0.0, 0.5, 0.25, -0.25):
    near = [vth + F32(e)]
    for _ in range(3):
      near = [np.nextafter(near[0], F32(-np.inf))] + near + [np.nextafter(near[-1], F32(np.inf))]
    hit = [c for c in near if c - vth == F32(e)]
    base = hit[0] if hit else near[3]
    if hit:
      reached.add(e)
    vals.append(base)
    if abs(e) == 0.5:
      lo = hi = base                      # the nearest h whose x is strictly beyond the edge
      while not lo - vth < F32(e):
        lo = np.nextafter(lo, F32(-np.inf))
      while not hi - vth > F32(e):
        hi = np.nextafter(hi, F32(np.inf))
      vals += [lo, hi]
  flat = h.reshape(-1)
  flat[:len(vals)] = vals
  return h, reached


# ---- the hand-derived backward ------------------------------------------------------------------

def scan_vjp(h, s, gs, tau, vth, name):
  """spiking_learning.py:410-414 differentiated: no gradient through the reset condition.
  sigma' is taken at the float32 difference fl(h - vth) the kernel forms, then all is float64."""
  T = h.shape[0]
  gI = np.zeros_like(gs)
  gu = np.zeros_like(gs[0])
  for t in range(T - 1, -1, -1):
    x = (np.asarray(h[t], F32) - F32(vth)).astype(F64)
    gh = gs[t] * sg64(name, x) + gu * (1.0 - s[t])
    gI[t] = gh / tau
    gu = gh * (1.0 - 1.0 / tau)
  return gI


def duq_vjp(g, leaf, bits, quantized):
  """quant.py:428-491: prune's grad_zero, DuQ with a straight-through round."""
  w = leaf["kernel"].astype(F64)
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  mask = leaf.get("prune_0", {}).get("mask")
  if mask is not None:
    g = g * mask
  if not quantized or a == -1.0:
    return g, 0.0, 0.0
  L = 2 ** (bits - 1) - 1
  x = leaf["kernel"] / np.float32(a)
  inside = np.abs(x.astype(F64)) <= 1
  r = np.round(np.clip(x, -1, 1) * np.float32(L)).astype(F64) / L
  gc = float((g * r).sum())
  gw = np.where(inside, g * c / a, 0.0)
  ga = float(-np.where(inside, g * c * w / (a * a), 0.0).sum())
  return gw, ga, gc


def hand_gradients(params, x_bt, m0, m1, h1, s1, h2, s2, gL, wq2, tau, vth, name, quantized,
                   bits=8, group=10):
  """{layer: (gW, ga, gc)} of DenseSNN's parameters for the logits' gradient gL [B, N // group],
  by the rules written out: the vote (models.py:253-255), scan_vjp, the two products and duq_vjp.
  h, s [T, B, N] and the masks are the forward's saved values; wq2 is layer 2's kernel_fwd."""
  m0, m1 = np.asarray(m0, F64), np.asarray(m1, F64)
  s1, s2 = np.asarray(s1, F64), np.asarray(s2, F64)
  T = s2.shape[0]
  gs2 = np.repeat(np.asarray(gL, F64), group, axis=1)[None].repeat(T, 0) / (group * T)
  gI2 = scan_vjp(h2, s2, gs2, tau, vth, name)
  x1 = s1 * m1
  gwq2 = np.einsum("tbk,tbn->kn", x1, gI2)
  gs1 = np.einsum("tbn,kn->tbk", gI2, np.asarray(wq2, F64)) * m1
  gI1 = scan_vjp(h1, s1, gs1, tau, vth, name)
  x0 = np.swapaxes(np.asarray(x_bt, F64) * m0, 0, 1)
  gwq1 = np.einsum("tbk,tbn->kn", x0, gI1)
  return {i: duq_vjp(g, params["QuantDense_%d" % i], bits, quantized)
          for i, g in ((0, gwq1), (1, gwq2))}


# ---- the literal forward in float64 torch, differentiated by autograd ----------------------------

class _SavedSpike(torch.autograd.Function):
  """Forward: the spike the float32 forward saved (x, the float64 h - vth, is not consulted, so a
  float64 forward cannot flip one).  Backward: g sigma'(saved float32 h - vth)."""

  @staticmethod
  def forward(ctx, x, s_saved, dsig):
    ctx.save_for_backward(dsig)
    return s_saved.clone()

  @staticmethod
  def backward(ctx, g):
    dsig, = ctx.saved_tensors
    return g * dsig, None, None


def _hard_tanh(x):                      # jax.nn.hard_tanh: where(x > 1, 1, where(x < -1, -1, x))
  one = torch.ones_like(x)
  return torch.where(x > 1, one, torch.where(x < -1, -one, x))


def _round_ste(x, levels):              # quant.py:441-451: round(x L) / L, the VJP passes g on
  return x + (torch.round(x * levels) / levels - x).detach()


class TorchDenseSNN64:
  """models.py:191-255 with train=True, float64, on the CPU.  Parameters are leaves `kernel[i]`,
  `a[i]`, `c[i]` (None where the tree has none); after a backward their .grad are the yardstick.
  `wq[i]` (kernel_fwd, gradient retained) is set by forward()."""

  def __init__(self, params, tau, vth, vr, surrogate, bits=8, group=10):
    self.tau, self.vth, self.vr = float(F32(tau)), float(F32(vth)), float(F32(vr))
    self.vth32 = F32(vth)
    self.surrogate, self.levels, self.group = surrogate, float(2 ** (bits - 1) - 1), group
    self.kernel, self.a, self.c, self.mask, self.wq = {}, {}, {}, {}, {}
    for i in (0, 1):
      leaf = params["QuantDense_%d" % i]
      t64 = lambda v: torch.from_numpy(np.asarray(v, F64).copy())   # noqa: E731
      self.kernel[i] = t64(leaf["kernel"]).requires_grad_(True)
      duq = leaf.get("DuQ_0")
      self.a[i] = None if duq is None else t64(duq["a"]).requires_grad_(True)
      self.c[i] = None if duq is None else t64(duq["c"]).requires_grad_(True)
      mask = leaf.get("prune_0", {}).get("mask")
      self.mask[i] = None if mask is None else t64(mask)
    self.flips = 0

  def kernel_fwd(self, i):
    """prune(DuQ(kernel)), flax_qdense.py:74-85."""
    w, a, c = self.kernel[i], self.a[i], self.c[i]
    if a is not None and float(a.detach()[0]) != -1.0:                         # quant.py:469
      w = c * _round_ste(_hard_tanh(w / a), self.levels)              # quant.py:466-467
    if self.mask[i] is not None:
      w = w * self.mask[i].detach()                                   # quant.py:491
    return w

  def _block(self, x, wq, h_saved, s_saved):
    """SpikingBlock over time: x [T, B, K] -> spikes [T, B, N] (spiking_learning.py:403-416)."""
    T = x.shape[0]
    h32 = np.asarray(h_saved, F32)
    dsig = torch.from_numpy(sg64(self.surrogate, (h32 - self.vth32).astype(F64)))
    s_sv = torch.from_numpy(np.asarray(s_saved, F64).copy())
    slack = T * 2.0 ** -22 * max(1.0, abs(self.vth))
    u = torch.zeros(x.shape[1], wq.shape[1], dtype=torch.float64)
    out = []
    for t in range(T):
      cur = x[t] @ wq
      h = u + (cur - (u - self.vr)) / self.tau                        # :410
      with torch.no_grad():
        flip = ((h - self.vth) >= 0) != (s_sv[t] != 0)
        far = flip & ((h - self.vth).abs() > slack)
        assert not bool(far.any()), (
            "float64 h disagrees with the saved spike away from the threshold: %d elements at "
            "t=%d, largest |h - vth| %.3g (allowed %.3g)"
            % (int(far.sum()), t, float((h - self.vth).abs()[far].max()), slack))
        self.flips += int(flip.sum())
      s = _SavedSpike.apply(h - self.vth, s_sv[t], dsig[t])           # :412
      u = torch.where(s.bool(), torch.full_like(h, self.vr), h)       # :414
      out.append(s)
    return torch.stack(out)

  def forward(self, x_bt, m0, m1, h1, s1, h2, s2):
    """x_bt [B, T, K], masks m0 [B, T, K] and m1 [T, B, hidden] as drawn by the forward under
    test, h / s [T, B, N] float32 as it saved them -> logits float64 [B, out // group]."""
    t64 = lambda v: torch.from_numpy(np.asarray(v, F64).copy())       # noqa: E731
    x = (t64(x_bt) * t64(m0)).transpose(0, 1)                         # models.py:192-198
    for i in (0, 1):
      self.wq[i] = self.kernel_fwd(i)
      self.wq[i].retain_grad()
    x = self._block(x, self.wq[0], h1, s1)
    x = x * t64(m1)                                                   # models.py:223-229
    x = self._block(x, self.wq[1], h2, s2)
    x = x.mean(0)                                                     # models.py:254
    return x.reshape(x.shape[0], -1, self.group).mean(-1)             # models.py:255

  def grads(self):
    """{layer: (gW, ga, gc)} after a backward, zeros where nothing reached a leaf."""
    out = {}
    for i in (0, 1):
      ga = 0.0 if self.a[i] is None or self.a[i].grad is None else float(self.a[i].grad[0])
      gc = 0.0 if self.c[i] is None or self.c[i].grad is None else float(self.c[i].grad[0])
      out[i] = (self.kernel[i].grad.numpy(), ga, gc)
    return out
