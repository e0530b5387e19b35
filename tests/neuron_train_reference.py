"""Plain references for the PLIF / LIF training kernels (csrc/train_neuron.hip); no GPU.

  neuron_save_ref                      float32 h, s of the PLIF / LIF scan, by the oracle's steps
  plif_backward_ref32 / lif_...        DESIGN.md section 17's recurrences in numpy float32
  param_sum                            the float64 parameter sum of float32 factors and sum |term|
  plif_backward_ref64 / lif_...        the same in float64 with a-priori bounds (slayer's expf)
  torch_scan_grads                     spiking_learning.py:381-385 / :432-436 in float64 torch,
                                       differentiated by torch.autograd
  conv_oracle_forward                  conv_train_reference.oracle_forward with PLIF / LIF neurons
  TorchConvDenseSNN64Neuron            conv_train_reference.TorchConvDenseSNN64 with the PLIF / LIF
                                       update and a `tau` leaf per block

Conventions: h, x, gs are [T, R, C]; m is PLIF's float32 multiplier sigmoid(tau), dec LIF's float32
decays [C].  u_{t-1} = s_{t-1} ? vr : h_{t-1} with u_{-1} = 0 is the state the forward carried,
d_t = fl(x_t - fl(u_{t-1} - vr)) the forward's own difference (PLIF).
"""
import numpy as np
import torch

from oracle import snn_oracle as oracle
from tests import conv_train_reference as cr
from tests.train_reference import F32, F64, U, gamma, sg32, sg64, sg_rel_err  # noqa: F401

PLIF, LIF = "plif", "lif"


# ---- forward scan -------------------------------------------------------------------------------

def neuron_save_ref(kind, cur, tau_param, vth=1.0, vr=0.0):
  """float32 currents [T, ...] -> (h, s) from a zero state, stepping the oracle's neuron
  (tau_param: the raw parameter, (1,) for PLIF and [C] for LIF).  h is the oracle's update before
  its reset, written out with the oracle's own sigmoid."""
  cur = np.asarray(cur, F32)
  u = np.zeros(cur.shape[1:], F32)
  hs, ss = np.empty_like(cur), np.empty_like(cur)
  k = oracle.sigmoid_f32(np.asarray(tau_param).reshape(-1)[0] if kind == PLIF else tau_param)
  for t in range(cur.shape[0]):
    if kind == PLIF:
      hs[t] = (u + (cur[t] - (u - F32(vr))) * k).astype(F32)
      u, s = oracle.parametric_leaky_if(u, cur[t], tau_param, v_threshold=vth, v_reset=vr)
    else:
      hs[t] = (u * k + cur[t]).astype(F32)
      u, s = oracle.lif(u, cur[t], tau_param, v_threshold=vth, v_reset=vr)
    ss[t] = s
  return hs, ss


def carried_state(h, vth, vr):
  """u_{t-1} for every t, float32 [T, ...]: zero, then the reset potentials."""
  h = np.asarray(h, F32)
  u = np.zeros_like(h)
  u[1:] = np.where((h[:-1] - F32(vth)) >= 0, F32(vr), h[:-1])
  return u


def plif_difference(h, x, vth, vr):
  """d_t = fl(x_t - fl(u_{t-1} - vr)), float32."""
  return (np.asarray(x, F32) - (carried_state(h, vth, vr) - F32(vr))).astype(F32)


# ---- backward scan, float32 ---------------------------------------------------------------------

def _backward32(h, gs, vth, surrogate, scale_i, keep):
  """gh = gs sigma'(h - vth) + gu (1 - s);  gI = gh scale_i (None: gh);  gu = gh keep.  Every
  operation rounds once.  -> (gI, gh), float32."""
  h, gs = np.asarray(h, F32), np.asarray(gs, F32)
  vth, one = F32(vth), F32(1)
  gI, ghs = np.empty_like(h), np.empty_like(h)
  gu = np.zeros(h.shape[1:], F32)
  for t in range(h.shape[0] - 1, -1, -1):
    x = h[t] - vth
    s = (x >= 0).astype(F32)
    gh = gs[t] * sg32(surrogate, x) + gu * (one - s)
    ghs[t] = gh
    gI[t] = gh if scale_i is None else gh * scale_i
    gu = gh * keep
  return gI, ghs


def plif_backward_ref32(h, gs, m, vth, surrogate):
  """gI_t = fl(gh_t m), gu_{t-1} = fl(gh_t keep), keep = fl(1 - m).  -> (gI, gh) float32."""
  m = F32(m)
  return _backward32(h, gs, vth, surrogate, m, F32(1) - m)


def lif_backward_ref32(h, gs, dec, vth, surrogate):
  """gI_t = gh_t, gu_{t-1} = fl(gh_t d_c).  -> (gI, gh) float32."""
  return _backward32(h, gs, vth, surrogate, None, np.asarray(dec, F32))


def param_sum(gh, factor, per_feature, skip_row=None):
  """sum gh * factor with every product formed in float64 (exact for float32 factors), and
  sum |gh * factor|: over (t, r, c) -> scalars (PLIF), or over (t, r) -> [C] (LIF).  skip_row
  leaves one row r out (what a dropped row would compute)."""
  term = np.asarray(gh, F64) * np.asarray(factor, F64)
  if skip_row is not None:
    term = np.delete(term, skip_row, axis=1)
  axes = (0, 1) if per_feature else None
  return term.sum(axis=axes), np.abs(term).sum(axis=axes)


# ---- backward scan, float64 with bounds ---------------------------------------------------------

def _backward64(h, gs, vth, surrogate, scale_i, keep):
  """tests.train_reference.lif_backward_ref64 with 1 / tau -> scale_i and keep given as the float32
  value the kernel holds (so it carries no error of its own: ek = 0).  Beside the values run the
  magnitudes Gh and the errors, u = 2^-24 per float32 rounding:
    Eh = |gs| sigma' ((1 + e)(1 + u)^2 - 1) + (1 - s) (Eu (1 + u) + Gu u)
    EI = (Eh (1 + u) + Gh u) scale_i          (scale_i None: gI is gh itself, EI = Eh)
    Eu = Eh keep + (Gh + Eh) keep u
  -> (gI, EI, gh, Eh), float64."""
  h, gs = np.asarray(h, F32), np.asarray(gs, F32)
  vth32 = F32(vth)
  keep = np.asarray(keep, F64)
  tiny = 4 * 2.0 ** -149
  gI, EI = np.empty(h.shape, F64), np.empty(h.shape, F64)
  ghs, Ehs = np.empty(h.shape, F64), np.empty(h.shape, F64)
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
    ghs[t], Ehs[t] = gh, Eh
    if scale_i is None:
      gI[t], EI[t] = gh, Eh
    else:
      gI[t] = gh * float(scale_i)
      EI[t] = (Eh * (1 + U) + Gh * U) * float(scale_i) + tiny
    gu = gh * keep
    Eu = Eh * keep + (Gh + Eh) * keep * U + tiny
    Gu = Gh * keep
  return gI, EI, ghs, Ehs


def plif_backward_ref64(h, gs, m, vth, surrogate):
  m = F32(m)
  return _backward64(h, gs, vth, surrogate, m, F32(1) - m)


def lif_backward_ref64(h, gs, dec, vth, surrogate):
  return _backward64(h, gs, vth, surrogate, None, np.asarray(dec, F32))


def param_sum_bound(gh64, Eh, factor, per_feature, n):
  """What a float64 accumulation, in any order, of the n exact products of float32 gh (within Eh
  of gh64) and float32 factors may differ from sum gh64 factor:
    gamma_n sum (|gh64| + Eh) |factor| + sum Eh |factor|,  gamma_n = n 2^-53 / (1 - n 2^-53)
  (n - 1 roundings of the additions; Higham, Accuracy and Stability, section 4.2).  With Eh = 0
  (a surrogate whose float32 gh is the reference's, bit for bit) it is gamma_n sum |term|."""
  f = np.abs(np.asarray(factor, F64))
  axes = (0, 1) if per_feature else None
  u53 = 2.0 ** -53
  g = n * u53 / (1.0 - n * u53)
  drift = (np.asarray(Eh, F64) * f).sum(axis=axes)
  return g * ((np.abs(gh64) * f).sum(axis=axes) + drift) + drift


# ---- the reference formulas in float64 torch, differentiated by autograd -------------------------

class _SavedSpike(torch.autograd.Function):
  """Forward: the spike the float32 forward saved.  Backward: g sigma'(saved float32 h - vth)."""

  @staticmethod
  def forward(ctx, x, s_saved, dsig):
    ctx.save_for_backward(dsig)
    return s_saved.clone()

  @staticmethod
  def backward(ctx, g):
    dsig, = ctx.saved_tensors
    return g * dsig, None, None


def _planted(expr, value):
  """expr's gradient with `value` as its value: the float32 forward's saved number."""
  return expr + (value - expr).detach()


def torch_scan_grads(kind, h, x, gs, par, vth, vr, surrogate):
  """spiking_learning.py:381-385 (PLIF) / :432-436 (LIF) over t in float64 torch with leaves x and
  par (m = sigmoid(tau), a scalar, or the decays [C]), the saved float32 potentials h planted as
  the values of the update (and, for PLIF, the float32 difference d as the value of
  s_in - (u - v_reset)), the spikes taken from them.  -> (gI, gpar) float64: the gradients of
  sum(s * gs) by torch.autograd -- no gradient passes through the `jnp.where` condition."""
  h32, x32 = np.asarray(h, F32), np.asarray(x, F32)
  T = h32.shape[0]
  t64 = lambda v: torch.from_numpy(np.asarray(v, F64).copy())       # noqa: E731
  hs = t64(h32)
  dsig = t64(sg64(surrogate, (h32 - F32(vth)).astype(F64)))
  ssv = t64(((h32 - F32(vth)) >= 0).astype(F64))
  d32 = t64(plif_difference(h32, x32, vth, vr))
  xs = t64(x32).requires_grad_(True)
  p = t64(np.asarray(par, F32)).requires_grad_(True)
  vr64, vth64 = float(F32(vr)), float(F32(vth))
  u = torch.zeros(h32.shape[1:], dtype=torch.float64)
  out = []
  for t in range(T):
    if kind == PLIF:
      u = u + _planted(xs[t] - (u - vr64), d32[t]) * p              # :381
    else:
      u = u * p + xs[t]                                             # :432
    u = _planted(u, hs[t])
    s = _SavedSpike.apply(u - vth64, ssv[t], dsig[t])               # :383 / :434
    u = torch.where(s > 0.5, torch.full_like(u, vr64), u)           # :385 / :436
    out.append(s)
  loss = (torch.stack(out) * t64(gs)).sum()
  gx, gp = torch.autograd.grad(loss, (xs, p))
  return gx.numpy(), gp.numpy()


# ---- the two-block ConvDenseSNN of tests/conv_train_reference.py with PLIF / LIF neurons ---------

def neuron_leaf_names(kind, nblocks):
  """The neuron modules' names in the parameter tree, block by block, the read-out last."""
  base = "parametric_leaky_IF" if kind == PLIF else "LIF"
  return ["%s_%d" % (base, i) for i in range(nblocks + 1)]


def conv_oracle_forward(kind, params, x_bt, mask, stats):
  """conv_train_reference.oracle_forward (quantised, integer path) with the block's PLIF / LIF
  neuron, its raw `tau` read from `params`: the float32 training forward by the oracle, BatchNorm
  on the given per-step statistics {i: (mean, var) [T, C]}."""
  x = np.swapaxes(np.asarray(x_bt, F32), 0, 1)
  out = {}
  n = sum(1 for k in params if k.startswith("QuantConv_"))
  names = neuron_leaf_names(kind, n)
  for i in range(n):
    qw = cr.qweight_of(oracle, params["QuantConv_%d" % i], cr.BITS, True)
    bn = params["BatchNorm_%d" % i]
    cur = np.stack([oracle.quant_conv(x[t], qw, None, ((1, 1), (1, 1)), mode="int") for t in range(x.shape[0])])
    mean, var = stats[i]
    y = np.stack([oracle.batchnorm_eval(cur[t], mean[t], var[t], bn["scale"], bn["bias"], cr.EPS)
                  for t in range(cur.shape[0])])
    h, s = neuron_save_ref(kind, y, params[names[i]]["tau"], cr.VTH, cr.VR)
    out.update({"h%d" % i: h, "s%d" % i: s})
    x = oracle.max_pool_2x2(s)
  flat = oracle.flatten_channel_major(x) * np.asarray(mask, F32)
  cur = oracle.quant_dense(flat, cr.qweight_of(oracle, params["QuantDense_0"], cr.BITS, True), "int")
  h, s = neuron_save_ref(kind, cur, params[names[n]]["tau"], cr.VTH, cr.VR)
  out.update(hd=h, sd=s, logits=s.astype(F64).mean(0).reshape(s.shape[1], -1, 10).mean(-1))
  return out


class TorchConvDenseSNN64Neuron(cr.TorchConvDenseSNN64):
  """TorchConvDenseSNN64 whose scans are spiking_learning.py:381-385 (PLIF) or :432-436 (LIF) with
  the block's `tau` a float64 leaf (sigmoid in float64), replaying the saved float32 spikes as the
  base class does.  grads() lists the `tau` leaves as (module name, "tau")."""

  def __init__(self, kind, params, surrogate="atan"):
    names = neuron_leaf_names(kind, sum(1 for k in params if k.startswith("QuantConv_")))
    super().__init__({k: v for k, v in params.items() if k not in names}, surrogate)
    self.kind, self.names = kind, names
    for name in names:
      t = torch.from_numpy(np.asarray(params[name]["tau"], F64).copy()).requires_grad_(True)
      self.leaf[name] = {"tau": t}
    self._vth, self._vr = float(F32(cr.VTH)), float(F32(cr.VR))

  def forward(self, x_bt, mask, saved):
    self._block = 0
    return super().forward(x_bt, mask, saved)

  def _scan(self, cur, h_saved, s_saved):
    k = torch.sigmoid(self.leaf[self.names[self._block]]["tau"])
    self._block += 1
    h32 = np.asarray(h_saved, F32)
    dsig = torch.from_numpy(sg64(self.surrogate, (h32 - F32(self._vth)).astype(F64)))
    s_sv = torch.from_numpy(np.asarray(s_saved, F64).copy())
    u = torch.zeros_like(cur[0])
    out = []
    for t in range(cur.shape[0]):
      if self.kind == PLIF:
        h = u + (cur[t] - (u - self._vr)) * k                        # :381
      else:
        h = u * k + cur[t]                                           # :432
      self.h_gap = max(self.h_gap, float((h.detach() - torch.from_numpy(h32[t].astype(F64))).abs().max()))
      s = _SavedSpike.apply(h - self._vth, s_sv[t], dsig[t])         # :383 / :434
      u = torch.where(s > 0.5, torch.full_like(h, self._vr), h)      # :385 / :436
      out.append(s)
    return torch.stack(out)
