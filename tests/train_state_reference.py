"""Plain references for training over windows of a recording; no GPU.  Thin
extensions of tests/train_reference.py, tests/neuron_train_reference.py and
tests/conv_train_reference.py: the same scans and recurrences from a membrane u0 to u_T, and from
the gradient arriving at u_T to the one of u0.

  save_ref                 float32 (h, s, u_T) of a scan from u0, stepping the oracle's neuron
  carried_state            u_{t-1} for every t with u_{-1} = u0
  backward_ref32           the float32 recurrences with gu_T -> (gI, gh, gu0)
  param_factor             the second factor of the PLIF / LIF parameter sum, u_{-1} = u0
  windows                  [(t0, t1)] of a split of T
  DenseSNN64State, ConvDenseSNN64State, ConvDenseSNN64NeuronState
                           the float64 models whose blocks start from constant membranes

Neuron kinds: ("msl", tau) multi_step_LIF; ("plif", raw tau (1,)); ("lif", raw tau [C]).
"""
import numpy as np
import torch

from oracle import snn_oracle as oracle
from tests import conv_train_reference as cr
from tests import neuron_train_reference as nr
from tests import train_reference as tr

F32, F64 = np.float32, np.float64
MSL, PLIF, LIF = "msl", nr.PLIF, nr.LIF


def windows(T, split):
  """[(t0, t1)] of the windows of lengths `split`, which add up to T."""
  assert sum(split) == T
  edges = np.concatenate([[0], np.cumsum(split)])
  return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


# ---- forward --------------------------------------------------------------------------------------

def save_ref(kind, cur, par, vth=1.0, vr=0.0, u0=None):
  """float32 currents [T, ...] -> (h, s, u_T) from the membrane u0 (None: zeros), stepping the
  oracle's neuron; h is the oracle's update before its reset (tr.lif_save_ref / nr.neuron_save_ref
  with u0 in place of their zero state).  par: tau (msl) or the raw parameter (plif, lif)."""
  cur = np.asarray(cur, F32)
  u = np.zeros(cur.shape[1:], F32) if u0 is None else np.asarray(u0, F32).reshape(cur.shape[1:]).copy()
  hs, ss = np.empty_like(cur), np.empty_like(cur)
  if kind != MSL:
    k = oracle.sigmoid_f32(np.asarray(par).reshape(-1)[0] if kind == PLIF else par)
  for t in range(cur.shape[0]):
    if kind == MSL:
      hs[t] = (u + (cur[t] - (u - F32(vr))) / F32(par)).astype(F32)
      u, s = oracle.multi_step_lif(u, cur[t], tau=par, v_threshold=vth, v_reset=vr)
    elif kind == PLIF:
      hs[t] = (u + (cur[t] - (u - F32(vr))) * k).astype(F32)
      u, s = oracle.parametric_leaky_if(u, cur[t], par, v_threshold=vth, v_reset=vr)
    else:
      hs[t] = (u * k + cur[t]).astype(F32)
      u, s = oracle.lif(u, cur[t], par, v_threshold=vth, v_reset=vr)
    ss[t] = s
  return hs, ss, np.asarray(u, F32)


def last_state(h, vth, vr, u0=None):
  """u_T from the saved potentials: s_{T-1} ? vr : h_{T-1}; u0 (None: zeros) when there is no step."""
  h = np.asarray(h, F32)
  if h.shape[0] == 0:
    return np.zeros(h.shape[1:], F32) if u0 is None else np.asarray(u0, F32)
  return np.where((h[-1] - F32(vth)) >= 0, F32(vr), h[-1]).astype(F32)


def carried_state(h, vth, vr, u0=None):
  """nr.carried_state with u0 in place of its leading zero."""
  u = nr.carried_state(h, vth, vr)
  if u0 is not None and u.shape[0]:
    u[0] = np.asarray(u0, F32).reshape(u.shape[1:])
  return u


# ---- backward -------------------------------------------------------------------------------------

def scales(kind, par):
  """(what gI is of gh, what gu keeps of gh) as float32; None: gI is gh.  par: tau (msl), float32 m
  (plif) or the float32 decays [C] (lif)."""
  one = F32(1)
  if kind == MSL:
    return ("div", F32(par)), one - one / F32(par)
  if kind == PLIF:
    return ("mul", F32(par)), one - F32(par)
  return None, np.asarray(par, F32)


def backward_ref32(kind, h, gs, par, vth, surrogate, gu_T=None):
  """tr.lif_backward_ref32 / nr._backward32 from gu_T (None: zeros) -> (gI, gh, gu0) float32:
    gh = gs sigma'(h - vth) + gu (1 - s);  gI = gh / tau | gh m | gh;  gu = gh keep
  Every operation rounds once; gu0 is the recurrence's last gu (gu_T itself without a step)."""
  h, gs = np.asarray(h, F32), np.asarray(gs, F32)
  vth, one = F32(vth), F32(1)
  scale, keep = scales(kind, par)
  gI, ghs = np.empty_like(h), np.empty_like(h)
  gu = np.zeros(h.shape[1:], F32) if gu_T is None else np.asarray(gu_T, F32).reshape(h.shape[1:]).copy()
  for t in range(h.shape[0] - 1, -1, -1):
    x = h[t] - vth
    s = (x >= 0).astype(F32)
    gh = gs[t] * tr.sg32(surrogate, x) + gu * (one - s)
    ghs[t] = gh
    gI[t] = gh if scale is None else (gh / scale[1] if scale[0] == "div" else gh * scale[1])
    gu = (gh * keep).astype(F32)
  return gI, ghs, gu


def param_factor(kind, h, x, vth, vr, u0=None):
  """The second factor of the parameter sum, float32 [T, R, C]: d_t = fl(x_t - fl(u_{t-1} - vr)) for
  PLIF, u_{t-1} for LIF, with u_{-1} = u0."""
  u = carried_state(h, vth, vr, u0)
  return (np.asarray(x, F32) - (u - F32(vr))).astype(F32) if kind == PLIF else u


def vote_upstream(gl, group, T, shape):
  """gs_t[r][c] = fl(glogits[r][c / group] / fl(group T)) for every t of a window of T steps."""
  g = (np.repeat(np.asarray(gl, F32), group, axis=1) / F32(group * T)).astype(F32)
  return np.broadcast_to(g[None], shape).copy()


# ---- the float64 models from constant membranes ----------------------------------------------------

def _t64(v):
  return torch.from_numpy(np.asarray(v, F64).copy())


class DenseSNN64State(tr.TorchDenseSNN64):
  """TorchDenseSNN64 whose two blocks start from the constant membranes u0s = [u0 [B, hidden],
  u0 [B, out]] (truncated BPTT: no gradient reaches them)."""

  def __init__(self, params, tau, vth, vr, surrogate, u0s, **kw):
    super().__init__(params, tau, vth, vr, surrogate, **kw)
    self.u0s, self._k = [_t64(u) for u in u0s], 0

  def forward(self, *a):
    self._k = 0
    return super().forward(*a)

  def _block(self, x, wq, h_saved, s_saved):
    u = self.u0s[self._k]
    self._k += 1
    T = x.shape[0]
    h32 = np.asarray(h_saved, F32)
    dsig = torch.from_numpy(tr.sg64(self.surrogate, (h32 - self.vth32).astype(F64)))
    s_sv = _t64(s_saved)
    out = []
    for t in range(T):
      h = u + (x[t] @ wq - (u - self.vr)) / self.tau                  # :410
      s = tr._SavedSpike.apply(h - self.vth, s_sv[t], dsig[t])        # :412
      u = torch.where(s.bool(), torch.full_like(h, self.vr), h)       # :414
      out.append(s)
    return torch.stack(out)


class ConvDenseSNN64State(cr.TorchConvDenseSNN64):
  """TorchConvDenseSNN64 whose scans start from the constant membranes u0s (block order, the
  read-out last; a conv block's [B, H, W, C])."""

  def __init__(self, params, u0s, **kw):
    super().__init__(params, **kw)
    self.u0s, self._k = [_t64(u) for u in u0s], 0

  def forward(self, x_bt, mask, saved):
    self._k = 0
    return super().forward(x_bt, mask, saved)

  def _scan(self, cur, h_saved, s_saved):
    u = self.u0s[self._k].reshape(cur[0].shape)
    self._k += 1
    h32 = np.asarray(h_saved, F32)
    dsig = torch.from_numpy(tr.sg64(self.surrogate, (h32 - F32(cr.VTH)).astype(F64)))
    s_sv = _t64(s_saved)
    out = []
    for t in range(cur.shape[0]):
      h = u + (cur[t] - (u - cr.VR)) / cr.TAU
      self.h_gap = max(self.h_gap, float((h.detach() - torch.from_numpy(h32[t].astype(F64))).abs().max()))
      s = tr._SavedSpike.apply(h - cr.VTH, s_sv[t], dsig[t])
      u = torch.where(s.bool(), torch.full_like(h, cr.VR), h)
      out.append(s)
    return torch.stack(out)


class ConvDenseSNN64NeuronState(nr.TorchConvDenseSNN64Neuron):
  """TorchConvDenseSNN64Neuron (PLIF / LIF, a `tau` leaf per block) from the constant membranes u0s."""

  def __init__(self, kind, params, u0s, **kw):
    super().__init__(kind, params, **kw)
    self.u0s = [_t64(u) for u in u0s]

  def _scan(self, cur, h_saved, s_saved):
    u = self.u0s[self._block].reshape(cur[0].shape)
    k = torch.sigmoid(self.leaf[self.names[self._block]]["tau"])
    self._block += 1
    h32 = np.asarray(h_saved, F32)
    dsig = torch.from_numpy(tr.sg64(self.surrogate, (h32 - F32(self._vth)).astype(F64)))
    s_sv = _t64(s_saved)
    out = []
    for t in range(cur.shape[0]):
      if self.kind == PLIF:
        h = u + (cur[t] - (u - self._vr)) * k                          # :381
      else:
        h = u * k + cur[t]                                             # :432
      self.h_gap = max(self.h_gap, float((h.detach() - torch.from_numpy(h32[t].astype(F64))).abs().max()))
      s = nr._SavedSpike.apply(h - self._vth, s_sv[t], dsig[t])        # :383 / :434
      u = torch.where(s > 0.5, torch.full_like(h, self._vr), h)        # :385 / :436
      out.append(s)
    return torch.stack(out)
