"""Plain references for training a conv block with rematerialisation (csrc/train_remat.hip,
conv_train.RematConvBlock); no GPU.

  bn_multiplier / bn_normalise   the float32 coefficient and the three roundings of the block's
                                 normalisation (conv_train.bn_multiplier, conv_train.bn_normalise)
  fused_ref                      the fused step: those three roundings, then the oracle's neuron step
                                 from u0 -> (h, s, u_T)
  pool_route_h                   the pool's gradient routing read from h by the forward's compare
  chunks                         [(t0, t1)] of T steps in chunks of W
  Block64                        one conv block in float64 torch (TorchConvDenseSNN64's pieces), its
                                 whole-run backward and the chunked one with chained gu0
"""
import numpy as np
import torch

from oracle import snn_oracle as oracle
from tests import conv_train_reference as cr
from tests import train_reference as tr

F32, F64 = np.float32, np.float64


def bn_multiplier(var, scale, eps):
  """fl(fl(1 / sqrt(fl(var + eps))) * scale), [T, C]."""
  r = (F32(1) / np.sqrt((np.asarray(var, F32) + F32(eps)).astype(F32)).astype(F32)).astype(F32)
  return (r * np.asarray(scale, F32)).astype(F32)


def bn_normalise(cur, mean, mul, bias):
  """cur [T, R, C], mean, mul [T, C], bias [C] -> fl(fl(fl(cur - mean) * mul) + bias)."""
  y = (np.asarray(cur, F32) - np.asarray(mean, F32)[:, None, :]).astype(F32)
  y = (y * np.asarray(mul, F32)[:, None, :]).astype(F32)
  return (y + np.asarray(bias, F32)).astype(F32)


def fused_ref(cur, mean, mul, bias, tau, vth=1.0, vr=0.0, u0=None):
  """The fused step, one step at a time: y_t by the three roundings, h_t the oracle's update before
  its reset, then oracle.multi_step_lif from the carried membrane -> (h, s, u_T) float32."""
  cur = np.asarray(cur, F32)
  mean, mul, bias = np.asarray(mean, F32), np.asarray(mul, F32), np.asarray(bias, F32)
  u = np.zeros(cur.shape[1:], F32) if u0 is None else np.asarray(u0, F32).reshape(cur.shape[1:]).copy()
  hs, ss = np.empty_like(cur), np.empty_like(cur)
  for t in range(cur.shape[0]):
    y = (cur[t] - mean[t]).astype(F32)
    y = (y * mul[t]).astype(F32)
    y = (y + bias).astype(F32)
    hs[t] = (u + (y - (u - F32(vr))) / F32(tau)).astype(F32)
    u, s = oracle.multi_step_lif(u, y, tau=tau, v_threshold=vth, v_reset=vr)
    ss[t] = s
  return hs, ss, np.asarray(u, F32)


def pool_route_h(h, vth, gp):
  """h [..., H, W, C], gp [..., H/2, W/2, C] -> gs like h: each gp element to the first position, in
  the order (0,0), (0,1), (1,0), (1,1), whose spike ((h - vth) >= 0) is the window's maximum -- the
  first that fired, or (0,0) where none did; zeros in a trailing odd row or column."""
  h, gp = np.asarray(h, F32), np.asarray(gp, F32)
  H, W = h.shape[-3:-1]
  PH, PW = H // 2, W // 2
  fired = (h - F32(vth)) >= 0
  gs = np.zeros(h.shape, F32)
  taken = np.zeros(gp.shape, bool)
  order = ((0, 0), (0, 1), (1, 0), (1, 1))
  for dh, dw in order:
    f = fired[..., dh:2 * PH:2, dw:2 * PW:2, :] & ~taken
    gs[..., dh:2 * PH:2, dw:2 * PW:2, :] = np.where(f, gp, F32(0))
    taken |= f
  gs[..., 0:2 * PH:2, 0:2 * PW:2, :] += np.where(taken, F32(0), gp)      # no spike: the first position
  return gs


def chunks(T, W):
  """[(t0, t1)]: 0..T in chunks of W, the last one ragged."""
  if W < 1:
    raise ValueError(W)
  return [(t0, min(t0 + W, T)) for t0 in range(0, T, W)]


# ---- one block in float64 ---------------------------------------------------------------------------

def _t64(v):
  return torch.from_numpy(np.asarray(v, F64).copy())


class Block64:
  """x [T, B, H, W, Cin] -> conv 3x3 (same), BatchNorm on each step's batch statistics,
  multi_step_LIF replaying saved spikes (train_reference._SavedSpike), the first-maximum 2x2 pool
  (conv_train_reference._FirstMaxPool): the pieces of TorchConvDenseSNN64, for one block, from a
  membrane u0 to u_T.  The saved h and spikes are those of its own float64 forward."""

  def __init__(self, x, wq, scale, bias, surrogate="atan"):
    self.x, self.wq, self.scale, self.bias = _t64(x), _t64(wq), _t64(scale), _t64(bias)
    self.surrogate = surrogate
    T = self.x.shape[0]
    with torch.no_grad():
      y = self._normalised(self.x, self.wq, self.scale, self.bias)
      u = torch.zeros_like(y[0])
      hs, self.starts = [], []
      for t in range(T):
        self.starts.append(u)
        h = u + (y[t] - (u - cr.VR)) / cr.TAU
        u = torch.where(h - cr.VTH >= 0, torch.full_like(h, cr.VR), h)
        hs.append(h)
    self.h32 = torch.stack(hs).numpy().astype(F32)
    self.s = ((self.h32 - F32(cr.VTH)) >= 0).astype(F64)

  @staticmethod
  def _normalised(x, wq, scale, bias):
    T, B, H, W, C = x.shape
    cur = torch.nn.functional.conv2d(x.reshape(T * B, H, W, C).permute(0, 3, 1, 2),
                                     wq.permute(3, 2, 0, 1), padding=1)
    cur = cur.permute(0, 2, 3, 1).reshape(T, B, H, W, -1)
    mean = cur.mean((1, 2, 3))
    var = (cur * cur).mean((1, 2, 3)) - mean * mean
    mul = torch.rsqrt(var + cr.EPS) * scale
    return (cur - mean[:, None, None, None]) * mul[:, None, None, None] + bias

  def run(self, t0, t1, x, wq, scale, bias, u):
    """Steps t0..t1 from the membrane u -> (pooled, u_T), differentiable in all five."""
    y = self._normalised(x, wq, scale, bias)
    dsig = torch.from_numpy(tr.sg64(self.surrogate, (self.h32[t0:t1] - F32(cr.VTH)).astype(F64)))
    s_sv = torch.from_numpy(self.s[t0:t1].copy())
    out = []
    for t in range(t1 - t0):
      h = u + (y[t] - (u - cr.VR)) / cr.TAU
      s = tr._SavedSpike.apply(h - cr.VTH, s_sv[t], dsig[t])
      u = torch.where(s.bool(), torch.full_like(h, cr.VR), h)
      out.append(s)
    return cr._FirstMaxPool.apply(torch.stack(out)), u

  def backward(self, gp, W=None, chain=True):
    """{"x", "wq", "scale", "bias"} float64 gradients of sum(pooled gp).  W None: one graph over the
    whole run.  Else chunk by chunk, last chunk first, each chunk a graph of its own from its
    starting membrane; `chain`: the chunk's gu0 enters the chunk before as the gradient of its u_T
    (False: dropped, the truncated gradient)."""
    T = self.x.shape[0]
    gp = _t64(gp)
    total = {"x": torch.zeros_like(self.x), "wq": 0.0, "scale": 0.0, "bias": 0.0}
    gu = None
    for t0, t1 in reversed(chunks(T, T if W is None else W)):
      leaves = [v.clone().requires_grad_(True) for v in
                (self.x[t0:t1], self.wq, self.scale, self.bias, self.starts[t0])]
      pooled, u_T = self.run(t0, t1, *leaves)
      outs, gouts = [pooled], [gp[t0:t1]]
      if gu is not None:
        outs.append(u_T)
        gouts.append(gu)
      g = torch.autograd.grad(outs, leaves, gouts, allow_unused=True)
      total["x"][t0:t1] = g[0]
      for name, part in zip(("wq", "scale", "bias"), g[1:4]):
        total[name] = total[name] + part
      gu = g[4] if chain else None
    return {k: v.numpy() for k, v in total.items()}
