"""Training forward and backward of one gated stage of CextNet, as one torch.autograd.Function:

  m = mean_{H,W}(x_seq)                       [T, B, C]       examples/tcja/models.py:42
  a = conv_t(m as [B, C, T]),  b = conv_c(m as [B, T, C])     :52-93, 1-D QuantConvs, k = 4, SAME
  gate = sigmoid(b * a)                       [T, B, C]       :95
  p = maxpool2x2(x_seq * gate)                                :97, :184-187

Forward: as eval computes it (models.CextNet, the TCJA closure) -- ops.spatial_mean, the two
currents from ops.conv_forward on the float32 connection (the channel means are real-valued),
ops.sigmoid_gate, then the pool first and ops.apply_gate on the pooled raster: the gate is >= 0
and constant over a window and rounding is monotone, so max_i fl(x_i g) == fl((max_i x_i) g).

Backward (csrc/train_gate.hip): ggate from the routed windows, the sigmoid and the product in
torch ops on [T, B, C] arrays, the two 1-D convs' gradient products on the kernels of
csrc/train_conv.hip (H = 1, KH = 1, padding (1, 2)), and one kernel that routes gp * gate to the
first maximum of each window and adds the gradient through the spatial mean.
"""

from __future__ import annotations

import torch

from . import ops


def gate_currents(m: torch.Tensor, pk_t, pk_c, geom_t: ops.ConvGeom, geom_c: ops.ConvGeom):
  """m [T, B, C] -> (a, b) float32 [T, B, C]: conv_t over the channel axis with the T steps as
  features, conv_c over the time axis with the C channels as features (eval's TCJA closure)."""
  T, B, C = m.shape
  x = m.transpose(0, 1).contiguous()                      # [B, T, C]
  x_c = x.transpose(1, 2).contiguous()                    # [B, C, T]
  a = ops.conv_forward(x_c.reshape(B, 1, C, T), geom_t, pk_t.float_weight()).reshape(B, C, T)
  b = ops.conv_forward(x.reshape(B, 1, T, C), geom_c, pk_c.float_weight()).reshape(B, T, C)
  return a.permute(2, 0, 1).contiguous(), b.transpose(0, 1).contiguous()


class TcjaGate(torch.autograd.Function):
  """x_seq [T, B, H, W, C] (the unpooled raster of the conv_t_i block), the transformed 1-D kernels
  wq_t [4, T, T] and wq_c [4, C, C] -> (p [T, B, H/2, W/2, C], gate [T, B, C] without gradient).
  Gradients to x_seq and to both kernels."""

  @staticmethod
  def forward(ctx, x_seq, wq_t, wq_c, pk_t, pk_c, geom_t, geom_c):
    x_seq = x_seq.contiguous()
    m = ops.spatial_mean(x_seq)
    a, b = gate_currents(m, pk_t, pk_c, geom_t, geom_c)
    gate = ops.sigmoid_gate(b, a)
    p = ops.apply_gate(ops.maxpool2x2(x_seq), gate)
    ctx.save_for_backward(x_seq, wq_t, wq_c, m, a, b, gate)
    ctx.geom_t, ctx.geom_c = geom_t, geom_c
    ctx.mark_non_differentiable(gate)
    return p, gate

  @staticmethod
  def backward(ctx, gp, _ggate):
    x_seq, wq_t, wq_c, m, a, b, gate = ctx.saved_tensors
    geom_t, geom_c = ctx.geom_t, ctx.geom_c
    T, B, H, W, C = x_seq.shape
    gp = gp.contiguous()
    ggate = ops.gate_pool_grad_gate(x_seq, gate, gp)      # [T, B, C]
    gz = ggate * (gate * (1.0 - gate))                    # z = a b
    ga = (gz * b).permute(1, 2, 0).contiguous().reshape(B, 1, C, T)      # like conv_t's output
    gb = (gz * a).transpose(0, 1).contiguous().reshape(B, 1, T, C)       # like conv_c's output
    x = m.transpose(0, 1).contiguous()                    # [B, T, C]
    x_c = x.transpose(1, 2).contiguous()                  # [B, C, T]
    gw_t = ops.conv_weight_grad(x_c.reshape(B, 1, C, T), ga, geom_t).reshape(wq_t.shape)
    gw_c = ops.conv_weight_grad(x.reshape(B, 1, T, C), gb, geom_c).reshape(wq_c.shape)
    gx = None
    if ctx.needs_input_grad[0]:
      gxc = ops.conv_input_grad(ga, wq_t.detach().reshape((1,) + tuple(wq_t.shape)), geom_t).reshape(B, C, T)
      gxx = ops.conv_input_grad(gb, wq_c.detach().reshape((1,) + tuple(wq_c.shape)), geom_c).reshape(B, T, C)
      gm = (gxx + gxc.transpose(1, 2)).transpose(0, 1).contiguous()     # [T, B, C]
      gx = ops.gate_pool_grad_input(x_seq, gate, gp, gm)
    return gx, gw_t, gw_c, None, None, None, None
