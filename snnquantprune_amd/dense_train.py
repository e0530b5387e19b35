"""Training forward and surrogate-gradient backward of DenseSNN (configs C1 / C2).

jax.grad of examples/tcja/models.py:191-255 in train mode, offline, stated as two
torch.autograd.Functions, one per dense block:

  block 1   x0 = x * M0 (dropout, not rescaled) -> QuantDense -> multi_step_LIF -> s1
  block 2   x1 = s1 * M1 -> QuantDense -> multi_step_LIF -> s2 -> vote -> logits

Forward: the block's currents come from the eval connection kernels (the same launch and
arithmetic as SpikingBlock, so the spikes are the eval spikes), then one scan writes the
spikes and the pre-reset potential h (ops.lif_forward_save).  Backward (csrc/train_dense.hip):
the BPTT scan (ops.lif_backward, the vote fused into block 2's), the weight gradient
x^T gI and, for block 2, the input gradient gI Wq^T with * M1 in the epilogue.

The weight transforms (DuQ, prune; quant.py:428-491) are weight-sized: their VJPs are torch ops
on the device (weight_transform_grads).
"""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L
from . import ops
from . import packing

SURROGATES = {
    "fast_sigmoid": L.SURR_FAST_SIGMOID,
    "atan": L.SURR_ATAN,
    "slayer": L.SURR_SLAYER,
    "smooth_step": L.SURR_SMOOTH_STEP,
    "piecewise_linear": L.SURR_PIECEWISE_LINEAR,
}


def surrogate_derivative(name: str, x: torch.Tensor) -> torch.Tensor:
  """sigma'(x) of the spike functions' custom VJPs (spiking_learning.py:139-241), as torch ops."""
  if name == "fast_sigmoid":                   # :151-156
    return 1.0 / (10.0 * x.abs() + 1.0) ** 2
  if name == "atan":                           # :226-233, alpha = 2
    return 1.0 / (1.0 + (torch.pi * x) ** 2)
  if name == "slayer":                         # :170-174
    return torch.exp(-5.0 * x.abs())
  if name == "smooth_step":                    # :188-192
    return ((x < 0.5) & (x >= -0.5)).to(x.dtype)
  if name == "piecewise_linear":               # :206-211
    return torch.relu(1.0 - 2.0 * x.abs())
  raise NotImplementedError("no surrogate gradient for spike function %r" % (name,))


def surrogate_of(neuron_module) -> int:
  """SURR_* of a multi_step_LIF module's spike_fn; anything else is refused."""
  from .spiking_learning import multi_step_LIF
  if type(neuron_module) is not multi_step_LIF:
    raise NotImplementedError("training supports the multi_step_LIF neuron only, not %s"
                              % type(neuron_module).__name__)
  name = getattr(neuron_module.spike_fn, "__name__", None)
  if name not in SURROGATES:
    raise NotImplementedError("no surrogate gradient for spike function %r" % (name,))
  return SURROGATES[name]


# ---------------------------------------------------------------------------
# weight transforms: prune(DuQ(kernel)), flax_qdense.py:74-85
# ---------------------------------------------------------------------------


def weight_transform_grads(g, kernel, a=None, c=None, mask=None, levels=None):
  """VJP of kernel_fwd = prune(DuQ(kernel)) for the upstream gradient g of kernel_fwd.

  prune (quant.py:472-491): g * mask reaches DuQ's output; the mask gets zero (grad_zero).
  DuQ (quant.py:428-469), y = c * R(hard_tanh(W / a)), R straight-through with factor 1
  (DuQ_round_quant's VJP returns g, :445-446):  gc = sum g R(.),  gW = g c / a and
  ga = -sum g c W / a^2 where |W / a| <= 1 (jax.nn.hard_tanh's derivative is 1 there, ends
  included).  a == -1 (pass-through, :469) or no quantiser (levels None): gW = g, ga = gc = 0.
  Returns (gW, ga, gc, gmask), None for an absent parameter."""
  gm = None if mask is None else torch.zeros_like(mask)
  if mask is not None:
    g = g * mask.to(g.dtype)
  ga = None if a is None else torch.zeros_like(a)
  gc = None if c is None else torch.zeros_like(c)
  if levels is None or a is None or float(a.reshape(-1)[0]) == -1.0:
    return g, ga, gc, gm
  av, cv = a.reshape(()), c.reshape(())
  x = kernel / av
  inside = x.abs() <= 1
  r = torch.round(torch.clamp(x, -1.0, 1.0) * levels) / levels
  gw = torch.where(inside, g * cv / av, torch.zeros_like(g))
  # the two scalar sums run over every weight and cancel heavily: accumulated in float64
  g64, a64, c64 = g.to(torch.float64), av.to(torch.float64), cv.to(torch.float64)
  gc = (g64 * r.to(torch.float64)).sum().to(c.dtype).reshape(c.shape)
  ga = (-torch.where(inside, g64 * c64 * kernel.to(torch.float64) / (a64 * a64),
                     torch.zeros_like(g64)).sum()).to(a.dtype).reshape(a.shape)
  return gw, ga, gc, gm


class _WeightTransform(torch.autograd.Function):
  """kernel, a, c, mask -> kernel_fwd.  The value is the one the forward kernels use (packed by
  PackedKernel.float_weight); the backward is weight_transform_grads."""

  @staticmethod
  def forward(ctx, kernel, a, c, mask, value, levels):
    ctx.save_for_backward(kernel, a, c, mask)
    ctx.levels = levels
    return value.clone()

  @staticmethod
  def backward(ctx, g):
    kernel, a, c, mask = ctx.saved_tensors
    gw, ga, gc, gm = weight_transform_grads(g, kernel, a, c, mask, ctx.levels)
    return gw, ga, gc, gm, None, None


def transformed_kernel(leaf: dict, pk: packing.PackedKernel):
  """kernel_fwd of one QuantDense leaf, attached to autograd through its parameters."""
  kernel = leaf["kernel"]
  duq = leaf.get("DuQ_0", {})
  a, c = duq.get("a"), duq.get("c")
  mask = leaf.get("prune_0", {}).get("mask")
  d = pk.desc
  levels = None if d is None else float(d.L)
  with torch.no_grad():
    value = pk.float_weight().w.view_as(kernel)
  return _WeightTransform.apply(kernel, a, c, mask, value, levels)


# ---------------------------------------------------------------------------
# the two blocks
# ---------------------------------------------------------------------------


def _currents(x_tm: torch.Tensor, pk: packing.PackedKernel, N: int, real: bool = False) -> torch.Tensor:
  """x [T, B, K] (uint8, float32 or PackedSpikes) -> float32 currents [T, B, N] on the eval
  connection kernels: integer codes for integer-valued rows, the float32 kernel otherwise
  (`real`: rows real-valued by construction -- the float32 kernel without looking at them)."""
  T, B = x_tm.shape[0], x_tm.shape[1]
  K = x_tm.shape[-1]
  w = None if real else pk.int_weight()
  if w is not None and isinstance(x_tm, torch.Tensor) and x_tm.dtype == torch.float32:
    if bool(((x_tm == torch.round(x_tm)) & (x_tm >= 0) & (x_tm <= 255)).all()):
      x_tm = x_tm.to(torch.uint8)
    else:
      w = None
  if w is None:
    w = pk.float_weight()
    if isinstance(x_tm, ops.PackedSpikes):
      x_tm = x_tm.to_dense().to(torch.float32)
  geom = ops.ConvGeom(1, 1, K, N, 1, 1)
  if isinstance(x_tm, ops.PackedSpikes):
    x4 = x_tm.reshape_leading(T * B, 1, 1)
  else:
    x4 = x_tm.contiguous().reshape(T * B, 1, 1, K)
  return ops.conv_forward(x4, geom, w).reshape(T, B, N)


class DenseBlock1(torch.autograd.Function):
  """x0 [T, B, K] (dropout applied, no gradient) -> spikes s1 float32 [T, B, N].  Gradient to the
  transformed kernel wq [K, N] only (the model's input needs none)."""

  @staticmethod
  def forward(ctx, wq, x0, pk, nrn, surrogate):
    T, B, K = x0.shape
    N = wq.shape[1]
    cur = _currents(x0, pk, N)
    h, s = ops.lif_forward_save(cur, nrn)
    ctx.save_for_backward(x0, h)
    ctx.nrn, ctx.surrogate = nrn, surrogate
    ctx.mark_non_differentiable(h)
    return s, h

  @staticmethod
  def backward(ctx, gs, _gh):
    x0, h = ctx.saved_tensors
    T, B, K = x0.shape
    N = h.shape[-1]
    gI = ops.lif_backward(h, ctx.nrn, ctx.surrogate, gs=gs)
    gw = ops.dense_weight_grad(x0.reshape(T * B, K).to(torch.float32), gI.reshape(T * B, N))
    return gw, None, None, None, None


class DenseBlock2(torch.autograd.Function):
  """s1 [T, B, K], dropout mask M1 [T, B, K] -> (logits [B, N // group], s2, h2).  Gradients to
  s1 (through * M1, fused into the input-gradient kernel) and to the transformed kernel wq.

  group None: a hidden block -- no vote; -> (s2, None, h2), and the spikes' gradient drives the
  scan.  real_input: s1 holds real-valued rows (CextNet's dense1 behind the second gate): they are
  not bit-packed and the currents come from the float32 connection."""

  @classmethod
  def apply(cls, s1, wq, m1, pk, nrn, surrogate, group, real_input=False):
    return super().apply(s1, wq, m1, pk, nrn, surrogate, group, real_input)

  @staticmethod
  def forward(ctx, s1, wq, m1, pk, nrn, surrogate, group, real_input):
    T, B, K = s1.shape
    N = wq.shape[1]
    x1 = s1 * m1 if m1 is not None else s1
    if real_input:
      cur = _currents(x1.contiguous(), pk, N, real=True)
    else:
      xin = ops.pack_bits(x1.contiguous()) if pk.int_weight() is not None else x1
      cur = _currents(xin, pk, N)
    h, s = ops.lif_forward_save(cur, nrn)
    ctx.save_for_backward(h, wq, m1)
    ctx.x1 = x1
    ctx.nrn, ctx.surrogate, ctx.group = nrn, surrogate, group
    if group is None:
      ctx.mark_non_differentiable(h)
      return s, None, h
    logits = ops.vote(s, group)
    ctx.mark_non_differentiable(s, h)
    return logits, s, h

  @staticmethod
  def backward(ctx, glogits, _gs, _gh):
    h, wq, m1 = ctx.saved_tensors
    x1 = ctx.x1
    T, B, K = x1.shape
    N = h.shape[-1]
    if ctx.group is None:
      gI = ops.lif_backward(h, ctx.nrn, ctx.surrogate, gs=glogits.contiguous())
    else:
      gI = ops.lif_backward(h, ctx.nrn, ctx.surrogate, glogits=glogits, group=ctx.group)
    gI2 = gI.reshape(T * B, N)
    gw = ops.dense_weight_grad(x1.reshape(T * B, K), gI2)
    gs1 = None
    if ctx.needs_input_grad[0]:
      gs1 = ops.dense_input_grad(gI2, wq.detach(), None if m1 is None else m1.reshape(T * B, K))
      gs1 = gs1.reshape(T, B, K)
    return gs1, gw, None, None, None, None, None, None


def dropout_mask(shape, keep: float, generator: torch.Generator, device) -> torch.Tensor:
  """jax.random.bernoulli(p=keep, shape) as float32 0/1 (uniform < keep), not rescaled."""
  u = torch.rand(tuple(shape), generator=generator, device=device, dtype=torch.float32)
  return (u < float(keep)).to(torch.float32)


def generator_of(rng, device) -> torch.Generator:
  if isinstance(rng, torch.Generator):
    return rng
  g = torch.Generator(device=device)
  g.manual_seed(int(rng))
  return g


def apply_input_mask(x: torch.Tensor, m0: torch.Tensor) -> torch.Tensor:
  """x * M0 in the input's own dtype (uint8 counts stay counts)."""
  if x.dtype == torch.uint8:
    return x * m0.to(torch.uint8)
  return x * m0


def input_time_major(x0: torch.Tensor) -> torch.Tensor:
  return x0.transpose(0, 1).contiguous()

