"""Training forward and surrogate-gradient backward of DenseSNN (configs C1 / C2).

jax.grad of examples/tcja/models.py:191-255 in train mode, offline, stated as one
torch.autograd.Function (DenseBlock) applied once per dense block:

  block 1   x0 = x * M0 (dropout, not rescaled) -> QuantDense -> multi_step_LIF -> s1
  block 2   x1 = s1 * M1 -> QuantDense -> multi_step_LIF -> s2 -> vote -> logits

Forward: the block's currents come from the eval connection kernels (the same launch and
arithmetic as SpikingBlock, so the spikes are the eval spikes), then one scan writes the
spikes and the pre-reset potential h (ops.lif_forward_save).  Backward (csrc/train_dense.hip):
the BPTT scan (ops.lif_backward, the vote fused into block 2's), the weight gradient
x^T gI and, for a block behind another, the input gradient gI Wq^T with * M1 in the epilogue.

The weight transforms (DuQ, prune; quant.py:428-491) are weight-sized: their VJPs are torch ops
on the device (weight_transform_grads).
"""

from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L
from . import ops
from . import packing
from .conv_train import (conv_currents, neuron_param_grad, saved_membrane, scan_backward,  # noqa: F401
                         scan_forward)

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


def neuron_train_form(neuron_module, cfg):
  """(SURR_*, kind) of a block's neuron in training: what the training forwards ask.

  Without config.learn_neuron_params this is surrogate_of -- multi_step_LIF or a refusal -- and
  the kind is NEURON_MULTI_STEP_LIF.  With it, parametric_leaky_IF and LIF are taken too
  (NEURON_PARAMETRIC_LEAKY_IF / NEURON_LIF): their scans are ops.neuron_forward_save and
  ops.neuron_backward, and the block hands the `tau` leaf its gradient (neuron_param_grad)."""
  from .spiking_learning import LIF, parametric_leaky_IF
  kinds = {parametric_leaky_IF: L.NEURON_PARAMETRIC_LEAKY_IF, LIF: L.NEURON_LIF}
  learn = cfg is not None and "learn_neuron_params" in cfg and bool(cfg["learn_neuron_params"])
  if not learn or type(neuron_module) not in kinds:
    return surrogate_of(neuron_module), L.NEURON_MULTI_STEP_LIF
  name = getattr(neuron_module.spike_fn, "__name__", None)
  if name not in SURROGATES:
    raise NotImplementedError("no surrogate gradient for spike function %r" % (name,))
  return SURROGATES[name], kinds[type(neuron_module)]


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
# the block
# ---------------------------------------------------------------------------


def _currents(x, pk: packing.PackedKernel, N: int, real: bool) -> torch.Tensor:
  """x [T, B, K] (uint8, float32 or PackedSpikes) -> float32 currents [T, B, N]: the 1x1 case of
  conv_train.conv_currents, on the plain codes and with uint8 rows handed over as they are."""
  T, B, K = x.shape
  if isinstance(x, ops.PackedSpikes):
    x4 = x.reshape_leading(T * B, 1, 1)
  else:
    x4 = x.contiguous().reshape(T * B, 1, 1, K)
  cur = conv_currents(x4, pk, ops.ConvGeom(1, 1, K, N, 1, 1), real, mfma=False, cast_uint8=False)
  return cur.reshape(T, B, N)


class DenseBlock(torch.autograd.Function):
  """x [T, B, K], dropout mask m [T, B, K] or None -> (logits [B, N // group], s, h) with the
  spikes s and the pre-reset potential h [T, B, N].  Gradients to x (through * m, fused into the
  input-gradient kernel) and to the transformed kernel wq [K, N].

  The input is one of three kinds, as conv_train.ConvBlock's: spikes of the block before
  (bit-packed when the layer has integer codes); `first`: as given, counts or spikes from
  outside -- the integer path if the values are integers, saved in its own dtype, no gradient to
  it; `real_input`: real-valued rows (CextNet's dense1 behind the second gate) -- not bit-packed,
  the float32 connection without looking at the values.

  group None: a hidden block -- no vote; -> (s, None, h), and the spikes' gradient drives the
  scan.

  tau: the neuron's parameter leaf when it is learnt (neuron_train_form: PLIF or LIF) -- a further
  input that receives its gradient.  PLIF's backward reads the scan's currents again, so the block
  keeps them ([T, B, N] float32 more than a multi_step_LIF or LIF block saves).

  u0 [B, N]: the membranes the scan starts from, a window of a recording -- a
  further input that receives dL/du0, and a fourth output u_T [B, N], differentiable: the gradient
  arriving at it enters the backward scan.  The block never writes into u0.  With the vote, the
  logits and their gradient are the window's own (T is the window's length)."""

  @classmethod
  def apply(cls, x, wq, m, pk, nrn, surrogate, group, first=False, real_input=False, tau=None,
            u0=None):
    return super().apply(x, wq, m, pk, nrn, surrogate, group, first, real_input, tau, u0)

  @staticmethod
  def forward(ctx, x, wq, m, pk, nrn, surrogate, group, first, real_input, tau, u0):
    x1 = x * m if m is not None else x
    if first or real_input or pk.int_weight() is None:
      xin = x1
    else:
      xin = ops.pack_bits(x1.contiguous())
    cur = _currents(xin, pk, wq.shape[1], real_input)
    if u0 is None:
      h, s = scan_forward(cur, nrn, tau)
      tail = ()
    else:
      if tuple(u0.shape) != tuple(cur.shape[1:]):
        raise ValueError("DenseBlock: u0 %s, the block's membranes are %s"
                         % (tuple(u0.shape), tuple(cur.shape[1:])))
      h, s, u_T = scan_forward(cur, nrn, tau, u0.detach())
      tail = (u_T,)
    if tau is None or nrn.kind != L.NEURON_PARAMETRIC_LEAKY_IF:
      cur = None
    ctx.save_for_backward(h, wq, m, x1, tau, cur, saved_membrane(u0, tau))
    ctx.nrn, ctx.surrogate, ctx.group, ctx.first = nrn, surrogate, group, first
    ctx.window = u0 is not None
    if group is None:
      ctx.mark_non_differentiable(h)
      return (s, None, h) + tail
    logits = ops.vote(s, group)
    ctx.mark_non_differentiable(s, h)
    return (logits, s, h) + tail

  @staticmethod
  def backward(ctx, gout, _gs, _gh, gu_T=None):
    h, wq, m, x1, tau, cur, u0 = ctx.saved_tensors
    T, B, K = x1.shape
    N = h.shape[-1]
    upstream = dict(gs=gout.contiguous()) if ctx.group is None else dict(glogits=gout, group=ctx.group)
    gu0 = None
    if ctx.window:
      gI, gtau, gu0 = scan_backward(h, cur, ctx.nrn, ctx.surrogate, tau,
                                    state=(u0, gu_T, ctx.needs_input_grad[10]), **upstream)
    else:
      gI, gtau = scan_backward(h, cur, ctx.nrn, ctx.surrogate, tau, **upstream)
    gI2 = gI.reshape(T * B, N)
    gw = ops.dense_weight_grad(x1.reshape(T * B, K).to(torch.float32), gI2)
    gx = None
    if not ctx.first and ctx.needs_input_grad[0]:
      gx = ops.dense_input_grad(gI2, wq.detach(), None if m is None else m.reshape(T * B, K))
      gx = gx.reshape(T, B, K)
    return gx, gw, None, None, None, None, None, None, None, gtau, gu0


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

