"""Training forward and surrogate-gradient backward of the conv blocks of ConvDenseSNN (config C3)
and CextNet.

jax.grad of examples/tcja/models.py:101-147 in train mode, offline, stated as one
torch.autograd.Function per block:

  x -> QuantConv 3x3 -> BatchNorm (batch statistics) -> multi_step_LIF -> 2x2 max pool

Forward: the currents come from the eval connection kernels (ops.conv_forward; from block 1 on
the input is the bit-packed raster of the block before, so the integer path stays exact, and
the connection runs on the currents form of the bit-input MFMA conv, nn.set_train_conv_mfma), the
batch-statistics BatchNorm runs as torch tensor ops, one scan writes the spikes and the pre-reset
potential h (ops.lif_forward_save), and ops.maxpool2x2 pools.  Backward (csrc/train_conv.hip,
csrc/train_dense.hip): the pool's routing, the BPTT scan, BatchNorm's backward in torch ops, then
the two conv gradient products.

BatchNorm in train mode, per scan step t and per channel over (B, H, W) -- the reference's
SpikingBlock scans over time, so each step normalises with its own statistics:
  mean = mean(x),  var = mean(x^2) - mean^2  (the flax 0.4.0 form, biased)
  y = (x - mean) * (rsqrt(var + eps) * scale) + bias
The two means are accumulated in float64 and rounded to float32 once; given those float32
statistics, y is the arithmetic of the eval BatchNorm (each op rounded in float32).  The running
statistics move once per step, in t order: ra = momentum * ra + (1 - momentum) * new.
"""

from __future__ import annotations

import torch

from . import _lib as _L
from . import linen as _nn
from . import ops
from . import packing


def batch_stats(x: torch.Tensor):
  """x [T, N, C] float32 -> (mean, var) float32 [T, C]: float64 accumulation, one rounding."""
  x64 = x.to(torch.float64)
  mean = x64.mean(1)
  var = (x64 * x64).mean(1) - mean * mean
  return mean.to(torch.float32), var.to(torch.float32)


def bn_multiplier(var: torch.Tensor, scale: torch.Tensor, eps: float) -> torch.Tensor:
  """fl(fl(1 / sqrt(fl(var + eps))) * scale), the fold of the eval BatchNorm."""
  return (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32, device=var.device))) * scale


def bn_normalise(x, mean, mul, bias):
  """x [T, N, C], per-step coefficients [T, C] -> fl(fl(fl(x - mean) * mul) + bias)."""
  y = x - mean[:, None, :]
  y *= mul[:, None, :]
  y += bias if bias.ndim == 1 else bias[:, None, :]
  return y


def bn_backward(g, x, mean, var, scale, eps):
  """The VJP of y = (x - mean) * (r * scale) + bias with r = (var + eps)^-1/2 and the batch
  statistics functions of x.  g, x [T, N, C]; -> (gx [T, N, C], gscale [C], gbias [C]).
  The channel-sized reductions and coefficients are float64, the image-sized result float32."""
  N = x.shape[1]
  g64 = g.to(torch.float64)
  mean64, var64, scale64 = mean.to(torch.float64), var.to(torch.float64), scale.to(torch.float64)
  r = torch.rsqrt(var64 + eps)                                   # [T, C]
  sg = g64.sum(1)                                                # sum g
  sgx = (g64 * x).sum(1) - mean64 * sg                           # sum g (x - mean)
  gbias = sg.sum(0)
  gscale = (sgx * r).sum(0)
  gvar = sgx * scale64 * (-0.5) * r * r * r
  gmean = -(r * scale64) * sg - 2.0 * mean64 * gvar
  # gx = g m + (gmean + 2 gvar x) / N
  m = (r * scale64).to(torch.float32)
  c0 = (gmean / N).to(torch.float32)
  c1 = (2.0 * gvar / N).to(torch.float32)
  gx = g * m[:, None, :]
  gx += c0[:, None, :]
  gx.addcmul_(x, c1[:, None, :])
  return gx, gscale.to(scale.dtype), gbias.to(scale.dtype)


def running_update(old: torch.Tensor, new_t: torch.Tensor, momentum: float) -> torch.Tensor:
  """T steps of ra = momentum * ra + (1 - momentum) * new_t, float32, in t order."""
  m = torch.tensor(momentum, dtype=torch.float32, device=old.device)
  k = 1.0 - m
  ra = old.to(torch.float32)
  for t in range(new_t.shape[0]):
    ra = m * ra + k * new_t[t]
  return ra


def conv_currents(x, pk: packing.PackedKernel, geom: ops.ConvGeom, real: bool = False,
                  mfma: bool = True, cast_uint8: bool = True) -> torch.Tensor:
  """x [NB, H, W, Cin] (uint8, float32 or PackedSpikes) -> float32 [NB, OH, OW, Cout] on the eval
  connection kernels: integer codes for integer-valued inputs, the float32 kernel otherwise.
  `real`: the input is real-valued by construction (a gated raster) -- the float32 connection
  without looking at the values, as eval runs it under packing.integer_inputs(False).

  The connection of every training block, conv and dense (dense_train.DenseBlock: the 1x1 case).
  The two kinds of block differ in two launches, which the last two arguments state: the conv
  blocks may take the MFMA-tiled codes for a bit-packed raster (`mfma`, under
  nn.set_train_conv_mfma) and cast a uint8 input to float32 in front of the float32 connection
  (`cast_uint8`); the dense blocks do neither -- ops.conv_forward gets the plain codes, and the
  uint8 rows as they are."""
  w = None if real else pk.int_weight()
  if mfma and w is not None and isinstance(x, ops.PackedSpikes) and _nn.train_conv_mfma():
    # the bit-packed raster of the block before: the codes tiled for the MFMA currents kernel
    # (ops.conv_forward takes it where the shape allows, the direct-form launch otherwise)
    w = pk.int_weight_mfma((geom.Cout + 31) // 32 * 32) or w
  if w is not None and isinstance(x, torch.Tensor) and x.dtype == torch.float32:
    if bool(((x == torch.round(x)) & (x >= 0) & (x <= 255)).all()):
      x = x.to(torch.uint8)
    else:
      w = None
  if w is None:
    w = pk.float_weight()
    if isinstance(x, ops.PackedSpikes):
      x = x.to_dense().to(torch.float32)
    elif cast_uint8 and x.dtype != torch.float32:
      x = x.to(torch.float32)
  return ops.conv_forward(x, geom, w)


# ---- the scan of a training block, conv or dense ------------------------------------------------
# (here, beside conv_currents, and not in dense_train: dense_train imports this module for the
# connection, so what both kinds of block share lives on this side of that import)


def neuron_param_grad(gparam: torch.Tensor, tau: torch.Tensor) -> torch.Tensor:
  """The `tau` leaf's gradient from the scan's float64 sum: Gm m (1 - m) for PLIF's scalar,
  Gd_c d_c (1 - d_c) for LIF's decays, m / d = sigmoid(tau) in float64 on the device; in the
  leaf's dtype and shape."""
  sg = torch.sigmoid(tau.detach().to(torch.float64))
  return (gparam.reshape(tau.shape) * sg * (1.0 - sg)).to(tau.dtype)


def scan_forward(cur, nrn, tau, u0=None):
  """(h, s) of a training block's scan, conv or dense: the multi_step_LIF kernel, or with a `tau`
  leaf (dense_train.neuron_train_form) the PLIF / LIF one.  u0 (a window of a recording, DESIGN.md
  18): the membrane the scan starts from, shaped like one step -> (h, s, u_T)."""
  scan = ops.lif_forward_save if tau is None else ops.neuron_forward_save
  return scan(cur, nrn) if u0 is None else scan(cur, nrn, u0=u0, return_state=True)


def scan_backward(h, cur, nrn, surrogate, tau, state=None, **upstream):
  """(gI, gtau) of that scan; gtau None without a `tau` leaf.  cur: the currents the scan consumed
  (read for PLIF only).  upstream: gs=, or glogits= and group=.  state (u0, gu_T, want_gu0) of a
  window's scan: the block's own copy of the membrane it started from (read for PLIF and LIF only,
  else None), the gradient arriving at u_T or None -> (gI, gtau, gu0), gu0 None unless wanted."""
  if state is None:
    if tau is None:
      return ops.lif_backward(h, nrn, surrogate, **upstream), None
    gI, gparam = ops.neuron_backward(h, cur, nrn, surrogate, **upstream)
    return gI, neuron_param_grad(gparam, tau)
  u0, gu_T, want = state
  if tau is None:
    out = ops.lif_backward(h, nrn, surrogate, gu_T=gu_T, return_gu0=True, **upstream)
    return out[0], None, (out[1] if want else None)
  gI, gparam, gu0 = ops.neuron_backward(h, cur, nrn, surrogate, u0=u0, gu_T=gu_T, return_gu0=True,
                                        **upstream)
  return gI, neuron_param_grad(gparam, tau), (gu0 if want else None)


def saved_membrane(u0, tau):
  """What a window's block keeps of u0 for its backward: its own copy where the backward reads it
  (PLIF, LIF: u_{-1} of the parameter sums) -- the caller overwrites the state's buffer with u_T
  before the backward runs --, nothing for multi_step_LIF."""
  return None if u0 is None or tau is None else u0.detach().clone()


class ConvBlock(torch.autograd.Function):
  """x [T, B, H, W, Cin] -> pooled spikes float32 [T, B, OH/2, OW/2, C], and without gradient the
  unpooled h, s [T, B, OH, OW, C] and the per-step statistics mean, var [T, C].  Gradients to x
  (not for the first block: the frames need none), the transformed kernel wq (HWIO) and
  BatchNorm's scale and bias.

  pool = 1: no pool, the first output is the spike raster itself and its gradient arrives
  directly (the blocks in front of CextNet's TCJA gates).  real_input: x is a real-valued raster
  (what a gate leaves), not spikes: it is not bit-packed and the currents come from the float32
  connection on it.  wgrad_f64: the weight gradient's chain runs in float64
  (ops.conv_weight_grad_f64) -- CextNet's first block, whose 64 x 64 and larger count frames make
  the sum cancel further than a float32 chain resolves.

  tau: the neuron's parameter leaf when it is learnt (dense_train.neuron_train_form: PLIF or LIF)
  -- a further input that receives its gradient.  PLIF's backward reads the scan's input again:
  it is recomputed from the saved currents and statistics (scan_input), the forward's bits.

  u0 [B, OH, OW, C]: the membranes the scan starts from, a window of a recording --
  a further input that receives dL/du0, and a sixth output u_T [B, OH, OW, C], differentiable: the
  gradient arriving at it enters the backward scan.  The block never writes into u0."""

  @classmethod
  def apply(cls, x, wq, scale, bias, pk, geom, nrn, surrogate, eps, first, pool=2,
            real_input=False, wgrad_f64=False, tau=None, u0=None):
    if pool not in (1, 2):
      raise ValueError("ConvBlock: pool must be 1 or 2, got %r" % (pool,))
    return super().apply(x, wq, scale, bias, pk, geom, nrn, surrogate, eps, first, pool,
                         real_input, wgrad_f64, tau, u0)

  @staticmethod
  def scan_input(cur, mean, var, scale, bias, eps):
    """The normalised currents the scan consumes, from what the block saves: one sequence of
    float32 operations, so the backward's recomputation is the forward's tensor bit for bit."""
    return bn_normalise(cur.clone(), mean, bn_multiplier(var, scale, eps), bias)

  @staticmethod
  def forward(ctx, x, wq, scale, bias, pk, geom, nrn, surrogate, eps, first, pool, real_input,
              wgrad_f64, tau, u0):
    T, B = x.shape[0], x.shape[1]
    C = geom.Cout
    if first or real_input or pk.int_weight() is None:
      xin = x.reshape(T * B, geom.H, geom.W, geom.Cin)
    else:
      xin = ops.pack_bits(x.reshape(T * B, geom.H, geom.W, geom.Cin).contiguous())
    cur = conv_currents(xin, pk, geom, real=real_input)
    OH, OW = cur.shape[1], cur.shape[2]
    cur = cur.reshape(T, B * OH * OW, C)
    mean, var = batch_stats(cur)
    y = ConvBlock.scan_input(cur, mean, var, scale, bias, eps)
    u_T = None
    if u0 is None:
      h, s = scan_forward(y, nrn, tau)
    else:
      if tuple(u0.shape) != (B, OH, OW, C):
        raise ValueError("ConvBlock: u0 %s, the block's membranes are %s" % (tuple(u0.shape), (B, OH, OW, C)))
      h, s, u_T = scan_forward(y, nrn, tau, u0.detach().reshape(B * OH * OW, C))
      u_T = u_T.reshape(B, OH, OW, C)
    del y
    h = h.reshape(T, B, OH, OW, C)
    s = s.reshape(T, B, OH, OW, C)
    pooled = ops.maxpool2x2(s) if pool == 2 else s.clone()
    plif = tau is not None and nrn.kind == _L.NEURON_PARAMETRIC_LEAKY_IF
    ctx.save_for_backward(x, wq, scale, cur, mean, var, h, tau, bias.detach() if plif else None,
                          saved_membrane(u0, tau))
    ctx.geom, ctx.nrn, ctx.surrogate, ctx.eps, ctx.first = geom, nrn, surrogate, eps, first
    ctx.pool, ctx.wgrad_f64, ctx.window = pool, wgrad_f64, u0 is not None
    ctx.mark_non_differentiable(h, s, mean, var)
    return (pooled, h, s, mean, var) if u0 is None else (pooled, h, s, mean, var, u_T)

  @staticmethod
  def backward(ctx, gp, _gh, _gs, _gmean, _gvar, gu_T=None):
    x, wq, scale, cur, mean, var, h, tau, bias, u0 = ctx.saved_tensors
    geom, nrn = ctx.geom, ctx.nrn
    T, B, OH, OW, C = h.shape
    if ctx.pool == 2:
      s = ((h - nrn.v_threshold) >= 0).to(torch.float32)        # the forward's spikes
      gs = ops.maxpool2x2_backward(s, gp.contiguous())
      del s
    else:
      gs = gp.contiguous()
    y = None if bias is None else ConvBlock.scan_input(cur, mean, var, scale.detach(), bias, ctx.eps)
    gu0 = None
    if ctx.window:
      gy, gtau, gu0 = scan_backward(h.reshape(T, B * OH * OW, C), y, nrn, ctx.surrogate, tau,
                                    state=(u0, gu_T, ctx.needs_input_grad[14]),
                                    gs=gs.reshape(T, B * OH * OW, C))
      gu0 = None if gu0 is None else gu0.reshape(B, OH, OW, C)
    else:
      gy, gtau = scan_backward(h.reshape(T, B * OH * OW, C), y, nrn, ctx.surrogate, tau,
                               gs=gs.reshape(T, B * OH * OW, C))
    del gs, y
    gcur, gscale, gbias = bn_backward(gy, cur, mean, var, scale, ctx.eps)
    del gy
    gcur = gcur.reshape(T * B, OH, OW, C)
    x4 = x.reshape(T * B, geom.H, geom.W, geom.Cin).to(torch.float32)
    gw = ops.conv_weight_grad_f64(x4, gcur, geom) if ctx.wgrad_f64 else ops.conv_weight_grad(x4, gcur, geom)
    gx = None
    if not ctx.first and ctx.needs_input_grad[0]:
      gx = ops.conv_input_grad(gcur, wq.detach(), geom).reshape(x.shape)
    return gx, gw, gscale, gbias, None, None, None, None, None, None, None, None, None, gtau, gu0


# ---- the block with rematerialisation --------------------------------------------


def check_remat(W):
  """config.remat: the steps per chunk, an integer of at least 1."""
  if isinstance(W, bool) or not isinstance(W, int) or W < 1:
    raise ValueError("config.remat must be an integer of at least 1 (the steps per chunk), got %r" % (W,))
  return W


def remat_chunks(T: int, W: int):
  """[(t0, t1), ...]: the steps 0..T cut into chunks of W in order, the last one ragged; W >= T is
  one chunk, T == 0 none."""
  check_remat(W)
  return [(t0, min(t0 + W, T)) for t0 in range(0, T, W)]


def _accumulate(acc, part):
  """The chunks' reductions, added in the order the backward visits them."""
  return part if acc is None else acc + part


class RematConvBlock(torch.autograd.Function):
  """ConvBlock (pool 2, spike or frame input, float32 weight-gradient chain) that keeps neither
  its currents nor h: x [T, B, H, W, Cin] is walked in chunks of `chunk` steps, forward and
  backward, and the backward recomputes each chunk's currents and scan from what the block keeps
  -- its input (the bit-packed raster from block 1 on, the frames as given for block 0), the
  per-step statistics, the membrane at the start of every chunk and the parameters.  The chunks'
  scans are chained exactly: a chunk starts from the membrane the one before left, and its
  backward scan takes the gu0 of the chunk after as gu_T, so every element-sized tensor is
  ConvBlock's bit for bit; gw, gscale, gbias and the `tau` sums are each chunk's own reduction,
  added last chunk first.

  Outputs as ConvBlock's; h and s are the chunks' concatenated and only with want_h (the sown
  intermediates), else None."""

  @classmethod
  def apply(cls, x, wq, scale, bias, pk, geom, nrn, surrogate, eps, first, chunk, want_h=False,
            tau=None, u0=None):
    check_remat(chunk)
    return super().apply(x, wq, scale, bias, pk, geom, nrn, surrogate, eps, first, chunk, want_h,
                         tau, u0)

  @staticmethod
  def kept_input(x, pk, geom, first):
    """(what the block keeps of x [T, B, H, W, Cin], how a chunk of it reaches conv_currents): the
    PackedSpikes [T, B, H, W, Cin] of a spike raster, or block 0's frames as given.  A float32 frame
    tensor is looked at once, whole, as ConvBlock's single launch looks at it: integer-valued
    frames go to the integer connection as uint8 ('u8'), others to the float32 one ('real')."""
    if not first:
      return ops.pack_bits(x), "bits"
    if pk.int_weight() is not None and x.dtype == torch.float32:
      whole = bool(((x == torch.round(x)) & (x >= 0) & (x <= 255)).all())
      return x, "u8" if whole else "real"
    return x, "frames"

  @staticmethod
  def chunk_input(kept, form, geom, t0, t1):
    """Steps t0..t1 of the kept input as conv_currents takes them, [NB, H, W, Cin]."""
    xc = kept[t0:t1]
    if form == "bits":
      return xc.reshape_leading(-1, geom.H, geom.W)
    xc = xc.reshape(-1, geom.H, geom.W, geom.Cin)
    return xc.to(torch.uint8) if form == "u8" else xc

  @staticmethod
  def chunk_currents(kept, form, pk, geom, t0, t1):
    """The chunk's raw currents [t1 - t0, B OH OW, C]: the launch of the forward on the same bits,
    so the backward's tensor is the forward's."""
    cur = conv_currents(RematConvBlock.chunk_input(kept, form, geom, t0, t1), pk, geom,
                        real=(form == "real"))
    return cur.reshape(t1 - t0, -1, geom.Cout)

  @staticmethod
  def chunk_scan(cur, mean, var, scale, bias, eps, nrn, tau, u, want_h, want_s):
    """(y, h, s, u_T) of a chunk from the membrane u (None: zeros): the fused kernel for
    multi_step_LIF (y None: never written), ConvBlock.scan_input and the PLIF / LIF scan with a
    `tau` leaf."""
    if tau is None:
      h, s, u_T = ops.bn_lif_forward(cur, mean, bn_multiplier(var, scale, eps), bias, nrn, u0=u,
                                     want_h=want_h, want_s=want_s, return_state=True)
      return None, h, s, u_T
    y = ConvBlock.scan_input(cur, mean, var, scale, bias, eps)
    h, s, u_T = ops.neuron_forward_save(y, nrn, u0=u, return_state=True)
    return y, h, s, u_T

  @staticmethod
  def forward(ctx, x, wq, scale, bias, pk, geom, nrn, surrogate, eps, first, chunk, want_h, tau, u0):
    T, B = x.shape[0], x.shape[1]
    C = geom.Cout
    OH, OW = geom.out_hw()
    if u0 is not None and tuple(u0.shape) != (B, OH, OW, C):
      raise ValueError("RematConvBlock: u0 %s, the block's membranes are %s" % (tuple(u0.shape), (B, OH, OW, C)))
    kept, form = RematConvBlock.kept_input(x, pk, geom, first)
    chunks = remat_chunks(T, chunk) or [(0, 0)]
    # the membrane each chunk starts from: the window's own copy (the caller overwrites the state's
    # buffer with u_T before the backward runs), then what each chunk hands on
    u = None if u0 is None else u0.detach().reshape(B * OH * OW, C).clone()
    starts, means, variances, hs, ss = [], [], [], [], []
    pooled = torch.empty((T, B, OH // 2, OW // 2, C), dtype=torch.float32, device=x.device)
    sd, bd = scale.detach(), bias.detach()
    for t0, t1 in chunks:
      starts.append(u)
      cur = RematConvBlock.chunk_currents(kept, form, pk, geom, t0, t1)
      mean, var = batch_stats(cur)
      y, h, s, u = RematConvBlock.chunk_scan(cur, mean, var, sd, bd, eps, nrn, tau, u, want_h, True)
      del cur, y
      s = s.reshape(t1 - t0, B, OH, OW, C)
      pooled[t0:t1] = ops.maxpool2x2(s)
      means.append(mean)
      variances.append(var)
      if want_h:
        hs.append(h.reshape(t1 - t0, B, OH, OW, C))
        ss.append(s)
      del h, s
    mean, var = torch.cat(means), torch.cat(variances)
    h = torch.cat(hs) if want_h else None
    s = torch.cat(ss) if want_h else None
    del hs, ss
    bits = kept.bits if form == "bits" else kept
    ctx.save_for_backward(bits, wq, scale, bias, mean, var, tau, *[v for v in starts if v is not None])
    ctx.zero_start = starts[0] is None
    ctx.form, ctx.pk, ctx.geom, ctx.nrn, ctx.surrogate, ctx.eps = form, pk, geom, nrn, surrogate, eps
    ctx.first, ctx.chunks, ctx.window, ctx.x_shape = first, chunks, u0 is not None, tuple(x.shape)
    ctx.mark_non_differentiable(*[v for v in (h, s, mean, var) if v is not None])
    u_T = u.reshape(B, OH, OW, C)
    return (pooled, h, s, mean, var) if u0 is None else (pooled, h, s, mean, var, u_T)

  @staticmethod
  def backward(ctx, gp, _gh, _gs, _gmean, _gvar, gu_T=None):
    bits, wq, scale, bias, mean, var, tau, *starts = ctx.saved_tensors
    if ctx.zero_start:
      starts = [None] + starts
    geom, nrn, form = ctx.geom, ctx.nrn, ctx.form
    T, B = ctx.x_shape[0], ctx.x_shape[1]
    C = geom.Cout
    OH, OW = geom.out_hw()
    kept = ops.PackedSpikes(bits, geom.Cin) if form == "bits" else bits
    sd, bd = scale.detach(), bias.detach()
    want_gx = not ctx.first and ctx.needs_input_grad[0]
    gx = torch.empty(ctx.x_shape, dtype=torch.float32, device=gp.device) if want_gx else None
    gw = gscale = gbias = gparam = None
    gu = None if gu_T is None else gu_T.reshape(B * OH * OW, C)
    gp = gp.contiguous()
    for k in range(len(ctx.chunks) - 1, -1, -1):
      t0, t1 = ctx.chunks[k]
      n = t1 - t0
      xin = RematConvBlock.chunk_input(kept, form, geom, t0, t1)
      cur = conv_currents(xin, ctx.pk, geom, real=(form == "real")).reshape(n, B * OH * OW, C)
      y, h, _, _ = RematConvBlock.chunk_scan(cur, mean[t0:t1], var[t0:t1], sd, bd, ctx.eps, nrn, tau,
                                             starts[k], True, False)
      gs = ops.maxpool2x2_backward_h(h.reshape(n, B, OH, OW, C), nrn.v_threshold, gp[t0:t1])
      gs = gs.reshape(n, B * OH * OW, C)
      # the chain: this chunk's gu_T is the gu0 of the chunk after (the block's own for the last)
      want_gu0 = k > 0 or (ctx.window and ctx.needs_input_grad[13])
      if tau is None:
        gy, _, gu = scan_backward(h, None, nrn, ctx.surrogate, None, state=(None, gu, want_gu0), gs=gs)
      else:
        gy, part, gu = ops.neuron_backward(h, y, nrn, ctx.surrogate, gs=gs, u0=starts[k], gu_T=gu,
                                           return_gu0=True)
        gparam = _accumulate(gparam, part)                    # float64, before neuron_param_grad
      del gs, y, h
      gcur, gscale_k, gbias_k = bn_backward(gy, cur, mean[t0:t1], var[t0:t1], scale, ctx.eps)
      del gy, cur
      gscale, gbias = _accumulate(gscale, gscale_k), _accumulate(gbias, gbias_k)
      gcur = gcur.reshape(n * B, OH, OW, C)
      x4 = xin.to_dense() if form == "bits" else xin.to(torch.float32)
      gw = _accumulate(gw, ops.conv_weight_grad(x4, gcur, geom))
      del x4, xin
      if want_gx:
        gx[t0:t1] = ops.conv_input_grad(gcur, wq.detach(), geom).reshape((n,) + ctx.x_shape[1:])
      del gcur
    gtau = None if tau is None else neuron_param_grad(gparam, tau)
    gu0 = gu.reshape(B, OH, OW, C) if ctx.window and ctx.needs_input_grad[13] else None
    return gx, gw, gscale, gbias, None, None, None, None, None, None, None, None, gtau, gu0
