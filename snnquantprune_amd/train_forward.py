"""What the three training forwards (models.py, `_train_forward`) are assembled from: the refusals
of a training call, and one function per kind of block.  Each block function constructs the
block's modules in the reference's order (Flax auto-naming numbers them as it does for eval),
attaches the block to torch autograd through the layer's own parameter leaf, and sows the saved
forward values under '<name>_h', '<name>_out', ... when 'intermediates' is mutable."""

from __future__ import annotations

import torch

from . import conv_train as ct
from . import dense_train as dt
from . import ops
from . import tcja_train as tt
from .models import _as_input, _batchnorm, _probing, _qconv1d, _qconv3x3, _qdense
from .quant import DuQ

_PACKED = (ops.PackedSpikes, ops.PackedFrames, ops.GatedSpikes)


def check_call(mod, inputs, rng, u_state, online, frames, min_hw=0, gpu=False, carries=False,
               remat=None):
  """Refuses what training does not support and returns the input tensor.

  carries: the model trains over windows of a recording (DenseSNN, ConvDenseSNN) and
  takes a models.StreamState as u_state.  Anything else given as u_state is refused by every
  model, and a StreamState by a model that does not carry (CextNet: its TCJA gates).  No refusal
  touches the state.

  remat: None, or why this model does not serve config.remat -- the key is then
  refused after every other refusal of the call's arguments; a model that serves it (ConvDenseSNN)
  has its value checked there, conv_train.check_remat.

  frames: the conv models -- a uint8 or float32 [B, T, H, W, C] tensor (of at least min_hw x
  min_hw), looked at before the rng, the config or the parameters, and on the GPU (`gpu`) once
  they are in order.  Otherwise DenseSNN -- the config first, then anything [B, T, K] that
  models._as_input takes as a tensor."""
  if frames:
    if isinstance(inputs, _PACKED) or not (isinstance(inputs, torch.Tensor) and inputs.ndim == 5
                                            and inputs.dtype in (torch.uint8, torch.float32)):
      raise NotImplementedError("training takes uint8 or float32 [B, T, H, W, C] tensors")
    if inputs.shape[2] < min_hw or inputs.shape[3] < min_hw:
      raise NotImplementedError("training %s needs frames of at least %d x %d (five 2x2 pools "
                                "leave the read-out an empty raster), got %d x %d"
                                % (type(mod).__name__, min_hw, min_hw, inputs.shape[2], inputs.shape[3]))
  mask, lines = ("mask", "219-224") if frames else ("masks", "193-197")
  cfg = mod.config
  if rng is None:
    raise NotImplementedError("train=True needs an rng (an int seed or a torch.Generator) for "
                              "the dropout %s; the reference splits it unconditionally" % mask)
  from .models import StreamState
  if online or (u_state is not None and not isinstance(u_state, StreamState)):
    raise NotImplementedError("training: the online mode and a carried state that is not a "
                              "models.StreamState are not supported")
  if u_state is not None and not carries:
    raise NotImplementedError(
        "training %s over windows: its TCJA gates are convolutions over the window's time axis with "
        "T features, so a window shorter than the configured T has no defined gate (DESIGN.md 15)"
        % type(mod).__name__)
  if _probing(mod, cfg):
    raise NotImplementedError("training: density probes are not supported")
  if "dropout" not in cfg:
    raise ValueError("train=True needs config.dropout (the keep probability of the dropout "
                     "%s, models.py:%s)" % (mask, lines))
  qw = cfg.quant.get("weight")
  if qw is not None and getattr(qw, "func", qw) is not DuQ:
    raise NotImplementedError("training supports the DuQ weight quantiser or none, not %r" % (qw,))
  if frames:
    _check_remat(mod, remat)
    if gpu:
      ops._require_gpu(inputs)
    return inputs
  if not (isinstance(inputs, torch.Tensor) or hasattr(inputs, "__array__")) or isinstance(inputs, _PACKED):
    raise NotImplementedError("training takes uint8 or float32 [B, T, K] tensors")
  x = _as_input(inputs)
  if x.ndim != 3:
    raise ValueError("DenseSNN expects [B, T, K] inputs, got %s" % (tuple(x.shape),))
  _check_remat(mod, remat)
  return x


def _check_remat(mod, why):
  """config.remat on a model that does not serve it (`why`) is refused; on one that does, its
  value is checked.  Nothing is launched and no state is looked at."""
  if "remat" not in mod.config:
    return
  if why is not None:
    raise NotImplementedError("training %s with config.remat: %s" % (type(mod).__name__, why))
  ct.check_remat(mod.config.remat)


def _transformed_kernel(mod, layer, pk):
  """dense_train.transformed_kernel of the layer's own leaf: the one its packed_kernel read."""
  leaf = mod._root.variables["params"]
  for name in layer._path:
    leaf = leaf[name]
  return dt.transformed_kernel(leaf, pk)


def _tau_leaf(mod, dyn, kind):
  """The block's own `tau` leaf when its neuron's parameter is learnt (dt.neuron_train_form gave
  PLIF or LIF), found as _transformed_kernel finds the kernel's: the tensor dyn.neuron() read, so
  the gradient reaches the leaf the caller holds.  None for multi_step_LIF."""
  if kind == dt.L.NEURON_MULTI_STEP_LIF:
    return None
  leaf = mod._root.variables["params"]
  for name in dyn._path:
    leaf = leaf[name]
  return leaf["tau"]


def carry_membrane(state, k, u_T):
  """Block k's u_T of a window into the state's own buffer (whose address stays): the value only --
  the next window reads it detached (truncated BPTT, the reference's train_step)."""
  with torch.no_grad():
    state.membranes[k].copy_(u_T)


def conv_block(mod, x, i, bits, pool=2, first=False, real_input=False, wgrad_f64=False, state=None,
               remat=None):
  """Conv block i on x [T, B, H, W, Cin]: QuantConv 3x3, BatchNorm on batch statistics, LIF, the
  2x2 max pool (conv_train.ConvBlock, whose arguments the last four are) -> the pooled spikes.
  Moves the running statistics and sows conv<i>_h, conv<i>_out, bn<i>_mean, bn<i>_var.
  state: a fitted models.StreamState -- the scan starts from state.membranes[i], a constant of this
  window's gradient, and leaves u_T there.
  remat: the steps per chunk of conv_train.RematConvBlock (config.remat), which then
  is the block; it keeps h and the spikes only for the sow."""
  cfg, C = mod.config, mod.config.channels
  conv = _qconv3x3(cfg, mod.dtype, bits)
  dyn = cfg.neuron_dynamics(dtype=mod.dtype)
  norm = _batchnorm(mod.dtype, train=True)
  surr, kind = dt.neuron_train_form(dyn, cfg)
  cin = x.shape[4]
  geom = conv.geometry((x.shape[2], x.shape[3]), cin)
  pk = conv.packed_kernel(cin)
  wq = _transformed_kernel(mod, conv, pk)
  nrn = dyn.neuron(C)
  u0 = None if state is None else state.membranes[i].detach()
  if remat is None:
    y, h, s, mean, var, *u_T = ct.ConvBlock.apply(
        x, wq, norm.scale_param(C), norm.bias_param(C), pk, geom, nrn, surr,
        float(norm.epsilon), first, pool, real_input, wgrad_f64, _tau_leaf(mod, dyn, kind), u0)
  else:
    assert pool == 2 and not real_input and not wgrad_f64, "RematConvBlock: ConvDenseSNN's blocks only"
    y, h, s, mean, var, *u_T = ct.RematConvBlock.apply(
        x, wq, norm.scale_param(C), norm.bias_param(C), pk, geom, nrn, surr,
        float(norm.epsilon), first, remat, mod.is_mutable_collection("intermediates"),
        _tau_leaf(mod, dyn, kind), u0)
  if state is not None:
    carry_membrane(state, i, u_T[0])
  norm.update_running(mean, var)
  if mod.is_mutable_collection("intermediates"):
    mod.sow("intermediates", "conv%d_h" % i, h)
    mod.sow("intermediates", "conv%d_out" % i, s)
    mod.sow("intermediates", "bn%d_mean" % i, mean)
    mod.sow("intermediates", "bn%d_var" % i, var)
  return y


def tcja_gate(mod, x, j, bits):
  """TCJA gate j on the spike raster x [T, B, H, W, C] (tcja_train.TcjaGate) -> the gated, pooled
  raster; sows tcja_gate_<j>."""
  T, C = x.shape[0], x.shape[-1]
  args = []
  for features, spatial, cin in ((T, C, T), (C, T, C)):   # over the channel axis on [B, C, T], over time on [B, T, C]
    conv = _qconv1d(mod.config, mod.dtype, bits, features)
    pk = conv.packed_kernel(cin)
    args.append((_transformed_kernel(mod, conv, pk), pk, conv.geometry((spatial,), cin)))
  (wq_t, pk_t, geom_t), (wq_c, pk_c, geom_c) = args
  y, gate = tt.TcjaGate.apply(x, wq_t, wq_c, pk_t, pk_c, geom_t, geom_c)
  if mod.is_mutable_collection("intermediates"):
    mod.sow("intermediates", "tcja_gate_%d" % j, gate)
  return y


def dense_layer(mod, features, bits, K):
  """Constructs the modules of a dense block K -> features and packs its kernel: what dense_block
  takes as `layer`.  The quantiser's scalars are read back here -- DenseSNN does so for both
  layers before it enqueues any work, so that no read-back waits for block 1's kernels."""
  dense = _qdense(mod.config, mod.dtype, bits, features)
  dyn = mod.config.neuron_dynamics(dtype=mod.dtype)
  return dense, dyn, dt.neuron_train_form(dyn, mod.config), dense.packed_kernel(K)


def dense_block(mod, x, name, layer, group, mask=None, first=False, real_input=False, state=None):
  """A dense block on x [T, B, K]: QuantDense, LIF and, with `group`, the vote
  (dense_train.DenseBlock, whose arguments the last three are) -> the logits, or the spikes of a
  hidden block (group None).  mask (generator, n): draws the block's dropout mask, shaped like
  x, and sows it as dropout_<n>; None: no mask.  Sows <name>_out and <name>_h.
  state (a fitted models.StreamState, k): the scan starts from state.membranes[k], a constant of
  this window's gradient, and leaves u_T there; with `group` -> (logits, s), the read-out raster
  for the state's counts."""
  dense, dyn, (surr, kind), pk = layer
  m = None if mask is None else dt.dropout_mask(x.shape, mod.config.dropout, mask[0], x.device)
  wq = _transformed_kernel(mod, dense, pk)
  nrn = dyn.neuron(dense.features)
  out, s, h, *u_T = dt.DenseBlock.apply(
      x, wq, m, pk, nrn, surr, group, first, real_input, _tau_leaf(mod, dyn, kind),
      None if state is None else state[0].membranes[state[1]].detach())
  if state is not None:
    carry_membrane(*state, u_T[0])
  if mod.is_mutable_collection("intermediates"):
    if m is not None:
      mod.sow("intermediates", "dropout_%d" % mask[1], m)
    mod.sow("intermediates", name + "_out", (out if group is None else s).detach())
    mod.sow("intermediates", name + "_h", h)
  if state is not None and group is not None:
    return out, s
  return out


def window_state(mod, u_state, shapes, n_out, B, device):
  """The StreamState of a training call fitted to this model and window before any launch (None:
  the whole-run call), and the zero logits of a window without a step (else None)."""
  if u_state is None:
    return None, None
  u_state._fit(shapes, n_out, device)
  return u_state, torch.zeros((B, mod.num_classes), dtype=torch.float32, device=device)


def window_done(state, s, logits, steps):
  """Books a training window as the eval path books one: the read-out raster into the counts, the
  steps for every row -> (window logits, state)."""
  ops.vote_accumulate(s.detach(), state.counts)
  state.advance(steps)
  return logits, state
