"""Models for the BASELINE.json configurations, built from the same blocks and
with the same call signature as the reference's CextNet
(examples/tcja/models.py:31-257):

  CextNet       the reference's full DVS128 model: 3 conv blocks, 2 conv blocks each
                followed by a TCJA attention gate, channel-major flatten, two
                dense blocks, vote (models.py:31-257)
  DenseSNN      configs C1 / C2: the two-layer head of CextNet,
                QuantDense(hidden)+LIF -> QuantDense(num_classes*10)+LIF -> vote
                (models.py:200-255)
  ConvDenseSNN  config C3: the three `for i in range(3)` conv blocks
                (QuantConv 3x3 + BatchNorm + LIF + 2x2 max-pool, models.py:111-147)
                -> channel-major flatten (:189-190) -> QuantDense + LIF (:231-246)
                -> vote (:253-255)

Variable names follow Flax auto-naming in construction order (QuantConv_i,
BatchNorm_i, QuantDense_i; tcja_load_pretrained_weights.py:19-36).

All three train (`apply(..., train=True, rng=...)`): the training forward
is each model's `_train_forward`, attached to torch autograd through the parameter leaves.

DenseSNN and ConvDenseSNN stream (`apply(variables, window, u_state=StreamState())`):
the membranes of every block and the read-out's spike counts survive between calls.
"""

from __future__ import annotations

from typing import Any, Callable

import torch

from . import linen as nn
from . import ops
from . import packing
from .flax_qconv import QuantConv
from .flax_qdense import QuantDense
from .spiking_learning import SpikingBlock, fused_dense_head


def flatten_channel_major(x):
  """transpose (T,B,C,H,W) + reshape [T, B, C*H*W]  (models.py:189-190).

  Packed spikes are not moved: the NHWC words are re-labelled and the consumer
  re-orders its weight rows (an exact re-indexing of an integer sum)."""
  if isinstance(x, ops.GatedSpikes):
    return x.flattened()
  if isinstance(x, ops.PackedSpikes):
    T, B, H, W, C = x.shape
    if C % 32:
      x = ops.expand_channels(x)
      C = x.channels
    if C % 32:
      d = x.to_dense().permute(0, 1, 4, 2, 3).reshape(T, B, C * H * W)
      return ops.pack_bits(d.contiguous())
    out = ops.PackedSpikes(x.bits.reshape(T, B, H * W * (C // 32)), H * W * C)
    out.flat_perm = (C, H, W)
    out.chan_map = x.chan_map      # a compacted raster: the read-out takes its rows
    return out
  x = x.permute(0, 1, 4, 2, 3)
  return x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3] * x.shape[4]).contiguous()   # (no -1: B may be 0)


def _layer_bits(cfg, i):
  """Bit width of the i-th quantised layer: `config.quant.layer_bits[i]` when
  given (mixed precision, BASELINE config C5), else `config.quant.bits`; every
  layer has its own `bits` attribute in the reference (flax_qconv.py:89)."""
  q = cfg.quant
  if "layer_bits" in q and q.layer_bits is not None:
    return int(q.layer_bits[i])
  return q.bits


# The layers every model is made of, for the eval and the training forward alike.  Each call
# constructs one module, which Flax auto-naming numbers in order of construction: callers
# construct them in the reference's order.

def _qconv3x3(cfg, dtype, bits):
  return QuantConv(features=cfg.channels, kernel_size=(3, 3), padding=((1, 1), (1, 1)),
                   use_bias=False, dtype=dtype, config=cfg.quant, bits=bits,
                   g_scale=cfg.quant.g_scale)


def _qconv1d(cfg, dtype, bits, features):
  return QuantConv(features=features, kernel_size=[4], padding="SAME", use_bias=False,
                   dtype=dtype, config=cfg.quant, bits=bits, g_scale=cfg.quant.g_scale)


def _qdense(cfg, dtype, bits, features):
  return QuantDense(features, use_bias=False, dtype=dtype, config=cfg.quant, bits=bits,
                    g_scale=cfg.quant.g_scale)


def _batchnorm(dtype, train=False):
  return nn.BatchNorm(use_running_average=not train, momentum=0.9, epsilon=1e-5, use_bias=True,
                      use_scale=True, dtype=dtype)


def _probing(mod, cfg):
  """Density probes are sown under the reference's names (models.py:45-51,128-142) when the
  caller both asks for them (config.density_probes) and made 'intermediates' mutable.  The
  reference sows them unconditionally -- under jit an unread probe costs nothing; here each
  probe is a kernel launch, and the `*_out_*` probes need the UNPOOLED raster, so the blocks
  then run with the 2x2 max-pool as a separate pass."""
  return bool(cfg.get("density_probes", False)) and mod.is_mutable_collection("intermediates")


def _compacting(mod, cfg, u_state):
  """Whether the plain conv blocks compute only the channels that can fire:
  nn.set_channel_compaction (default on), off while density probes run or a state carry is given."""
  return nn.channel_compaction() and not _probing(mod, cfg) and u_state is None


def _sow_raster(mod, name, x):
  """Sows a block's spikes at their logical width (a compacted raster is scattered back)."""
  if mod.is_mutable_collection("intermediates"):
    mod.sow("intermediates", name, ops.expand_channels(x))


def _sow_density(mod, name, x, lead_dims=2):
  """sparse_nums = nnz / size per leading slice; `<name>_min` is its MAXIMUM (the reference's
  naming, models.py:131-133) and `<name>_mean` its mean, float32 device scalars."""
  d = ops.density(x, lead_dims=lead_dims).reshape(-1)
  mod.sow("intermediates", name + "_min", d.max())
  mod.sow("intermediates", name + "_mean", d.mean())


def _as_input(inputs):
  if isinstance(inputs, (ops.PackedSpikes, ops.PackedFrames, ops.GatedSpikes)):
    return inputs
  x = torch.as_tensor(inputs)
  if x.dtype not in (torch.uint8, torch.float32):
    x = x.to(torch.float32)
  return x


class StreamState:
  """What a model carries from one window of a stream to the next:

    membranes  the float32 potentials of every SpikingBlock, in model order: [B, OH, OW, C] at the
               block's own, pre-pool resolution for a conv block, [B, N] for a dense block
    counts     int32 [B, N_out]: the read-out's spike counts so far
    row_steps  int32 [B]: the steps every batch row has seen since its last reset
    steps      host int: the steps since the state was created or last reset as a whole

  `StreamState()` is empty; the first `apply(..., u_state=state)` sizes it with zeros (the initial
  potentials of initialize_carry).  Every later call updates the same tensors."""

  def __init__(self):
    self.membranes = []
    self.counts = None
    self.row_steps = None
    self.steps = 0

  @classmethod
  def zeros(cls, shapes, n_out, device=None):
    """A zero state for blocks whose membranes have `shapes` (each [B, ...]) and n_out read-out neurons."""
    st = cls()
    st._fit([tuple(int(d) for d in sh) for sh in shapes], int(n_out), device)
    return st

  def _fit(self, shapes, n_out, device):
    """Sizes an empty state; ValueError when a sized one is not for these blocks / this batch / device."""
    B = shapes[0][0]
    if self.counts is None:
      self.membranes = [torch.zeros(sh, dtype=torch.float32, device=device) for sh in shapes]
      self.counts = torch.zeros((B, n_out), dtype=torch.int32, device=device)
      self.row_steps = torch.zeros((B,), dtype=torch.int32, device=device)
      self.steps = 0
      return
    have = [tuple(u.shape) for u in self.membranes]
    if self.counts.shape[0] != B:
      raise ValueError("u_state holds %d batch rows, the window has %d" % (self.counts.shape[0], B))
    if have != list(shapes) or tuple(self.counts.shape) != (B, n_out):
      raise ValueError("u_state was sized for membranes %s and %d outputs, this model and window need %s and %d"
                       % (have, self.counts.shape[1], list(shapes), n_out))
    if device is not None and self.counts.device != torch.device(device):
      raise ValueError("u_state lives on %s, the window on %s" % (self.counts.device, device))

  def _tensors(self):
    return list(self.membranes) + [self.counts, self.row_steps]

  def advance(self, steps: int):
    """Books `steps` time steps for every row (the model does this once per window)."""
    self.steps += int(steps)
    self.row_steps += int(steps)

  def logits(self, group: int = 10):
    """float32 [B, num_classes]: the vote over every step so far -- counts / steps, then the in-order
    mean over each class's `group` neurons: the operations and order of ops.vote, on the device
    (snnqp_vote_counts).  A row that has seen no step votes 0."""
    if self.counts is None:
      raise ValueError("an empty StreamState has no vote")
    if self.counts.is_cuda:
      return ops.vote_counts(self.counts, self.row_steps, group)
    B, N = self.counts.shape
    if N % group:
      raise ValueError("vote: %d features not divisible by group %d" % (N, group))
    steps = self.row_steps.to(torch.float32)[:, None]
    mean_t = (self.counts.to(torch.float32) / steps).reshape(B, N // group, group)
    acc = torch.zeros((B, N // group), dtype=torch.float32)
    for g in range(group):
      acc = acc + mean_t[:, :, g]
    return torch.where(steps > 0, acc / float(group), torch.zeros_like(acc))

  def reset(self, rows=None):
    """Zeroes the membranes, counts and step counts of the batch rows `rows` (all rows when None):
    a new recording starts in those slots."""
    if self.counts is None:
      return self
    if rows is None:
      for t in self._tensors():
        t.zero_()
      self.steps = 0
      return self
    idx = torch.as_tensor(rows, dtype=torch.long).reshape(-1)
    B = self.counts.shape[0]
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= B):
      raise ValueError("reset: rows %s outside the state's %d batch rows" % (idx.tolist(), B))
    idx = idx.to(self.counts.device)
    for t in self._tensors():
      t.index_fill_(0, idx, 0)
    return self

  def clone(self):
    """A snapshot: new tensors with the same values."""
    st = StreamState()
    st.membranes = [u.clone() for u in self.membranes]
    st.counts = None if self.counts is None else self.counts.clone()
    st.row_steps = None if self.row_steps is None else self.row_steps.clone()
    st.steps = self.steps
    return st


def _stream_state(mod, cfg, u_state):
  """The StreamState of an eval call (None: the whole-run call), after the refusals every model shares."""
  if u_state is None:
    return None
  if not isinstance(u_state, StreamState):
    raise TypeError("u_state must be a models.StreamState, got %s" % type(u_state).__name__)
  if _probing(mod, cfg):
    raise NotImplementedError("density probes together with u_state: probe the whole-run call")
  return u_state


def _window_done(state, x, window_logits, steps):
  """The read-out raster `x` of a window behind the per-block path: counted, voted, booked."""
  ops.vote_accumulate(x, state.counts)
  state.advance(steps)
  return window_logits, state


def _carry(state, i, layer, x):
  """Block i of a stream on the per-block path.  A block there may be a launch pair (the float32 stand-by
  of ops.FloatFallback, the event layer's binary-first launch and its redo), so it never updates a
  potential in place: it reads the state's buffer, writes u_T to a buffer of its own, and that is
  copied into the state's -- whose address stays what a captured window was recorded with."""
  u_T, x = layer(state.membranes[i], x)
  state.membranes[i].copy_(u_T)
  return x


# The dense head of a given set of parameters, prepared once: what `fused_dense_head` hands to
# the kernel depends on the parameter tensors (identity and version), the two bit widths, the
# quantiser and neuron factories of the config and the input's layout -- nothing else.  A step
# whose keys match skips the module machinery (ten modules bound and ~400 Python calls to arrive
# at the same two descriptors): config C2 is a 0.03 ms kernel, the host must not cost more.
_head_plans = None


def _head_key(mod, cfg, x, hidden, nout):
  """(tensors, extra) identifying the head's prepared launch, or None when the step is not the
  plain one (initialising, mutable collections, probes, parameters missing or of another shape)."""
  root = mod._root
  if root.initializing or root.mutable or mod._path != ():
    return None
  if isinstance(x, ops.PackedSpikes):
    if not (x.bits.is_cuda and x.ndim == 3 and x.flat_perm is None):
      return None
  elif not (isinstance(x, torch.Tensor) and x.dtype in (torch.uint8, torch.float32) and x.is_cuda
            and x.ndim == 3 and x.is_contiguous()):
    return None
  if isinstance(x, torch.Tensor) and x.dtype == torch.float32 and not packing.AUTO_INTEGER_INPUTS:
    return None
  p = root.variables.get("params")
  try:
    l0, l1 = p["QuantDense_0"], p["QuantDense_1"]
    ts = (l0["kernel"], l0["DuQ_0"]["a"], l0["DuQ_0"]["c"], l0["prune_0"]["mask"],
          l1["kernel"], l1["DuQ_0"]["a"], l1["DuQ_0"]["c"], l1["prune_0"]["mask"])
  except (KeyError, TypeError):
    return None
  # the neurons' own parameters (PLIF / LIF `tau`): a training step moves them too
  ts += tuple(v["tau"] for _, v in sorted(p.items())
              if isinstance(v, dict) and isinstance(v.get("tau"), torch.Tensor))
  q = cfg.quant
  extra = (type(x).__name__, str(getattr(x, "dtype", "")), tuple(x.shape), hidden, nout, _layer_bits(cfg, 0), _layer_bits(cfg, 1), id(q.get("weight")),
           float(q.prune_percentage) >= 0.0, id(cfg.neuron_dynamics))
  return ts, extra


class DenseSNN(nn.Module):
  """inputs [B, T, K] -> logits [B, num_classes] (configs C1 / C2)."""
  num_classes: int = 11
  dtype: Any = torch.float32
  config: dict = nn.FrozenConfigDict({})

  def __call__(self, inputs, trgt=None, train: bool = False, rng: Any = None,
               u_state=None, online=False):
    if train:
      return self._train_forward(inputs, rng, u_state, online)
    cfg = self.config
    x = _as_input(inputs)
    hidden = cfg.hidden if "hidden" in cfg else cfg.channels * 2 * 2
    probe = _probing(self, cfg)
    state = _stream_state(self, cfg, u_state)
    nout = self.num_classes * 10
    if state is not None:
      if x.ndim != 3:
        raise ValueError("DenseSNN expects [B, T, K] inputs, got %s" % (tuple(x.shape),))
      B, steps = x.shape[0], x.shape[1]
      state._fit([(B, hidden), (B, nout)], nout, x.device)
      if steps == 0:                                   # nothing to scan: the state stays as it is
        return torch.zeros((B, self.num_classes), dtype=torch.float32, device=x.device), state
    global _head_plans
    key = None if probe else _head_key(self, cfg, x, hidden, nout)
    if key is not None:
      if state is not None:
        key = (key[0], key[1] + ("stream",))           # a stateless plan is never a stateful call's
      if _head_plans is None:
        from ._cache import TensorCache
        _head_plans = TensorCache(32)
      plan = _head_plans.get(*key)
      if plan is not None:
        w1, K, N1, nrn1, w2, N2, nrn2, group, tm, fb, _refs = plan
        if state is not None:
          return self._head_window(state, steps, ops.dense_head_forward_state(
              x, w1, K, N1, nrn1, w2, N2, nrn2, state.membranes[0], state.membranes[1], state.counts,
              group=group, time_major=tm, fallback=fb))
        return ops.dense_head_forward(x, w1, K, N1, nrn1, w2, N2, nrn2, group=group, time_major=tm,
                                      fallback=fb)[0], None
    layer = SpikingBlock(
        connection_fn=_qdense(cfg, self.dtype, _layer_bits(cfg, 0), hidden),
        neural_dynamics=cfg.neuron_dynamics(dtype=self.dtype),
        return_state=state is not None, batch_major_input=True)
    layer2 = SpikingBlock(
        connection_fn=_qdense(cfg, self.dtype, _layer_bits(cfg, 1), nout),
        neural_dynamics=cfg.neuron_dynamics(dtype=self.dtype),
        return_state=state is not None)
    if not probe:
      # both blocks and the vote as one launch when the head fits it (the hidden raster then
      # never leaves the CU); the output raster only when somebody collects the intermediates
      want_s2 = self.is_mutable_collection("intermediates")
      head = fused_dense_head(layer, layer2, x, 10, want_s1=want_s2 and state is not None, want_s2=want_s2,
                              state=None if state is None else (state.membranes[0], state.membranes[1], state.counts))
      if head is not None:
        if want_s2:
          if state is not None:
            self.sow("intermediates", "dense1_out", head[1])
          self.sow("intermediates", "dense2_out", head[2])
        if key is not None and fused_dense_head.last_plan is not None:
          # (the factories are kept alive with the plan: their ids are part of its key)
          _head_plans.put(key[0], key[1], fused_dense_head.last_plan + ((cfg.quant.get("weight"), cfg.neuron_dynamics),))
        if state is not None:
          return self._head_window(state, steps, head)
        return head[0], None
    if state is not None:
      # the head does not fit the one launch: block by block with their carries, the counting vote
      x = _carry(state, 0, layer, x)
      self.sow("intermediates", "dense1_out", x)
      x = _carry(state, 1, layer2, x)
      self.sow("intermediates", "dense2_out", x)
      return _window_done(state, x, ops.vote(x, 10), steps)
    if probe:
      _sow_density(self, "dense1_inpt", x)
    _, x = layer(None, x)
    if probe:
      _sow_density(self, "dense1_out", x)
      _sow_density(self, "dense2_inpt", x)
    _, x = layer2(None, x)
    self.sow("intermediates", "dense2_out", x)
    if probe:
      _sow_density(self, "dense2_out", x)
    return ops.vote(x, 10), None                       # models.py:253-255

  @staticmethod
  def _head_window(state, steps, head):
    """Books a window the stateful head has run: it counted into state.counts itself; the membranes
    are the tensors it hands back (the state's own, or -- float32 rows -- the copies it wrote)."""
    state.membranes[0], state.membranes[1] = head[3], head[4]
    state.advance(steps)
    return head[0], state

  def _train_forward(self, inputs, rng, u_state, online):
    """The training forward of models.py:191-255 (dropout masks M0 on the input and M1 on the
    hidden spikes, keep probability config.dropout, not rescaled), attached to torch autograd
    through the parameter leaves (dense_train.py).  Same spikes and logits as the eval forward
    when every mask is one."""
    from . import dense_train as dt
    from . import train_forward as fw
    cfg = self.config
    x = fw.check_call(self, inputs, rng, u_state, online, frames=False, carries=True,
                      remat="its residuals are weight-sized, not image-sized (DESIGN.md 18.6)")
    hidden = cfg.hidden if "hidden" in cfg else cfg.channels * 2 * 2
    nout = self.num_classes * 10
    B, steps = x.shape[0], x.shape[1]
    state, empty = fw.window_state(self, u_state, [(B, hidden), (B, nout)], nout, B, x.device)
    if state is not None and steps == 0:               # nothing to scan: the state stays as it is
      return empty, state
    dense1 = fw.dense_layer(self, hidden, _layer_bits(cfg, 0), x.shape[-1])
    dense2 = fw.dense_layer(self, self.num_classes * 10, _layer_bits(cfg, 1), hidden)
    gen = dt.generator_of(rng, x.device)
    m0 = dt.dropout_mask(x.shape, cfg.dropout, gen, x.device)           # models.py:193-197
    if self.is_mutable_collection("intermediates"):
      self.sow("intermediates", "dropout_0", m0)
    x = dt.input_time_major(dt.apply_input_mask(x, m0))                 # [T, B, K], in x's own dtype
    if state is not None:                              # a window of a recording, DESIGN.md 18
      x = fw.dense_block(self, x, "dense1", dense1, None, first=True, state=(state, 0))
      logits, s = fw.dense_block(self, x, "dense2", dense2, 10, mask=(gen, 1), state=(state, 1))
      return fw.window_done(state, s, logits, steps)
    x = fw.dense_block(self, x, "dense1", dense1, None, first=True)     # models.py:200-216
    logits = fw.dense_block(self, x, "dense2", dense2, 10, mask=(gen, 1))   # models.py:219-255
    return logits, None


class ConvDenseSNN(nn.Module):
  """inputs [B, T, H, W, 2] -> logits [B, num_classes] (config C3)."""
  num_classes: int = 11
  dtype: Any = torch.float32
  config: dict = nn.FrozenConfigDict({})

  def __call__(self, inputs, trgt=None, train: bool = False, rng: Any = None,
               u_state=None, online=False):
    if train:
      return self._train_forward(inputs, rng, u_state, online)
    cfg = self.config
    x = _as_input(inputs)
    nblocks = cfg.num_conv_blocks if "num_conv_blocks" in cfg else 3
    probe = _probing(self, cfg)
    state = _stream_state(self, cfg, u_state)
    compact = _compacting(self, cfg, u_state)
    nout = self.num_classes * 10
    if state is not None:
      if x.ndim != 5:
        raise ValueError("ConvDenseSNN expects [B, T, H, W, 2] inputs, got %s" % (tuple(x.shape),))
      B, steps, H, W = x.shape[:4]
      # a conv block's membranes at its own resolution: the 2x2 pool halves what the next one sees
      state._fit([(B, H >> i, W >> i, cfg.channels) for i in range(nblocks)] + [(B, nout)], nout, x.device)
      if steps == 0:                                   # nothing to scan: the state stays as it is
        return torch.zeros((B, self.num_classes), dtype=torch.float32, device=x.device), state
    for i in range(nblocks):
      layer = SpikingBlock(
          connection_fn=_qconv3x3(cfg, self.dtype, _layer_bits(cfg, i)),
          neural_dynamics=cfg.neuron_dynamics(dtype=self.dtype),
          norm_fn=_batchnorm(self.dtype),
          pool=1 if probe else 2,       # the reduce_window max of models.py:145-147
          return_state=state is not None,
          batch_major_input=(i == 0),   # models.py:109 swapaxes, done by strides
          compact=compact)
      if probe:
        _sow_density(self, "conv_%d_inpt" % i, x)
      if state is not None:
        x = _carry(state, i, layer, x)
      else:
        _, x = layer(None, x)
      if probe:
        _sow_density(self, "conv_%d_out" % i, x)
        x = ops.maxpool2x2(x)
      _sow_raster(self, "pool%d" % i, x)
    x = flatten_channel_major(x)
    if probe:
      _sow_density(self, "dense1_inpt", x)
    layer = SpikingBlock(
        connection_fn=_qdense(cfg, self.dtype, _layer_bits(cfg, nblocks), nout),
        neural_dynamics=cfg.neuron_dynamics(dtype=self.dtype),
        return_state=state is not None)
    if state is not None:
      x = _carry(state, nblocks, layer, x)
      self.sow("intermediates", "dense_out", x)
      return _window_done(state, x, ops.vote(x, 10), steps)
    _, x = layer(None, x)
    self.sow("intermediates", "dense_out", x)
    if probe:
      _sow_density(self, "dense1_out", x)
    return ops.vote(x, 10), None

  def _train_forward(self, inputs, rng, u_state, online):
    """The training forward of models.py:101-147, :189-190, :219-255 (BatchNorm on batch
    statistics, one dropout mask with keep probability config.dropout, not rescaled, in front of
    the read-out), attached to torch autograd through the parameter leaves (conv_train.py,
    dense_train.py).  Channel compaction and the fused kernels are not used."""
    from . import dense_train as dt
    from . import train_forward as fw
    x = fw.check_call(self, inputs, rng, u_state, online, frames=True, carries=True)
    cfg = self.config
    remat = cfg.remat if "remat" in cfg else None         # steps per chunk, DESIGN.md 19
    nblocks = cfg.num_conv_blocks if "num_conv_blocks" in cfg else 3
    nout = self.num_classes * 10
    B, steps, H, W = x.shape[:4]
    # (a conv block's membranes at its own resolution, as the eval path sizes them)
    state, empty = fw.window_state(
        self, u_state, [(B, H >> i, W >> i, cfg.channels) for i in range(nblocks)] + [(B, nout)],
        nout, B, x.device)
    if state is not None and steps == 0:               # nothing to scan: the state stays as it is
      return empty, state
    x = x.transpose(0, 1).contiguous()                    # models.py:109, [T, B, H, W, C]
    for i in range(nblocks):                              # models.py:111-147
      x = fw.conv_block(self, x, i, _layer_bits(cfg, i), first=(i == 0), state=state, remat=remat)
    x = flatten_channel_major(x)                          # models.py:189-190
    dense = fw.dense_layer(self, nout, _layer_bits(cfg, nblocks), x.shape[-1])
    mask = (dt.generator_of(rng, x.device), 0)
    if state is not None:                              # a window of a recording, DESIGN.md 18
      logits, s = fw.dense_block(self, x, "dense", dense, 10, mask=mask, state=(state, nblocks))
      return fw.window_done(state, s, logits, steps)
    logits = fw.dense_block(self, x, "dense", dense, 10, mask=mask)     # models.py:219-255
    return logits, None


class CextNet(nn.Module):
  """TCJA-SNN, examples/tcja/models.py:31-257 (eval forward; train=True: _train_forward).

  inputs [B, T, H, W, 2] -> (logits [B, num_classes], None).  Variables:
  QuantConv_0..8, BatchNorm_0..4, QuantDense_0..1 in the reference's order
  (tcja_load_pretrained_weights.py:19-36).  After the first TCJA gate the
  activations are real-valued: those layers use the float (fmaf-chain) kernels
  with the fake-quantised weights, as the reference does."""
  num_classes: int = 11
  dtype: Any = torch.float32
  config: dict = nn.FrozenConfigDict({})

  def __call__(self, inputs, trgt=None, train: bool = False, rng: Any = None,
               u_state=None, online=False):
    if train:
      return self._train_forward(inputs, rng, u_state, online)
    if u_state is not None:
      raise NotImplementedError(
          "CextNet does not stream: its TCJA gates are convolutions over the window's time axis with T "
          "features, so a window shorter than the configured T has no defined gate (DESIGN.md 15)")
    cfg = self.config

    def qconv1d(features, x):
      return _qconv1d(cfg, self.dtype, cfg.quant.bits, features)(x)

    probe = _probing(self, cfg)

    def TCJA(x_seq, i=0, gated=False):                  # models.py:41-99
      T, C = x_seq.shape[0], x_seq.shape[-1]
      m = ops.spatial_mean(x_seq)                       # [T, B, C]
      x = m.transpose(0, 1).contiguous()                # [B, T, C]
      x_c = x.transpose(1, 2).contiguous()              # [B, C, T]
      with packing.integer_inputs(False):               # channel means are real-valued
        conv_t_out = qconv1d(T, x_c)                    # [B, C, T]
        conv_c_out = qconv1d(C, x)                      # [B, T, C]
      if probe:                                         # per sample, models.py:45-91
        _sow_density(self, "conv_tcja1_%d_inpt" % i, x_c, 1)
        _sow_density(self, "conv_tcja1_%d_out" % i, conv_t_out, 1)
        _sow_density(self, "conv_tcja2_%d_inpt" % i, x, 1)
        _sow_density(self, "conv_tcja2_%d_out" % i, conv_c_out, 1)
      conv_t_out = conv_t_out.permute(2, 0, 1).contiguous()   # [T, B, C]
      conv_c_out = conv_c_out.transpose(0, 1).contiguous()    # [T, B, C]
      gate = ops.sigmoid_gate(conv_c_out, conv_t_out)
      self.sow("intermediates", "tcja_gate_%d" % i, gate)
      # The reference gates the raster and then max-pools it 2x2 (models.py:99, 145-147).
      # The gate is a sigmoid (>= 0) and constant over H, W, the raster is 0/1, so
      # max(g * s_i) == g * max(s_i) exactly: pool the spikes first (an OR of bits) and
      # gate the pooled raster -- a quarter of the float32 traffic, same numbers.
      pooled = ops.maxpool2x2(x_seq)
      if gated and isinstance(pooled, ops.PackedSpikes):
        # the next block is a quantised 3x3 conv (i = 0) or the flatten + dense block (i = 1): it
        # contracts gate x raster without the product being written (SpikingBlock._gated_block;
        # config.gated_int = False multiplies it out)
        return ops.GatedSpikes(pooled, gate)
      return ops.apply_gate(pooled, gate)   # [T, B, H/2, W/2, C] float32

    compact = _compacting(self, cfg, u_state)

    def conv_block(x, first, pool, packed=None, compact=False):
      layer = SpikingBlock(
          connection_fn=_qconv3x3(cfg, self.dtype, cfg.quant.bits),
          neural_dynamics=cfg.neuron_dynamics(dtype=self.dtype),
          norm_fn=_batchnorm(self.dtype),
          pool=pool, return_state=False, batch_major_input=first, packed=packed, compact=compact)
      return layer(None, x)[1]

    def dense_block(x, features, packed=None):
      layer = SpikingBlock(
          connection_fn=_qdense(cfg, self.dtype, cfg.quant.bits, features),
          neural_dynamics=cfg.neuron_dynamics(dtype=self.dtype), return_state=False, packed=packed)
      return layer(None, x)[1]

    x = _as_input(inputs)
    for i in range(3):                                  # models.py:111-147
      if probe:
        _sow_density(self, "conv_%d_inpt" % i, x)
      # (the plain blocks feed 3x3 conv blocks: they may compact; conv_t_0 / 1 feed the TCJA gates,
      # whose channel-axis convolution needs every channel)
      x = conv_block(x, first=(i == 0), pool=1 if probe else 2, compact=compact)
      if probe:
        _sow_density(self, "conv_%d_out" % i, x)
        x = ops.maxpool2x2(x)
      _sow_raster(self, "pool%d" % i, x)
    real_valued = False
    for i in range(2):                                  # models.py:149-187
      if probe:
        _sow_density(self, "conv_t_%d_inpt" % i, x)
      with packing.integer_inputs(not real_valued):
        # TCJA needs the unpooled raster; bit-packed also when the input is real-valued
        x = conv_block(x, first=False, pool=1, packed=True)
      self.sow("intermediates", "conv_t_%d" % i, x)
      if probe:
        _sow_density(self, "conv_t_%d_out" % i, x)
      # gated and pooled; the blocks behind the gates may take the product unmultiplied
      x = TCJA(x, i, gated=bool(cfg.get("gated_int", True)))
      real_valued = True
    x = flatten_channel_major(x)                        # models.py:189-190
    if probe:
      _sow_density(self, "dense1_inpt", x)
    with packing.integer_inputs(False):
      # real-valued inputs, but what comes out are spikes: bit-packed, so that dense2 runs on the
      # integer kernels without anybody having to look at the values first
      x = dense_block(x, cfg.channels * 2 * 2, packed=True)          # models.py:200-216
    self.sow("intermediates", "dense1_out", x)
    if probe:
      _sow_density(self, "dense1_out", x)
      _sow_density(self, "dense2_inpt", x)
    x = dense_block(x, self.num_classes * 10)           # models.py:231-246
    self.sow("intermediates", "dense2_out", x)
    if probe:
      _sow_density(self, "dense2_out", x)
    return ops.vote(x, 10), None

  def _train_forward(self, inputs, rng, u_state, online):
    """The training forward of models.py:101-257 (BatchNorm on batch statistics in all five conv
    blocks, the two TCJA gates, dropout masks with keep probability config.dropout, not rescaled,
    in front of both dense blocks), attached to torch autograd through the parameter leaves
    (conv_train.py, tcja_train.py, dense_train.py).  Behind the first gate the activations are
    real-valued: those blocks run the float32 connection on the multiplied-out product, as eval
    does under config.gated_int = False.  Channel compaction, the gated integer kernels and the
    fused kernels are not used."""
    from . import dense_train as dt
    from . import train_forward as fw
    x = fw.check_call(self, inputs, rng, u_state, online, frames=True, min_hw=32, gpu=True,
                      remat="its first block's weight gradient runs the float64 chain of DESIGN.md 12.3, "
                            "and per-chunk roundings of that chain are not served")
    cfg = self.config
    bits = cfg.quant.bits
    x = x.transpose(0, 1).contiguous()                    # models.py:109, [T, B, H, W, C]
    for i in range(3):                                    # models.py:111-147
      # block 0's weight gradient in float64: the most rows, count frames
      x = fw.conv_block(self, x, i, bits, first=(i == 0), wgrad_f64=(i == 0))
    for j in range(2):                                    # models.py:149-187
      if self.is_mutable_collection("intermediates"):     # what a test steps the oracle block on
        self.sow("intermediates", "conv%d_in" % (3 + j), x.detach())
      x = fw.conv_block(self, x, 3 + j, bits, pool=1, real_input=(j == 1))
      x = fw.tcja_gate(self, x, j, bits)
    x = flatten_channel_major(x)                          # models.py:189-190
    gen = dt.generator_of(rng, x.device)
    hidden = cfg.channels * 2 * 2
    x = fw.dense_block(self, x, "dense1", fw.dense_layer(self, hidden, bits, x.shape[-1]), None,
                       mask=(gen, 0), real_input=True)    # models.py:192-216
    logits = fw.dense_block(self, x, "dense2", fw.dense_layer(self, self.num_classes * 10, bits, hidden),
                            10, mask=(gen, 1))            # models.py:223-255
    return logits, None
