"""Pack-time inputs of the hot path: prune masks and DuQ `a`, `c` -- mirror of
examples/train_inpt_spikingjelly.py:147-223 (host side, run once per model).

  update_prune_mask     per-layer magnitude mask (:147-157)
  global masks          one magnitude threshold over all kernels in tree order
                        (:174-223, the path the shipped configs reach:
                        `prune_global = True`)
  update_quant_params   a = c = init_fn(kernel, bits, sign=True) (:159-172)

They operate on the `params` tree ({'QuantConv_0': {'kernel', 'DuQ_0', 'prune_0'},
...}) and return a new tree; leaves stay torch tensors on their device.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch


def check_quant_obj(x) -> bool:
  """A quantised layer's leaf dict (has 'kernel'), train_inpt_spikingjelly.py:199-204."""
  return isinstance(x, dict) and "kernel" in x


def _map_layers(fn, tree):
  if check_quant_obj(tree):
    return fn(tree)
  if isinstance(tree, dict):
    return {k: _map_layers(fn, v) for k, v in tree.items()}
  return tree


def _layers(tree, out=None):
  out = [] if out is None else out
  if check_quant_obj(tree):
    out.append(tree)
  elif isinstance(tree, dict):
    for v in tree.values():
      _layers(v, out)
  return out


def _like(arr: np.ndarray, ref: torch.Tensor):
  return torch.from_numpy(np.ascontiguousarray(arr)).to(ref.device, ref.dtype)


def update_prune_mask(params, prune_percentage: float):
  """Local (layer-wise) pruning: zero the int(numel * p) smallest |kernel|."""
  def f(x):
    k = x["kernel"].detach().cpu().numpy()
    mask = np.ones(k.shape)
    n = int(np.prod(k.shape) * prune_percentage)
    idx = np.argpartition(np.abs(k).reshape(-1), n)[:n]
    mask.reshape(-1)[idx] = 0
    y = dict(x)
    y["prune_0"] = {"mask": _like(mask, x["kernel"])}
    return y
  return _map_layers(f, params)


def update_global_prune_mask(params, prune_percentage: float):
  """Global pruning: one magnitude cut over the concatenation of all kernels."""
  layers = _layers(params)
  flat = np.concatenate([l["kernel"].detach().cpu().numpy().reshape(-1) for l in layers])
  gm = np.ones(flat.shape)
  n = int(np.prod(flat.shape) * prune_percentage)
  idx = np.argpartition(np.abs(flat), n)[:n]
  gm[idx] = 0
  off = [0]

  def f(x):
    sz = int(np.prod(x["kernel"].shape))
    local = gm[off[0]:off[0] + sz].reshape(tuple(x["kernel"].shape))
    off[0] += sz
    y = dict(x)
    y["prune_0"] = {"mask": _like(local, x["kernel"])}
    return y
  return _map_layers(f, params)


def update_quant_params(params, init_fn, bits: int):
  """DuQ_0/{a, c} = init_fn(kernel, bits=bits, sign=True), shape (1,)."""
  def f(x):
    v = init_fn(x["kernel"], bits=bits, sign=True).reshape(1).to(torch.float32)
    y = dict(x)
    y["DuQ_0"] = {"a": v.clone(), "c": v.clone()}
    return y
  return _map_layers(f, params)


def prepare_params(params, config, prune: bool = True):
  """The sequence of train_inpt_spikingjelly.py:206-230 for a `config.quant`.  prune=False leaves
  the one-shot masks out (a run with `quant.prune_schedule` prunes in its loop) and gives every
  layer that has none a mask of ones."""
  q = config.quant
  if not prune:
    params = ones_masks(params)
  elif q.prune_percentage > 0.:
    if "prune_global" in q and q.prune_global is False:
      params = update_prune_mask(params, q.prune_percentage)
    else:
      params = update_global_prune_mask(params, q.prune_percentage)
  if "start_epoch" not in q or q.start_epoch == -1:
    params = update_quant_params(params, q.init_fn, q.bits)
  return params


# ---------------------------------------------------------------------------
# Gradual magnitude pruning inside the training loop
# ---------------------------------------------------------------------------
#
# `config.quant.prune_schedule = dict(start_epoch=, end_epoch=, every_steps=, initial=0.0)` with the
# final sparsity `config.quant.prune_percentage`: the cubic schedule of Zhu & Gupta ("To prune, or
# not to prune", 2017).  The masks are selected on the device (ops.magnitude_prune); nothing here
# reads a tensor.

PRUNE_SCHEDULE_KEYS = ("start_epoch", "end_epoch", "every_steps", "initial")


class PruneSchedule(NamedTuple):
  """Steps, not epochs: events at t0, t0 + every, ..., t1."""
  t0: int
  t1: int
  every: int
  initial: float

  def is_event(self, step: int) -> bool:
    return self.t0 <= step <= self.t1 and (step - self.t0) % self.every == 0


def check_prune_schedule(q):
  """Refuses a `config.quant` whose prune_schedule cannot be run (ValueError); returns the
  schedule as a plain dict with `initial` filled in.  Looks at the config alone."""
  sched = dict(q["prune_schedule"])
  unknown = sorted(set(sched) - set(PRUNE_SCHEDULE_KEYS))
  if unknown:
    raise ValueError("quant.prune_schedule: unknown keys %s (known: %s)" % (unknown, list(PRUNE_SCHEDULE_KEYS)))
  missing = [k for k in PRUNE_SCHEDULE_KEYS[:3] if k not in sched]
  if missing:
    raise ValueError("quant.prune_schedule: missing keys %s" % missing)
  final = float(q.get("prune_percentage", 0.0))
  if not 0.0 < final <= 1.0:
    raise ValueError("quant.prune_schedule needs 0 < quant.prune_percentage <= 1 (the final sparsity), got %r" % final)
  sched.setdefault("initial", 0.0)
  if int(sched["every_steps"]) != sched["every_steps"] or sched["every_steps"] < 1:
    raise ValueError("quant.prune_schedule: every_steps = %r, must be an integer >= 1" % (sched["every_steps"],))
  if not 0.0 <= float(sched["initial"]) <= final:
    raise ValueError("quant.prune_schedule: initial = %r outside [0, prune_percentage = %r]" % (sched["initial"], final))
  if sched["start_epoch"] < 0:
    raise ValueError("quant.prune_schedule: start_epoch = %r < 0" % (sched["start_epoch"],))
  if sched["end_epoch"] < sched["start_epoch"]:
    raise ValueError("quant.prune_schedule: end_epoch = %r before start_epoch = %r"
                     % (sched["end_epoch"], sched["start_epoch"]))
  return sched


def resolve_prune_schedule(q, steps_per_epoch: int) -> PruneSchedule:
  """The schedule of `config.quant` in steps.  t1 is the last step t0 + j every_steps that is no
  later than end_epoch * steps_per_epoch: the last event lands exactly on the final sparsity."""
  sched = check_prune_schedule(q)
  every = int(sched["every_steps"])
  t0 = int(sched["start_epoch"] * steps_per_epoch)
  end = int(sched["end_epoch"] * steps_per_epoch)
  return PruneSchedule(t0, t0 + (end - t0) // every * every, every, float(sched["initial"]))


def sparsity_at(step: int, schedule: PruneSchedule, final: float) -> float:
  """s(t) = final + (initial - final) (1 - (t - t0) / (t1 - t0))^3 in Python floats, `initial` up
  to t0 and `final` from t1 on (t1 == t0: `final`).  Non-decreasing in t."""
  final = float(final)
  if step >= schedule.t1:
    return final
  if step <= schedule.t0:
    return schedule.initial
  left = 1.0 - (step - schedule.t0) / (schedule.t1 - schedule.t0)
  return min(max(final + (schedule.initial - final) * left ** 3, schedule.initial), final)


def ones_masks(params):
  """A mask of ones on every quantised layer that has none (a new tree; existing masks stay)."""
  def f(x):
    if "prune_0" in x:
      return x
    y = dict(x)
    y["prune_0"] = {"mask": torch.ones_like(x["kernel"])}
    return y
  return _map_layers(f, params)


def prune_event(params, sparsity: float, global_: bool = True) -> None:
  """One prune event at `sparsity`: the masks of the quantised layers of `params`,
  in tree order, grow to int(count * sparsity) zeros by the rule of ops.magnitude_prune -- over
  the concatenation of all kernels (global_, one launch sequence) or layer by layer.  The masks
  are written INTO the leaves the optimiser holds (its moments stay); an entry already pruned stays
  pruned whatever its kernel value has become.  Everything stays on the kernels' device: no host
  read, nothing returned.  Every rank of a data-parallel run holds the same kernels and masks and
  the rule is a function of their values alone, so each rank prunes for itself: no collective."""
  from . import ops
  layers = _layers(params)
  for l in layers:
    if "prune_0" not in l:
      raise ValueError("prune_event: a quantised layer without a prune_0/mask leaf")
  if not layers:
    return
  with torch.no_grad():
    if not global_:
      for l in layers:
        mask = l["prune_0"]["mask"]
        ops.magnitude_prune(l["kernel"].detach().to(torch.float32), mask, int(mask.numel() * sparsity))
      return
    w = torch.cat([l["kernel"].detach().to(torch.float32).reshape(-1) for l in layers])
    m = torch.cat([l["prune_0"]["mask"].detach().reshape(-1) for l in layers])
    ops.magnitude_prune(w, m, int(m.numel() * sparsity))
    off = 0
    for l in layers:
      mask = l["prune_0"]["mask"]
      mask.copy_(m[off:off + mask.numel()].reshape(mask.shape))
      off += mask.numel()


def mask_zeros(params):
  """(zeros, weights) of the masks of `params`: zeros a 0-d int64 tensor on the masks' device (the
  caller reads it when it logs), weights a Python int."""
  layers = _layers(params)
  zeros = sum((l["prune_0"]["mask"] == 0).sum() for l in layers)
  return zeros, sum(int(l["prune_0"]["mask"].numel()) for l in layers)


# ---------------------------------------------------------------------------
# Channel liveness: output channels the prune mask leaves unable to spike
# ---------------------------------------------------------------------------
#
# An output channel whose largest reachable input current keeps the membrane below threshold
# never fires, whatever the input; its spikes are zeros that the next layer multiplies by its
# codes.  The rule and its float32 proof are DESIGN.md section 9.  Everything below is host-side
# numpy on the packed codes and the folded BatchNorm constants, run once per weight version.

_EPS32 = 2.0 ** -24          # unit roundoff of float32
_ETA32 = 2.0 ** -126         # absolute error of one float32 operation near zero (subnormals, FTZ)
_K_MIN = 2.0 ** -16          # smallest convex factor the slack below is derived for


def _np(a):
  if a is None:
    return None
  if isinstance(a, torch.Tensor):
    return a.detach().cpu().numpy()
  return np.asarray(a)


def _current_f32(acc, L, m, bn):
  """Input current of integer accumulators `acc` (int64 [C]) in the kernels' and the oracle's
  float32 operation order: y = fl(fl(acc / L) * m), then fl(fl(fl(y - mean) * mul) + bias)."""
  f = np.float32
  y = (acc.astype(f) / f(L)) * f(m)
  if bn is not None:
    mean, mul, bias = bn
    y = ((y - mean.astype(f)) * mul.astype(f)) + bias.astype(f)
  return y.astype(f)


def _neuron_factor(neuron):
  """(convex factor k in (0, 1] of the membrane update, v_threshold, v_reset), or None when the
  update is not a convex combination the proof covers."""
  from . import _lib as L
  kind = getattr(neuron, "kind", None)
  vth, vr = float(np.float32(neuron.v_threshold)), float(np.float32(neuron.v_reset))
  if kind == L.NEURON_MULTI_STEP_LIF:
    tau = float(np.float32(neuron.k))
    if not tau >= 1.0:
      return None
    k = 1.0 / tau
  elif kind == L.NEURON_PARAMETRIC_LEAKY_IF:
    k = float(np.float32(neuron.k))      # sigmoid(tau), rounded to float32: (0, 1]
    if not 0.0 < k <= 1.0:
      return None
  else:
    return None                          # LIF: u * k + x is not convex in (u, x)
  if k < _K_MIN:
    return None
  return k, vth, vr


def channel_liveness(kernel_codes, dequant, bn, neuron, x_max, live_in=None, u0=None):
  """Output channels that can fire: bool numpy [Cout] (True = live).

  kernel_codes  integer codes * mask, input channels on axis -2 and output channels on axis -1
                (HWIO conv or [K, N] dense)
  dequant       (L, m) of y = fl(fl(acc / L) * m); None for float (fake-quantised) weights
  bn            (mean, mul, bias) float32 [Cout] of the folded eval BatchNorm
                (linen.BatchNorm.coeffs; ops.BnCoeffs is taken too), or None
  neuron        ops.Neuron of the block
  x_max         largest input value: 1 spikes / EV1 frames, 15 EV4, 255 uint8 frames
  live_in       bool [Cin]: input channels that may be non-zero (None: all)
  u0            a carried-in membrane state (anything but None: nothing is provably silent)

  A channel is silent when the block starts from zero state, its neuron update is convex
  (multi_step_LIF with tau >= 1, parametric_leaky_IF) and max(0, x_hi + v_reset) plus the float32
  rounding slack of DESIGN.md 9 stays below v_threshold, x_hi being the largest current its
  reachable accumulators [-neg * x_max, pos * x_max] give.  In every other case every channel is
  live."""
  codes = _np(kernel_codes)
  live = np.ones(codes.shape[-1], bool)
  if dequant is None:
    return live
  nf = _neuron_factor(neuron)
  if nf is None or u0 is not None:
    return live
  k, vth, vr = nf
  if not vth > 0.0:
    return live
  c = codes.reshape((-1,) + codes.shape[-2:]).astype(np.int64)       # [taps, Cin, Cout]
  if live_in is not None:
    li = np.asarray(_np(live_in), bool)
    assert li.shape == (c.shape[1],), (li.shape, c.shape)
    c = c * li[None, :, None]
  pos = np.clip(c, 0, None).sum((0, 1))
  neg = np.clip(-c, 0, None).sum((0, 1))
  if isinstance(bn, (tuple, list)) or bn is None:
    bnn = None if bn is None else tuple(_np(v).astype(np.float32) for v in bn)
  else:
    bnn = (_np(bn.mean).astype(np.float32), _np(bn.mul).astype(np.float32),
           _np(bn.bias).astype(np.float32))
  L_, m_ = dequant
  xm = int(x_max)
  # dequantisation and BatchNorm are monotone in the accumulator: the extremes of the current are
  # at the two ends of the reachable accumulator range
  e1 = _current_f32(pos * xm, L_, m_, bnn).astype(np.float64)
  e0 = _current_f32(-neg * xm, L_, m_, bnn).astype(np.float64)
  x_hi, x_lo = np.maximum(e0, e1), np.minimum(e0, e1)
  fin = np.isfinite(x_hi) & np.isfinite(x_lo)       # (a NaN / inf current proves nothing)
  # exact in float64: both terms are float32
  bound = np.maximum(0.0, x_hi + vr)
  S = np.maximum(np.abs(x_hi), np.abs(x_lo)) + abs(vr)
  slack = (32.0 * _EPS32 * S + 8.0 * _ETA32) / k
  silent = fin & (bound + slack + 2.0 * _ETA32 < vth)
  return ~silent


def computed_channels(live, multiple: int = 32):
  """The channel set a compacted block computes: its live channels in their original order,
  padded with silent ones (appended in original order) to a multiple of `multiple` (at least
  one multiple).  int64 numpy indices."""
  live = np.asarray(live, bool)
  idx = np.flatnonzero(live)
  n = max(multiple, -(-idx.size // multiple) * multiple)
  n = min(n, live.size)
  pad = np.flatnonzero(~live)[:n - idx.size]
  return np.concatenate([idx, pad]).astype(np.int64)


def half_group_fire(n_live: int, n_computed: int) -> int:
  """snnqp_weight_t.cout_fire of a compacted event layer: computed_channels puts the
  live channels first, so the computed channels from 16 ceil(live / 16) on are silent padding.
  Where that leaves the upper 16 channels of the last 32-channel group silent (live mod 32 in
  1 .. 16) the kernel computes that group in a 16-channel half; otherwise 0: nothing to say."""
  fire = -(-int(n_live) // 16) * 16
  return fire if 0 < fire < int(n_computed) else 0


def _host_codes(leaf, bits):
  """DuQ codes * mask of a layer leaf on the host (round half to even of hard_tanh(w / a) * L,
  float32), and (L, m); None when the layer is not integer-coded (a == -1, bits > 8)."""
  f = np.float32
  w = _np(leaf["kernel"]).astype(f)
  a = f(_np(leaf["DuQ_0"]["a"]).reshape(-1)[0])
  c = f(_np(leaf["DuQ_0"]["c"]).reshape(-1)[0])
  if a == f(-1) or bits == -1 or bits > 8:
    return None
  L_ = f(2 ** (bits - 1) - 1)
  q = np.rint(np.clip(w / a, f(-1), f(1)) * L_)
  if "prune_0" in leaf:
    q = q * _np(leaf["prune_0"]["mask"]).astype(f)
  return q.astype(np.int64), (float(L_), float(c))


def _host_bn(params, stats, name, eps=1e-5):
  f = np.float32
  mean = _np(stats[name]["mean"]).astype(f)
  var = _np(stats[name]["var"]).astype(f)
  mul = f(1) / np.sqrt(var + f(eps))
  if "scale" in params[name]:
    mul = mul * _np(params[name]["scale"]).astype(f)
  bias = _np(params[name]["bias"]).astype(f) if "bias" in params[name] else np.zeros_like(mean)
  return mean, mul.astype(f), bias


def conv_net_liveness(variables, config, x_max, nblocks: int = 3, neuron=None):
  """Liveness of the conv blocks QuantConv_0 .. nblocks-1 of models.ConvDenseSNN (or the three
  plain conv blocks of models.CextNet) for model inputs bounded by `x_max`, cascaded: a block's
  live input rows are the previous block's live outputs.  Returns a list of bool [Cout] arrays.
  `neuron` (ops.Neuron) defaults to the config's multi_step_LIF."""
  from . import _lib as L
  from . import ops
  params, stats = variables["params"], variables.get("batch_stats", {})
  if neuron is None:
    nd = config.neuron_dynamics
    kw = dict(getattr(nd, "keywords", {}) or {})
    neuron = ops.Neuron(L.NEURON_MULTI_STEP_LIF, float(np.float32(kw.get("tau", 2.0))),
                        float(kw.get("v_threshold", 1.0)), float(kw.get("v_reset", 0.0)))
  q = config.quant
  out, live_in, xm = [], None, int(x_max)
  for i in range(nblocks):
    bits = int(q.layer_bits[i]) if ("layer_bits" in q and q.layer_bits is not None) else q.bits
    hc = _host_codes(params["QuantConv_%d" % i], bits) if "weight" in q else None
    if hc is None:
      live = np.ones(_np(params["QuantConv_%d" % i]["kernel"]).shape[-1], bool)
    else:
      live = channel_liveness(hc[0], hc[1], _host_bn(params, stats, "BatchNorm_%d" % i), neuron,
                              xm, live_in)
    out.append(live)
    live_in, xm = live, 1                # spikes from here on
  return out
