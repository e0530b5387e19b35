"""Step functions -- mirror of examples/train_utils.py (eval_step :370-390, compute_metrics
:220-225, mse_loss :210-217, cross_entropy_loss :196-207, create_model :133-134, and for the
models that train here (DenseSNN, ConvDenseSNN, CextNet) create_train_state :161-195, weight_decay_fn :228-234 and the
offline branch of train_step :249-368), create_learning_rate_fn :44-130 with the optax schedules
it joins as plain functions of an integer step, save_checkpoint / restore_checkpoint :30-41 of a
TrainState and sync_batch_stats :242-246.  Not ported: the online branch.
"""

from __future__ import annotations

import dataclasses
import math
import os
import re
from dataclasses import dataclass
from typing import Any, Callable, Optional

import numpy as np
import torch


@dataclass
class EvalState:
  """The fields of the reference's TrainState that eval_step reads."""
  apply_fn: Callable
  params: dict          # {'params': ...} as in train_utils.py:187-192
  batch_stats: dict


def create_model(*, model_cls, num_classes, model_dtype=torch.float32, **kwargs):
  return model_cls(num_classes=num_classes, dtype=model_dtype, **kwargs)


def onehot(labels, num_classes):
  labels = torch.as_tensor(labels).to(torch.int64)
  return torch.nn.functional.one_hot(labels, num_classes).to(torch.float32)


def mixed_targets(labels, labels2, weight, num_classes):
  """The soft target of mixed recordings: w * onehot(y) + (1 - w) * onehot(y') as
  float32 [B, classes], w the row's `weight` (the share of its own events among those counted)."""
  w = torch.as_tensor(weight).to(torch.float32).reshape(-1, 1)
  a, b = onehot(labels, num_classes), onehot(labels2, num_classes)
  return w.to(a.device) * a + (1 - w.to(a.device)) * b.to(a.device)


def _targets(logits, labels):
  """The target rows of a loss: the one-hot of integer labels, or a 2-D float `labels` -- a soft
  target, [B, classes] -- as it is."""
  if isinstance(labels, torch.Tensor) and labels.dim() == 2 and labels.is_floating_point():
    if tuple(labels.shape) != tuple(logits.shape):
      raise ValueError("a soft target must have the logits' shape %s, got %s" % (tuple(logits.shape), tuple(labels.shape)))
    return labels.to(logits.device)
  return onehot(labels, logits.shape[1]).to(logits.device)


def cross_entropy_loss(logits, labels, smoothing=0):
  oh = _targets(logits, labels)
  oh = oh * (1 - smoothing) + smoothing / oh.shape[1]
  return torch.mean(-(oh * torch.log_softmax(logits, -1)).sum(-1))


def mse_loss(logits, labels, smoothing=0, T=1):
  oh = _targets(logits, labels)
  oh = oh * (1 - smoothing) + smoothing / oh.shape[1]
  return torch.mean(torch.square(logits / T - oh))


def compute_metrics(logits, labels, smoothing, loss_fn):
  loss = loss_fn(logits, labels, smoothing)
  accuracy = torch.argmax(logits, -1) == torch.as_tensor(labels).to(logits.device)
  return {"loss": loss, "accuracy": accuracy}


def eval_step(state, batch, rng, smoothing, loss_type, burnin=0):
  variables = {"params": state.params["params"], "batch_stats": state.batch_stats}
  (logits, _), _ = state.apply_fn(
      variables, batch["dvs_matrix"], trgt=batch["label"], train=False,
      online=False, rng=rng, mutable=["batch_stats"], rngs={"dropout": rng})
  return compute_metrics(logits, batch["label"], smoothing, loss_type)


# ---------------------------------------------------------------------------
# training (offline branch)
# ---------------------------------------------------------------------------


def _flatten(tree, prefix=()):
  """[(path tuple, tensor)] of a nested dict, in insertion order."""
  out = []
  for k, v in tree.items():
    if isinstance(v, dict):
      out.extend(_flatten(v, prefix + (k,)))
    else:
      out.append((prefix + (k,), v))
  return out


def _unflatten(items):
  tree = {}
  for path, v in items:
    node = tree
    for k in path[:-1]:
      node = node.setdefault(k, {})
    node[path[-1]] = v
  return tree


def weight_decay_fn(params):
  """0.5 * sum p^2 over every parameter whose path names no BatchNorm (train_utils.py:228-234;
  DuQ's a, c and the prune mask included, as there)."""
  terms = [torch.sum(torch.square(p)) for path, p in _flatten(params)
           if "BatchNorm" not in str(path) and "bn_init" not in str(path)]
  if not terms:
    return torch.zeros(())
  return 0.5 * sum(terms)


@dataclass
class TrainState(EvalState):
  """The reference's TrainState (flax.training.train_state + batch_stats): `params` holds
  {'params': tree} as plain tensors that `tx` updates in place; `step` counts the updates."""
  tx: Any = None
  step: int = 0


def make_optimizer(config, tensors):
  """optax.adam (defaults: b1 0.9, b2 0.999, eps 1e-8) or optax.sgd(momentum, nesterov) over the
  given tensors, as torch.optim; the learning rate is set by train_step each step."""
  name = config.optimizer
  if name == "adam":
    return torch.optim.Adam(tensors, lr=0.0, betas=(0.9, 0.999), eps=1e-8)
  if name == "sgd":
    momentum = float(config.get("momentum", 0.0) or 0.0)
    return torch.optim.SGD(tensors, lr=0.0, momentum=momentum,
                           nesterov=bool(config.get("nesterov", False)))
  raise ValueError("Unknown optimizer in config: " + str(name))


def create_train_state(variables, config, model) -> TrainState:
  """A TrainState over existing variables (model.init's, or a loaded checkpoint's): the params
  are taken over as they are and updated in place (train_utils.py:161-195 creates them with
  model.init first)."""
  params = variables["params"]
  tensors = []
  for _, p in _flatten(params):
    if p.requires_grad:
      p.requires_grad_(False)
    tensors.append(p)
  tx = make_optimizer(config, tensors)
  return TrainState(apply_fn=model.apply, params={"params": params},
                    batch_stats=variables.get("batch_stats", {}), tx=tx, step=0)


def train_step(state: TrainState, batch, rng, learning_rate_fn, weight_decay, smoothing,
               loss_type, online=False, burnin=0, return_grads=False, u_state=None):
  """One offline step (train_utils.py:249-368): loss = loss_type(logits, labels, smoothing) +
  weight_decay * weight_decay_fn(params); gradients by the model's backward (the blocks
  train_forward.py assembles: dense_train.DenseBlock, conv_train.ConvBlock, tcja_train.TcjaGate), averaged over ranks when torch.distributed is initialised; then one update.
  Returns (state, metrics) -- metrics with loss, accuracy, learning_rate and logits --, and the
  gradient tree as a third element when return_grads.

  u_state (a models.StreamState; DenseSNN and ConvDenseSNN): the batch is one window
  of a recording.  The blocks start from the state's membranes, constants of this step's gradient
  (truncated BPTT, the reference's loss_fn(params, inputs, targets, u_state)), and leave theirs
  there; still one update per call, and the metrics are the window's -- the vote over the
  recording so far is u_state.logits()."""
  if online:
    raise NotImplementedError("the online branch of train_step is not supported")
  from .parallel import mean_over_ranks
  params = state.params["params"]
  items = _flatten(params)
  leaves = [(path, p.detach().requires_grad_(True)) for path, p in items]
  ptree = _unflatten(leaves)
  carried = {} if u_state is None else {"u_state": u_state}
  (logits, _), mutated = state.apply_fn(
      {"params": ptree, "batch_stats": state.batch_stats}, batch["dvs_matrix"],
      trgt=batch["label"], train=True, rng=rng, mutable=["batch_stats"], rngs={"dropout": rng},
      **carried)
  # a mixed batch (input_pipeline, config.mix): the loss is against the soft target of both labels;
  # the model's trgt= and the accuracy stay with the row's own label
  target = batch["label"]
  if "label_mix" in batch and "mix_weight" in batch:
    target = mixed_targets(batch["label"], batch["label_mix"], batch["mix_weight"], logits.shape[1]).to(logits.device)
  loss = loss_type(logits, target, smoothing)
  if weight_decay:
    loss = loss + weight_decay * weight_decay_fn(ptree)
  loss.backward()
  grads = [torch.zeros_like(p) if p.grad is None else p.grad for _, p in leaves]
  mean_over_ranks(grads)
  lr = learning_rate_fn(state.step)
  with torch.no_grad():
    for (_, p), g in zip(items, grads):
      p.grad = g.detach()
    for group in state.tx.param_groups:
      group["lr"] = float(lr)
    state.tx.step()
    for _, p in items:
      p.grad = None
  logits = logits.detach()
  metrics = compute_metrics(logits, batch["label"], smoothing, loss_type)
  if target is not batch["label"]:
    metrics["loss"] = loss_type(logits, target, smoothing)
  metrics["learning_rate"] = lr
  metrics["logits"] = logits
  # the running statistics the apply returned (each rank keeps its own, as the reference does
  # between evals); a model without BatchNorm returns the tree it was given
  new_state = dataclasses.replace(state, step=state.step + 1,
                                  batch_stats=mutated.get("batch_stats", state.batch_stats))
  if return_grads:
    return new_state, metrics, _unflatten([(path, g) for (path, _), g in zip(items, grads)])
  return new_state, metrics


def window_rng(rng, k: int):
  """The rng of window k of a recording whose step was given `rng`.  A torch.Generator is handed on
  as it is: every window draws from it in turn.  An int seed s gives window 0 the seed s itself --
  a recording of one window is the train_step of that seed -- and window k > 0 the seed
  (s + k * 0x9E3779B97F4A7C15) mod 2^63: a function of (s, k) alone, so a run repeats, and the
  windows of the steps seeded s and s + 1 share no seed."""
  if isinstance(rng, torch.Generator) or k == 0:
    return rng
  return (int(rng) + k * 0x9E3779B97F4A7C15) % (1 << 63)


def train_step_windows(state: TrainState, batch, rng, learning_rate_fn, weight_decay, smoothing,
                       loss_type, window, online=False, burnin=0):
  """Truncated BPTT over one batch of recordings: batch["dvs_matrix"] [B, T, ...]
  is cut on T into windows of `window` steps (the last one may be shorter), a fresh
  models.StreamState carries the membranes and the vote from window to window, and every window is
  one train_step -- one update, against the recording's labels -- with the rng window_rng gives it.
  The backward keeps one window's residuals at a time, not the recording's.

  Returns (state, metrics, u_state): the TrainState after the last window, the list of the
  windows' metrics, and the StreamState, whose logits() are the vote over the whole recording.
  window >= T is one train_step."""
  from .models import StreamState
  window = int(window)
  if window < 1:
    raise ValueError("train_step_windows: window must be at least 1 step, got %d" % window)
  x = batch["dvs_matrix"]
  T = x.shape[1]
  u_state, metrics = StreamState(), []
  for k, t0 in enumerate(range(0, T, window)):
    part = dict(batch, dvs_matrix=x[:, t0:t0 + window])
    state, m = train_step(state, part, window_rng(rng, k), learning_rate_fn, weight_decay,
                          smoothing, loss_type, online=online, burnin=burnin, u_state=u_state)
    metrics.append(m)
  return state, metrics, u_state


# ---------------------------------------------------------------------------
# learning-rate schedules (train_utils.py:44-130)
# ---------------------------------------------------------------------------
#
# The optax schedules the reference joins, as functions of an integer step that compute in Python
# floats (float64).  optax is not available here: the formulas are recalled from upstream
# (DESIGN.md 14.2 lists them and says which conventions are recalled only).


def linear_schedule(init_value, end_value, transition_steps):
  """optax.linear_schedule: init -> end over transition_steps, constant after; init at every step
  when transition_steps is 0."""
  init, end, n = float(init_value), float(end_value), float(transition_steps)

  def schedule(step):
    if n <= 0:
      return init
    c = min(max(float(step), 0.0), n)
    return (init - end) * (1.0 - c / n) + end
  return schedule


def cosine_decay_schedule(init_value, decay_steps):
  """optax.cosine_decay_schedule with alpha = 0: init * (1 + cos(pi min(step, n) / n)) / 2."""
  init, n = float(init_value), float(decay_steps)
  if not n > 0:
    raise ValueError("cosine_decay_schedule needs positive decay_steps, got %r" % (decay_steps,))

  def schedule(step):
    c = min(float(step), n)
    return init * 0.5 * (1.0 + math.cos(math.pi * c / n))
  return schedule


def join_schedules(schedules, boundaries):
  """optax.join_schedules: schedule i + 1 takes over at boundaries[i] and counts from there.  The
  cascade is evaluated in order, whatever the boundaries are, so boundaries that do not increase
  (the start_epoch = -1 case of create_learning_rate_fn) still define every step."""
  schedules, boundaries = list(schedules), list(boundaries)

  def schedule(step):
    out = schedules[0](step)
    for b, s in zip(boundaries, schedules[1:]):
      out = out if step < b else s(step - b)
    return out
  return schedule


def piecewise_constant_schedule(init_value, boundaries_and_scales=None):
  """optax.piecewise_constant_schedule: init times the scale of every boundary passed.  A boundary
  counts as passed from the step AFTER it (step > boundary); the step equal to the boundary still
  has the old value."""
  init = float(init_value)
  items = sorted((float(b), float(s)) for b, s in (boundaries_and_scales or {}).items())

  def schedule(step):
    out = init
    for b, s in items:
      if step > b:
        out *= s
    return out
  return schedule


def sgdr_schedule(cosine_kwargs):
  """optax.sgdr_schedule: one warmup_cosine_decay_schedule (end value 0) per dict of init_value,
  peak_value, warmup_steps and decay_steps, each starting where the previous one's decay_steps
  end."""
  schedules, boundaries, at = [], [], 0
  for kw in cosine_kwargs:
    warm = linear_schedule(kw["init_value"], kw["peak_value"], kw["warmup_steps"])
    cos = cosine_decay_schedule(kw["peak_value"], kw["decay_steps"] - kw["warmup_steps"])
    schedules.append(join_schedules([warm, cos], [kw["warmup_steps"]]))
    at += kw["decay_steps"]
    boundaries.append(at)
  return join_schedules(schedules, boundaries[:-1])


def create_learning_rate_fn(config, base_learning_rate: float, steps_per_epoch: int):
  """train_utils.py:44-130, branch for branch and in its order: lr_boundaries_scale, t_max,
  quant.start_epoch, plain warmup + cosine.  Returns step -> learning rate (a Python float)."""
  if "lr_boundaries_scale" in config:
    return piecewise_constant_schedule(
        config.learning_rate,
        {int(k) * steps_per_epoch: v for k, v in config.lr_boundaries_scale.items()})
  if "t_max" in config:
    return sgdr_schedule([{"decay_steps": config.t_max * steps_per_epoch,
                           "init_value": base_learning_rate, "peak_value": base_learning_rate,
                           "warmup_steps": 0}] * math.ceil(config.num_epochs / config.t_max))
  if "quant" in config and "start_epoch" in config.quant:
    start = config.quant.start_epoch
    cosine_fn1 = cosine_decay_schedule(
        base_learning_rate, max(start - config.warmup_epochs, 1) * steps_per_epoch)
    cosine_fn2 = cosine_decay_schedule(
        base_learning_rate, max(config.num_epochs - start - config.warmup_epochs, 1) * steps_per_epoch)
    if config.warmup_epochs != 0.0:
      warmup_fn1 = linear_schedule(0.0, base_learning_rate, config.warmup_epochs * steps_per_epoch)
      warmup_fn2 = linear_schedule(0.0, base_learning_rate, config.warmup_epochs * steps_per_epoch)
      b_len = [config.warmup_epochs * steps_per_epoch,             # :96-100, as it stands there
               (start - config.warmup_epochs) * steps_per_epoch,
               config.warmup_epochs * steps_per_epoch]
      b_len[1] += b_len[0]
      b_len[2] += b_len[1]
      return join_schedules([warmup_fn1, cosine_fn1, warmup_fn2, cosine_fn2], b_len)
    return join_schedules([cosine_fn1, cosine_fn2], [start * steps_per_epoch])
  cosine_fn = cosine_decay_schedule(
      base_learning_rate, max(config.num_epochs - config.warmup_epochs, 1) * steps_per_epoch)
  if config.warmup_epochs != 0.0:
    warmup_fn = linear_schedule(0.0, base_learning_rate, config.warmup_epochs * steps_per_epoch)
    return join_schedules([warmup_fn, cosine_fn], [config.warmup_epochs * steps_per_epoch])
  return cosine_fn


# ---------------------------------------------------------------------------
# checkpoints of a TrainState (train_utils.py:30-41), batch statistics over ranks (:242-246)
# ---------------------------------------------------------------------------


def _rank() -> int:
  import torch.distributed as dist
  return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _host(t) -> np.ndarray:
  return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32, copy=False))


def _host_tree(tree):
  return {k: (_host_tree(v) if isinstance(v, dict) else _host(v)) for k, v in tree.items()}


def _moment_tree(state: TrainState, key: str):
  """{'params': tree} of one per-parameter entry of the torch.optim state; zeros where the
  optimiser has not touched a leaf yet."""
  items = []
  for path, p in _flatten(state.params["params"]):
    m = state.tx.state.get(p, {}).get(key)
    items.append((path, _host(torch.zeros_like(p) if m is None else m)))
  return {"params": _unflatten(items)}


def _opt_kind(tx) -> str:
  if isinstance(tx, torch.optim.Adam):
    return "adam"
  if isinstance(tx, torch.optim.SGD):
    return "sgd_momentum" if tx.param_groups[0]["momentum"] else "sgd"
  raise ValueError("no checkpoint layout for the optimiser %s" % type(tx).__name__)


def _opt_state_dict(state: TrainState):
  """The optimiser state in the layout optax gives the reference's optimisers (chains of two:
  the transform, then scale_by_schedule with its own count)."""
  kind = _opt_kind(state.tx)
  steps = [s["step"] for s in state.tx.state.values() if "step" in s]
  count = np.array(int(steps[0]) if steps else int(state.step), np.int32)
  if kind == "adam":
    first = {"count": count, "mu": _moment_tree(state, "exp_avg"), "nu": _moment_tree(state, "exp_avg_sq")}
  elif kind == "sgd_momentum":
    first = {"trace": _moment_tree(state, "momentum_buffer")}
  else:
    first = {}
  return {"0": first, "1": {"count": count.copy()}}


def state_dict(state: TrainState):
  """TrainState.to_state_dict() of the reference, leaves as float32 numpy arrays."""
  return {"step": int(state.step), "params": {"params": _host_tree(state.params["params"])},
          "opt_state": _opt_state_dict(state), "batch_stats": _host_tree(state.batch_stats)}


_CKPT = re.compile(r"checkpoint_(\d+(?:\.\d+)?)")


def save_checkpoint(state: TrainState, workdir: str, keep: int = 3) -> Optional[str]:
  """Writes workdir/checkpoint_<step> (flax's msgpack format, checkpoint.msgpack_serialize) from
  rank 0, atomically and over an existing file of that step, then deletes all but the `keep`
  newest checkpoints of the directory.  Returns the path, None on the other ranks."""
  if _rank() != 0:
    return None
  from . import checkpoint
  os.makedirs(workdir, exist_ok=True)
  path = os.path.join(workdir, "checkpoint_%d" % int(state.step))
  tmp = path + ".tmp-%d" % os.getpid()
  with open(tmp, "wb") as f:
    f.write(checkpoint.msgpack_serialize(state_dict(state)))
  os.replace(tmp, path)
  found = []
  for name in os.listdir(workdir):
    m = _CKPT.fullmatch(name)
    if m and os.path.isfile(os.path.join(workdir, name)):
      found.append((float(m.group(1)), name))
  for _, name in sorted(found)[:max(len(found) - int(keep), 0)]:
    os.remove(os.path.join(workdir, name))
  return path


def _check_like(got, want, path):
  """Raises ValueError naming the first path at which the restored tree `got` differs from the
  state's tree `want` (dict against dict, array against a tensor of the same shape)."""
  where = "/".join(path) or "<root>"
  if isinstance(want, dict):
    if not isinstance(got, dict):
      raise ValueError("checkpoint does not fit the state at %s: a tree is expected" % where)
    for k in want:
      if k not in got:
        raise ValueError("checkpoint does not fit the state at %s: missing" % "/".join(path + (k,)))
      _check_like(got[k], want[k], path + (k,))
    for k in got:
      if k not in want:
        raise ValueError("checkpoint does not fit the state at %s: not in the state" % "/".join(path + (k,)))
  elif isinstance(got, dict) or tuple(np.shape(got)) != tuple(want.shape):
    raise ValueError("checkpoint does not fit the state at %s: shape %s, the state has %s"
                     % (where, "of a tree" if isinstance(got, dict) else tuple(np.shape(got)), tuple(want.shape)))


def _copy_tree_(dst, src):
  for k, v in dst.items():
    if isinstance(v, dict):
      _copy_tree_(v, src[k])
    else:
      v.copy_(torch.from_numpy(np.ascontiguousarray(src[k], dtype=np.float32)))


def restore_checkpoint(state: TrainState, workdir: str) -> TrainState:
  """The newest checkpoint of `workdir` over `state`, or `state` unchanged when there is none
  (flax's behaviour).  The tensors are copied into the state's own, which the optimiser keeps
  pointing at; the torch.optim state is rebuilt from opt_state and state.step is set."""
  from . import checkpoint
  from .eval import latest_checkpoint
  path = latest_checkpoint(workdir) if workdir and os.path.isdir(workdir) else None
  if path is None:
    return state
  with open(path, "rb") as f:
    tree = checkpoint.msgpack_restore(f.read())
  params = state.params["params"]
  kind = _opt_kind(state.tx)
  moments = {"adam": ("mu", "nu"), "sgd_momentum": ("trace",), "sgd": ()}[kind]
  want_opt = {"0": dict({m: {"params": params} for m in moments},
                        **({"count": torch.zeros(())} if kind == "adam" else {})),
              "1": {"count": torch.zeros(())}}
  _check_like(tree, {"step": torch.zeros(()), "params": {"params": params}, "opt_state": want_opt,
                     "batch_stats": state.batch_stats}, ())
  with torch.no_grad():
    _copy_tree_(params, tree["params"]["params"])
    _copy_tree_(state.batch_stats, tree["batch_stats"])
    opt = tree["opt_state"]
    count = int(opt["1"]["count"])
    state.tx.state.clear()
    if count > 0:            # (at count 0 torch.optim creates its state itself, as zeros)
      got = {m: dict(_flatten(opt["0"][m]["params"])) for m in moments}
      names = {"mu": "exp_avg", "nu": "exp_avg_sq", "trace": "momentum_buffer"}
      for path_, p in _flatten(params):
        entry = {names[m]: torch.from_numpy(np.ascontiguousarray(got[m][path_], dtype=np.float32)).to(p.device)
                 for m in moments}
        if kind == "adam":
          entry = dict(step=torch.tensor(float(opt["0"]["count"]), dtype=torch.get_default_dtype()), **entry)
        if entry:
          state.tx.state[p] = entry
  state.step = int(tree["step"])
  return state


def sync_batch_stats(state: TrainState) -> TrainState:
  """train_utils.py:242-246: every batch_stats leaf becomes its mean over the ranks (one
  all-reduce); the identity when torch.distributed is not initialised."""
  from .parallel import mean_over_ranks
  mean_over_ranks([t for _, t in _flatten(state.batch_stats)])
  return state
