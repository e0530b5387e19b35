"""Step functions -- mirror of examples/train_utils.py (eval_step :370-390, compute_metrics
:220-225, mse_loss :210-217, cross_entropy_loss :196-207, create_model :133-134, and for the
models that train here (DenseSNN, ConvDenseSNN, CextNet) create_train_state :161-195, weight_decay_fn :228-234 and the
offline branch of train_step :249-368).  Not ported: the optax learning-rate schedules (any
step -> lr callable is taken), the online branch, checkpoint writing.
"""

from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Any, Callable, Optional

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


def cross_entropy_loss(logits, labels, smoothing=0):
  oh = onehot(labels, logits.shape[1]).to(logits.device)
  oh = oh * (1 - smoothing) + smoothing / oh.shape[1]
  return torch.mean(-(oh * torch.log_softmax(logits, -1)).sum(-1))


def mse_loss(logits, labels, smoothing=0, T=1):
  oh = onehot(labels, logits.shape[1]).to(logits.device)
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
               loss_type, online=False, burnin=0, return_grads=False):
  """One offline step (train_utils.py:249-368): loss = loss_type(logits, labels, smoothing) +
  weight_decay * weight_decay_fn(params); gradients by the model's backward (the blocks
  train_forward.py assembles: dense_train.DenseBlock, conv_train.ConvBlock, tcja_train.TcjaGate), averaged over ranks when torch.distributed is initialised; then one update.
  Returns (state, metrics) -- metrics with loss, accuracy, learning_rate and logits --, and the
  gradient tree as a third element when return_grads."""
  if online:
    raise NotImplementedError("the online branch of train_step is not supported")
  from .parallel import mean_over_ranks
  params = state.params["params"]
  items = _flatten(params)
  leaves = [(path, p.detach().requires_grad_(True)) for path, p in items]
  ptree = _unflatten(leaves)
  (logits, _), mutated = state.apply_fn(
      {"params": ptree, "batch_stats": state.batch_stats}, batch["dvs_matrix"],
      trgt=batch["label"], train=True, rng=rng, mutable=["batch_stats"], rngs={"dropout": rng})
  loss = loss_type(logits, batch["label"], smoothing)
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
  metrics["learning_rate"] = lr
  metrics["logits"] = logits
  # the running statistics the apply returned (each rank keeps its own, as the reference does
  # between evals); a model without BatchNorm returns the tree it was given
  new_state = dataclasses.replace(state, step=state.step + 1,
                                  batch_stats=mutated.get("batch_stats", state.batch_stats))
  if return_grads:
    return new_state, metrics, _unflatten([(path, g) for (path, _), g in zip(items, grads)])
  return new_state, metrics
