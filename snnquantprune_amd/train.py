"""Training loop -- mirror of examples/train.py:70-338 (`train_and_evaluate(config, workdir)`) with
the fine-tuning workflow of examples/train_inpt_spikingjelly.py:127-424 folded in: load a
pretrained tree, prune it, switch quantisation on at `quant.start_epoch`, train, evaluate every
epoch, keep the best checkpoint.  DESIGN.md 14 has the rules; in short:

  * every launch of a step is an existing kernel (events_bin, the training forward and backward,
    the optimiser's update); the loop puts no host read between them.  Metrics stay on the device
    until a log point (`config.log_every_steps`), an evaluation or a checkpoint;
  * a step's batch, dropout seed and learning rate are functions of (config.seed, rank, step)
    alone, and the gradient kernels are atomics-free, so a run resumed from `checkpoint_<step>`
    continues bit for bit where the uninterrupted run would be;
  * one PROCESS per GPU, as in eval.py; rank 0 writes the checkpoints and the records
    (`workdir/train/metrics.jsonl`, `workdir/eval/metrics.jsonl`: one JSON object per line, in
    place of the reference's clu writers).

  python -m snnquantprune_amd.train --config CONFIG.py --workdir DIR
  python -m snnquantprune_amd.eval --config CONFIG.py --workdir DIR
CONFIG.py defines get_config() as for eval.py, with the reference's training keys: dataset,
eval_dataset (event or image sources, input_pipeline.py; images: encoding, image_layout), batch_size, eval_batch_size, num_epochs,
num_train_steps, steps_per_eval, learning_rate, warmup_epochs, optimizer, weight_decay,
smoothing, log_every_steps, checkpoint_every_epochs, pretrained, quant.start_epoch.

`quant.prune_schedule = dict(start_epoch=, end_epoch=, every_steps=, initial=0.0)` (optional; this
port's own key) prunes gradually inside the loop instead of once at load: at the steps
t0, t0 + every_steps, ..., t1 the masks grow, by magnitude and on the device, to the cubic
schedule's sparsity, which reaches `quant.prune_percentage` at t1; the event runs in front of the
step's train_step and is recorded as {"step", "event": "prune", "sparsity", "zeros", "weights"}.
An evaluation can be `best` only once the event at t1 has run.  Every rank holds the same weights
and the selection is deterministic, so each rank prunes for itself and no collective is added.
"""

from __future__ import annotations

import argparse
import hashlib
import json
import logging
import os
import time
from typing import Optional

import torch

from . import checkpoint, input_pipeline, parallel
from . import linen as nn
from .eval import eval_pass, initialized, load_config
from .train_utils import (TrainState, create_learning_rate_fn, create_model, create_train_state,
                          mse_loss, restore_checkpoint, save_checkpoint, sync_batch_stats, train_step)


def step_rng(seed: int, rank: int, step: int) -> int:
  """The dropout seed of a step: a function of (seed, rank, step) and nothing else, so that a
  step's masks do not depend on which steps this process ran before it."""
  h = hashlib.sha256(("train_step/%d/%d/%d" % (int(seed), int(rank), int(step))).encode()).digest()
  return int.from_bytes(h[:8], "little") >> 1


class _Records:
  """One JSON object per line, appended and flushed per record; silent off rank 0."""

  def __init__(self, path: str, enabled: bool):
    self.path = path if enabled else None
    if self.path:
      os.makedirs(os.path.dirname(self.path), exist_ok=True)

  def read(self):
    if not self.path or not os.path.exists(self.path):
      return []
    with open(self.path) as f:
      return [json.loads(line) for line in f if line.strip()]

  def rewind(self, step: int):
    """Drops what a run wrote past the checkpoint it is resumed from: metrics after `step`
    updates, events at or after them (they happen again)."""
    if not self.path:
      return
    kept = [r for r in self.read() if r["step"] < step or (r["step"] == step and "event" not in r)]
    tmp = self.path + ".tmp-%d" % os.getpid()
    with open(tmp, "w") as f:
      for r in kept:
        f.write(json.dumps(r) + "\n")
    os.replace(tmp, self.path)

  def write(self, record: dict):
    if self.path:
      with open(self.path, "a") as f:
        f.write(json.dumps(record) + "\n")


def _start_quantisation(params, config):
  """train_inpt_spikingjelly.py:159-172, :329-338: a = c = init_fn(kernel) on every quantised
  layer, written into the leaves the optimiser already holds (its moments stay)."""
  from . import prune_utils
  new = prune_utils.update_quant_params(params, config.quant.init_fn, config.quant.bits)
  with torch.no_grad():
    for old, upd in zip(prune_utils._layers(params), prune_utils._layers(new)):
      for k in ("a", "c"):
        old["DuQ_0"][k].copy_(upd["DuQ_0"][k])


def _load_pretrained(path: str, config, device):
  """train_inpt_spikingjelly.py:144-230: the pretrained tree, then the prune masks and (at
  start_epoch == -1) the DuQ scalars from its kernels."""
  from . import prune_utils
  tree = checkpoint.load_torch_checkpoint(path) if path.endswith(".pth") \
      else checkpoint.load_flax_checkpoint(path)
  variables = nn.tree_from_numpy(tree, device)
  # with a prune schedule the loop prunes: no one-shot masks at load
  variables["params"] = prune_utils.prepare_params(variables["params"], config,
                                                   prune="prune_schedule" not in config.quant)
  logging.info("Successfully restored model from: %s", path)
  return variables


def _run(config, workdir: str, model, source, eval_source, device):
  if "online" in config:
    raise NotImplementedError("the online branch of train_step is not supported")
  from . import prune_utils
  scheduled = "prune_schedule" in config.get("quant", {})
  if scheduled:
    prune_utils.check_prune_schedule(config.quant)                  # refusals before anything is loaded
  world = int(os.environ.get("WORLD_SIZE", "1"))
  for size in (config.batch_size, config.eval_batch_size):        # train.py:96-98
    if size % world > 0:
      raise ValueError("Batch size (" + str(size) + ") must be divisible by "
                       "the number of devices (" + str(world) + ").")
  source = input_pipeline.load_source(config.dataset if source is None else source)
  if not (input_pipeline.is_event_source(source) or input_pipeline.is_image_source(source)):
    raise NotImplementedError("the training split needs an event source (addrs, times, offsets, "
                              "label, sensor_size); frame sources are eval only")
  if eval_source is None:
    eval_source = config.get("eval_dataset", None)
  eval_source = source if eval_source is None else input_pipeline.load_source(eval_source)

  rank, world, local = parallel.init_from_env(config.get("backend", None))
  if device is None:
    device = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
  device = torch.device(device)
  if device.type == "cuda":
    torch.cuda.set_device(device)

  steps_per_epoch = source["label"].shape[0] // config.batch_size   # train.py:112-127
  num_steps = int(steps_per_epoch * config.num_epochs) if config.get("num_train_steps", -1) == -1 \
      else int(config.num_train_steps)
  steps_per_eval = eval_source["label"].shape[0] // config.eval_batch_size \
      if config.get("steps_per_eval", -1) == -1 else int(config.steps_per_eval)
  steps_per_checkpoint = steps_per_epoch * int(config.get("checkpoint_every_epochs", 10))
  if steps_per_epoch < 1:
    raise ValueError("batch_size %d leaves no step in an epoch of %d samples"
                     % (config.batch_size, source["label"].shape[0]))

  if model is None:
    from . import models
    model = create_model(model_cls=getattr(models, config.model),
                         num_classes=config.num_classes, config=config)
  learning_rate_fn = create_learning_rate_fn(config, config.learning_rate, steps_per_epoch)

  if config.get("pretrained", None):
    variables = _load_pretrained(config.pretrained, config, device)
  else:
    key = torch.Generator()
    key.manual_seed(int(config.seed))
    if input_pipeline.is_image_source(source):                    # [1, T, K] or [1, T, H, W, 2]
      params, batch_stats = initialized(key, None, model, config.num_frames, device,
                                        input_shape=input_pipeline.image_input_shape(source, config))
    else:
      image_size = int(int(source["sensor_size"][-1]) // config.get("resolution_scale", 1))
      params, batch_stats = initialized(key, image_size, model, config.num_frames, device)
    variables = {"params": params, "batch_stats": batch_stats}
  state = create_train_state(variables, config, model)
  state = restore_checkpoint(state, workdir)
  step_offset = int(state.step)                                   # > 0 if restarting from a checkpoint
  info = {"eval": None, "best_accuracy": 0.0, "steps_per_epoch": steps_per_epoch}
  if step_offset >= num_steps:
    logging.info("Nothing to train: the checkpoint of %s is at step %d of %d", workdir, step_offset, num_steps)
    return state, info

  writer_train = _Records(os.path.join(workdir, "train", "metrics.jsonl"), rank == 0)
  writer_eval = _Records(os.path.join(workdir, "eval", "metrics.jsonl"), rank == 0)
  if step_offset > 0:
    writer_train.rewind(step_offset)
    writer_eval.rewind(step_offset)
  eval_best = max([r["accuracy"] for r in writer_eval.read() if r.get("best")] + [0.0])
  if parallel.dist.is_initialized():                              # rank 0 holds the records
    best = [eval_best]
    parallel.dist.broadcast_object_list(best, 0)
    eval_best = float(best[0])

  # Evaluation k (0: before training; e: after epoch e) reads batches [k, k + 1) * steps_per_eval
  # of the eval stream, in a resumed run as well: the iterator starts at the evaluation the
  # checkpoint's last finished epoch had, which the evaluation before training then repeats.
  evals_done = step_offset // steps_per_epoch
  cache = config.get("cache", True)
  train_iter = input_pipeline.create_input_iter(source, config, train=True, cache=cache, rank=rank,
                                                world=world, device=device, skip=step_offset)
  eval_iter = input_pipeline.create_input_iter(eval_source, config, train=False, cache=cache, rank=rank,
                                               world=world, device=device,
                                               skip=evals_done * steps_per_eval)

  loss_fn = config.get("loss_fn", mse_loss)
  smoothing = config.get("smoothing", 0.0)
  weight_decay = config.get("weight_decay", 0.0)
  q = config.get("quant", {})
  quant_step = q.start_epoch * steps_per_epoch if "start_epoch" in q else None
  quant_is_duq = "DuQ" in str(q.get("weight", ""))
  # Gradual pruning: a prune event is a function of the step and of the kernels and
  # masks alone, both checkpointed, so a resumed run repeats the events from its checkpoint on
  # (_Records.rewind) and continues bit for bit.  Every rank prunes its own, identical, copy.
  prune_sched = prune_utils.resolve_prune_schedule(q, steps_per_epoch) if scheduled else None

  def evaluate(step, epochs, record):
    summary, _, _ = eval_pass(state, eval_iter, steps_per_eval, config, world)
    summary = dict(step=step, epoch=epochs, **summary)
    # the epoch just finished is epochs - 1, counted from 0 as :405 counts it; under a prune
    # schedule a model that is not yet at the final sparsity must not win
    summary["best"] = bool(epochs > 0 and summary["accuracy"] > eval_best
                           and ("start_epoch" not in q or epochs - 1 > q.start_epoch)
                           and (prune_sched is None or step > prune_sched.t1))
    if record:
      writer_eval.write(summary)
    return summary

  summary = evaluate(step_offset, evals_done, record=step_offset == 0)   # train.py:243-256
  logging.info("Before training eval - loss: %.4f, accuracy: %.2f", summary["loss"], summary["accuracy"] * 100)
  info["eval"] = summary

  train_metrics = []
  last_t, last_step = time.time(), step_offset
  for step in range(step_offset, num_steps):
    if prune_sched is not None and prune_sched.is_event(step):
      sparsity = prune_utils.sparsity_at(step, prune_sched, q.prune_percentage)
      prune_utils.prune_event(state.params["params"], sparsity, q.get("prune_global", True) is not False)
      zeros, weights = prune_utils.mask_zeros(state.params["params"])
      zeros = int(zeros)                                            # the event's read, as a log point's
      logging.info("Prune event at step %d: sparsity %.4f, %d of %d weights pruned", step, sparsity, zeros, weights)
      writer_train.write({"step": step, "event": "prune", "sparsity": sparsity, "zeros": zeros, "weights": weights})
    if step == quant_step and quant_is_duq:
      logging.info("Quantization start.")
      _start_quantisation(state.params["params"], config)
      writer_train.write({"step": step, "event": "quant_start"})

    batch = next(train_iter)
    state, metrics = train_step(state, batch, step_rng(config.seed, rank, step), learning_rate_fn,
                                weight_decay, smoothing, loss_fn)

    if config.get("log_every_steps"):
      train_metrics.append((metrics["loss"].to(torch.float32), metrics["accuracy"].to(torch.float32).mean(),
                            float(metrics["learning_rate"])))
      if (step + 1) % config.log_every_steps == 0:
        mean = torch.stack([torch.stack([m[0] for m in train_metrics]).mean(),
                            torch.stack([m[1] for m in train_metrics]).mean()])
        loss, acc = parallel.all_gather_rows(mean[None]).mean(0).tolist()   # the log point's read
        now = time.time()
        writer_train.write({"step": step + 1, "loss": loss, "accuracy": acc,
                            "learning_rate": sum(m[2] for m in train_metrics) / len(train_metrics),
                            "steps_per_second": (step + 1 - last_step) / max(now - last_t, 1e-9)})
        train_metrics = []
        last_t, last_step = time.time(), step + 1

    if (step + 1) % steps_per_epoch == 0:
      epochs = (step + 1) // steps_per_epoch
      state = sync_batch_stats(state)
      summary = evaluate(step + 1, epochs, record=True)
      logging.info("eval epoch: %d, loss: %.4f, accuracy: %.2f", epochs, summary["loss"], summary["accuracy"] * 100)
      info["eval"] = summary
      if summary["best"]:
        save_checkpoint(state, os.path.join(workdir, "best"))
        logging.info("!!!! Saved new best model with accuracy %.4f", summary["accuracy"])
        eval_best = summary["accuracy"]

    if (step + 1) % steps_per_checkpoint == 0 or step + 1 == num_steps:
      state = sync_batch_stats(state)
      save_checkpoint(state, workdir)

  if device.type == "cuda":
    torch.cuda.synchronize()
  info["best_accuracy"] = eval_best
  logging.info("Best accuracy: %.4f", eval_best)
  return state, info


def train_and_evaluate(config, workdir: str, *, model=None, source=None, eval_source=None,
                       device=None) -> TrainState:
  """examples/train.py:70-338: trains `config.model` on the event or image source `config.dataset` (or
  `source`, an in-memory dict), evaluates on `config.eval_dataset` (or `eval_source`; default: the
  training source) before training and after every epoch, writes checkpoints and records under
  `workdir`, and continues from the newest checkpoint found there.  Returns the final state."""
  return _run(config, workdir, model, source, eval_source, device)[0]


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  ap.add_argument("--workdir", required=True, help="directory of the checkpoints and records")
  ap.add_argument("--config", required=True, help="Python file with get_config()")
  args = ap.parse_args(argv)
  logging.basicConfig(level=logging.INFO)
  try:
    _, info = _run(load_config(args.config), args.workdir, None, None, None, None)
    if int(os.environ.get("RANK", "0")) == 0:
      print(json.dumps({"eval": info["eval"], "best_accuracy": info["best_accuracy"]}))
  finally:
    if torch.distributed.is_available() and torch.distributed.is_initialized():
      torch.distributed.destroy_process_group()


if __name__ == "__main__":
  main()
