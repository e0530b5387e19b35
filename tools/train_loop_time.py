"""Times the training loop (snnquantprune_amd/train.py) against the two launches it is made of, on
the shapes of `tools/train_step_time.py --conv`: ConvDenseSNN at the C3 topology (three conv blocks
of 128 channels on 128 x 128 x 2 frames, 4-bit DuQ, 90 % pruned, B = 2, T = 20, Adam), fed from a
synthetic event source whose recordings bin to those frames (split_by = "number", uniformly random
events, 0.3 per frame slot).  In one process, --reps times each:

  loop         train_and_evaluate over --warmup steps, then resumed for --steps more with one record
               at the end: ms per step from the record's own steps_per_second
  train_step   the bare train_utils.train_step on the same batches (taken from the same iterator
               beforehand), wall clock around --steps calls and a synchronize
  events_bin   the iterator's next() alone, the same way

Then the loop once more with a record (a device-to-host read) after every step, each step's time
from its own record: whether a difference sits in one step.  Prints one JSON line.  The loop
should cost the sum of the other two and no more than the step's run-to-run spread (DESIGN.md
11.5, 14.5).

  python tools/train_loop_time.py [--steps 10] [--warmup 3] [--batch 2] [--frames 20] [--hw 128] [--reps 3]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_source(n, events, hw, classes, seed):
  rng = np.random.Generator(np.random.PCG64(seed))
  addrs = np.stack([rng.integers(0, hw, n * events), rng.integers(0, hw, n * events),
                    rng.integers(0, 2, n * events)], 1)
  times = np.sort(rng.integers(0, 20000, (n, events)), axis=1).reshape(-1)
  return {"addrs": addrs, "times": times, "offsets": np.arange(n + 1, dtype=np.int64) * events,
          "label": (np.arange(n) % classes).astype(np.int8), "sensor_size": np.array([hw, hw])}


def _wall(fn, steps):
  torch.cuda.synchronize()
  t0 = time.time()
  for _ in range(steps):
    fn()
  torch.cuda.synchronize()
  return (time.time() - t0) / steps * 1e3


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--batch", type=int, default=2)
  ap.add_argument("--frames", type=int, default=20)
  ap.add_argument("--hw", type=int, default=128)
  ap.add_argument("--reps", type=int, default=3)
  args = ap.parse_args(argv)
  assert torch.cuda.is_available(), "train_loop_time.py needs the GPU"
  from snnquantprune_amd import checkpoint, input_pipeline, models, synthetic as syn
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import prune_utils, train, train_utils as tu
  dev = torch.device("cuda:0")
  B, T, HW, C, NB = args.batch, args.frames, args.hw, 128, 3
  total = args.warmup + args.steps
  events = int(0.3 * T * HW * HW * 2)
  src = event_source(B * (total + 1), events, HW, 11, 941)          # one epoch holds the whole run
  test = event_source(B, events, HW, 11, 942)

  work = tempfile.mkdtemp(prefix="train_loop_time_")
  try:
    v = syn.conv_net_variables(C, 2, NB, HW, 110, True, 0.9)
    pretrained = os.path.join(work, "pretrained_0")
    with open(pretrained, "wb") as f:
      f.write(checkpoint.msgpack_serialize({"step": 0, "params": {"params": v["params"]},
                                            "batch_stats": v["batch_stats"]}))
    cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=C, dropout=0.9)
    cfg.model, cfg.num_frames, cfg.split_by, cfg.feed_format = "ConvDenseSNN", T, "number", "u8"
    cfg.batch_size, cfg.eval_batch_size, cfg.steps_per_eval = B, B, 1
    cfg.optimizer, cfg.learning_rate, cfg.weight_decay = "adam", 1e-4, 0.0
    cfg.num_epochs, cfg.warmup_epochs, cfg.checkpoint_every_epochs = 1, 0, 1
    cfg.pretrained = pretrained
    model = models.ConvDenseSNN(num_classes=11, config=cfg)

    loop_ms, step_ms, bin_ms = [], [], []
    for rep in range(args.reps):
      # the loop: warm-up steps, then the timed ones as a resumed run whose one record covers them
      workdir = os.path.join(work, "run%d" % rep)
      cfg.num_train_steps, cfg.log_every_steps = args.warmup, 0
      train.train_and_evaluate(cfg, workdir, model=model, source=src, eval_source=test, device=dev)
      cfg.num_train_steps, cfg.log_every_steps = total, total
      train.train_and_evaluate(cfg, workdir, model=model, source=src, eval_source=test, device=dev)
      with open(os.path.join(workdir, "train", "metrics.jsonl")) as f:
        rec = [json.loads(line) for line in f]
      assert len(rec) == 1 and rec[0]["step"] == total, rec
      loop_ms.append(1e3 / rec[0]["steps_per_second"])

      # the bare step on the same batches, from the same start
      variables = nn.tree_from_numpy(checkpoint.load_flax_checkpoint(pretrained), dev)
      variables["params"] = prune_utils.prepare_params(variables["params"], cfg)
      box = [tu.create_train_state(variables, cfg, model)]
      it = input_pipeline.create_input_iter(src, cfg, train=True, cache=True, device=dev)
      batches = [next(it) for _ in range(total)]
      lr = tu.create_learning_rate_fn(cfg, cfg.learning_rate, len(src["label"]) // B)

      def step():
        s = box[0]
        box[0], _ = tu.train_step(s, batches[s.step], train.step_rng(cfg.seed, 0, s.step), lr, 0.0, 0.0, tu.mse_loss)

      _wall(step, args.warmup)
      step_ms.append(_wall(step, args.steps))
      _wall(lambda: next(it), args.warmup)
      bin_ms.append(_wall(lambda: next(it), args.steps))
      shutil.rmtree(workdir)

    # where a difference sits: the same resumed run with a record (and so a host read) per step
    workdir = os.path.join(work, "per_step")
    cfg.num_train_steps, cfg.log_every_steps = args.warmup, 0
    train.train_and_evaluate(cfg, workdir, model=model, source=src, eval_source=test, device=dev)
    cfg.num_train_steps, cfg.log_every_steps = total, 1
    train.train_and_evaluate(cfg, workdir, model=model, source=src, eval_source=test, device=dev)
    with open(os.path.join(workdir, "train", "metrics.jsonl")) as f:
      per_step = [round(1e3 / json.loads(line)["steps_per_second"], 3) for line in f]
    print(json.dumps({"tool": "train_loop_time", "batch": B, "frames": T, "hw": HW, "events_per_sample": events,
                      "steps": args.steps, "warmup": args.warmup,
                      "loop_ms_per_step": [round(t, 3) for t in loop_ms],
                      "train_step_ms": [round(t, 3) for t in step_ms],
                      "events_bin_ms": [round(t, 4) for t in bin_ms],
                      "loop_minus_parts_ms": [round(a - b - c, 3) for a, b, c in zip(loop_ms, step_ms, bin_ms)],
                      "loop_ms_each_step_with_a_record_per_step": per_step}))
  finally:
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
  main()
