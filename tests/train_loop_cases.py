"""Fixtures of the training-loop tests (snnquantprune_amd/train.py): the learnable event sources, the
loop's config on the two-block ConvDenseSNN of tests/conv_train_reference.py, a toy TrainState for
the checkpoint tests that need no model, and the float64 replay that says whether the fixture can
be learnt at all.  Nothing here needs a GPU."""
import dataclasses
import types

import numpy as np
import torch

from tests import conv_train_reference as cr
from tests import event_cases as ec

F32, F64 = np.float32, np.float64
H = W = cr.HW                     # 8 x 8 sensor
T = cr.T_STEPS                    # 3 frames
N_TRAIN, N_TEST, BATCH = 16, 8, 4
EVENTS, T_HI = 240, 12000         # per recording: some 0.6 events per frame slot; 12 ms long
# The settings of "it learns".  The float64 reference (test_train_loop_cpu) takes its epoch-mean loss
# from 0.38 to 0.17 .. 0.20 with them, whatever the dropout draws (four mask seeds tried); at 2 epochs
# and learning rate 1e-2 it moved by 0.006 .. 0.04, no more than the masks' own noise.
LEARN = dict(num_epochs=4, learning_rate=0.1)


def make_source(seed, n):
  """`n` recordings of two classes: class c's events fall in half c of the sensor's columns."""
  rng = np.random.Generator(np.random.PCG64(seed))
  labels = np.arange(n) % cr.CLASSES
  samples = []
  for y in labels:
    addrs, times = ec.make_sample(rng, EVENTS, H, W, outside=False, t_hi=T_HI)
    addrs[:, 0] = addrs[:, 0] % (W // 2) + (W // 2) * y
    samples.append((addrs, times))
  return dict(ec.make_set(samples), label=labels.astype(np.int8), sensor_size=np.array([H, W]))


def sources():
  return make_source(1, N_TRAIN), make_source(2, N_TEST)


def make_config(split_by="number", **kw):
  """The loop's config: ConvDenseSNN (16 channels, 2 blocks, 4-bit, 90 % pruned, dropout 0.9), adam,
  2 epochs of 4 steps, a record per step and a checkpoint per epoch."""
  from snnquantprune_amd import synthetic as syn
  cfg = syn.make_config(bits=cr.BITS, prune_percentage=0.9, channels=cr.CHANNELS, tau=cr.TAU,
                        num_conv_blocks=cr.NBLOCKS, dropout=cr.KEEP)
  cfg.model, cfg.num_classes, cfg.num_frames, cfg.split_by = "ConvDenseSNN", cr.CLASSES, T, split_by
  cfg.time_step, cfg.input_scale, cfg.train_chunk_size, cfg.test_chunk_size = 1, 1, 3, 3
  cfg.batch_size, cfg.eval_batch_size, cfg.feed_format, cfg.seed = BATCH, BATCH, "u8", 5
  cfg.optimizer, cfg.learning_rate, cfg.weight_decay, cfg.smoothing = "adam", 1e-2, 0.0, 0.0
  cfg.num_epochs, cfg.warmup_epochs, cfg.num_train_steps, cfg.steps_per_eval = 2, 1, -1, -1
  cfg.log_every_steps, cfg.checkpoint_every_epochs = 1, 1
  for k, v in kw.items():
    if k.startswith("quant_"):
      cfg.quant[k[len("quant_"):]] = v
    else:
      cfg[k] = v
  return cfg


def pretrained_tree(masks=False):
  """Weights that fire (tests/test_conv_train_reference_cpu.py): the fixture of
  conv_train_reference, as a checkpoint holds them before pruning -- no DuQ scalars, and no masks
  unless asked for."""
  v, _ = cr.fixture(True)
  params = {}
  for name, leaf in v["params"].items():
    params[name] = {k: t for k, t in leaf.items() if k in ("kernel", "scale", "bias") or (masks and k == "prune_0")}
  return {"params": params, "batch_stats": v["batch_stats"]}


def write_flax_file(path, tree):
  from snnquantprune_amd import checkpoint
  with open(path, "wb") as f:
    f.write(checkpoint.msgpack_serialize({"step": 0, "params": {"params": tree["params"]},
                                          "batch_stats": tree["batch_stats"]}))
  return path


def host_batches(source, cfg, steps, train=True):
  """The first `steps` batches of the split as the loop's plan draws them, decoded on the host
  (event_cases): [(counts uint8 [B, T, H, W, 2], labels)]."""
  from snnquantprune_amd import input_pipeline as ip
  n = source["label"].shape[0]
  plan = ip.EventPlan(cfg, source["sensor_size"], n, train)
  off = source["offsets"]
  t_min = np.array([source["times"][off[i]] for i in range(n)], np.int64)
  t_max = np.array([source["times"][off[i + 1] - 1] for i in range(n)], np.int64)
  it = plan.batches(t_min, t_max)
  out = []
  for _ in range(steps):
    idx, starts = next(it)
    x = ec.decode_batch(source, idx, T, H, W, plan.split_by, starts, plan.step_us)
    out.append((np.minimum(x, 255).astype(np.uint8), source["label"][idx].astype(np.int64)))
  return out


# ---- a TrainState without a model ----------------------------------------------------------------

def toy_state(optimizer="adam", seed=0, **kw):
  """A TrainState over a small CPU tree: a quantised layer (kernel, DuQ, mask) and a BatchNorm."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import train_utils as tu
  g = torch.Generator()
  g.manual_seed(seed)
  r = lambda *s: torch.randn(*s, generator=g)                        # noqa: E731
  params = {"QuantDense_0": {"kernel": r(4, 3), "DuQ_0": {"a": r(1).abs() + 1, "c": r(1).abs() + 1},
                             "prune_0": {"mask": (r(4, 3) > -0.5).to(torch.float32)}},
            "BatchNorm_0": {"scale": r(3), "bias": r(3)}}
  stats = {"BatchNorm_0": {"mean": r(3), "var": r(3).abs() + 0.5}}
  cfg = nn.ConfigDict(optimizer=optimizer, **kw)
  return tu.create_train_state({"params": params, "batch_stats": stats}, cfg, types.SimpleNamespace(apply=None))


def toy_step(state, lr=0.01):
  """One update with made-up gradients, a function of the step and the leaf's place alone; the
  running statistics move too."""
  from snnquantprune_amd import train_utils as tu
  with torch.no_grad():
    for i, (_, p) in enumerate(tu._flatten(state.params["params"])):
      g = torch.Generator()
      g.manual_seed(1000 * state.step + i)
      p.grad = torch.randn(p.shape, generator=g)
    for group in state.tx.param_groups:
      group["lr"] = lr
    state.tx.step()
    for _, p in tu._flatten(state.params["params"]):
      p.grad = None
    stats = {k: {n: t * 0.9 + 0.1 * (state.step + 1) for n, t in s.items()} for k, s in state.batch_stats.items()}
  return dataclasses.replace(state, step=state.step + 1, batch_stats=stats)


def state_arrays(state):
  """Every tensor a checkpoint has to carry, by name: parameters, statistics and optimiser moments."""
  from snnquantprune_amd import train_utils as tu
  out = {"step": np.array(state.step)}
  for path, p in tu._flatten(state.params["params"]):
    out["params/" + "/".join(path)] = p.detach().cpu().numpy().copy()
    for k, v in state.tx.state.get(p, {}).items():
      if v is not None:
        out["opt/%s/%s" % (k, "/".join(path))] = torch.as_tensor(v).detach().cpu().numpy().copy()
  for path, p in tu._flatten(state.batch_stats):
    out["stats/" + "/".join(path)] = p.detach().cpu().numpy().copy()
  return out


# ---- can the fixture be learnt?  The float64 model, stepped with the loop's batches and Adam -----

def reference_losses(variables, batches, lr_fn, keep=cr.KEEP, seed=3):
  """Loss per step of TorchConvDenseSNN64 trained on `batches` with Adam (b1 0.9, b2 0.999, eps 1e-8, written
  out in float64) at lr_fn(step).  The spikes it replays are the oracle's float32 forward of the current weights on
  batch statistics; the read-out's dropout masks are draws of its own with the same keep
  probability (the device generator's cannot be drawn here)."""
  from snnquantprune_amd import train_utils as tu
  params = {k: {n: (dict(t) if isinstance(t, dict) else np.array(t, F32)) for n, t in leaf.items()}
            for k, leaf in variables["params"].items()}
  rng = np.random.default_rng(seed)
  moments, losses = None, []
  for step, (x, y) in enumerate(batches):
    B = x.shape[0]
    K = (H >> cr.NBLOCKS) * (W >> cr.NBLOCKS) * cr.CHANNELS
    mask = (rng.random((T, B, K)) < keep).astype(F32)
    fwd = cr.oracle_forward(params, x, mask, True)
    saved = {"hd": fwd["hd"], "sd": fwd["sd"]}
    for i in range(cr.NBLOCKS):
      saved["h%d" % i], saved["s%d" % i] = fwd["h%d" % i], fwd["s%d" % i]
    m = cr.TorchConvDenseSNN64(params)
    loss = tu.mse_loss(m.forward(x, mask, saved), y)
    loss.backward()
    losses.append(float(loss.detach()))
    # Adam in float64 on (layer, name) leaves, written back as the float32 the next forward reads
    grads = m.grads()
    if moments is None:
      moments = {k: (np.zeros_like(g), np.zeros_like(g)) for k, g in grads.items()}
    lr, t = lr_fn(step), step + 1
    for (layer, name), g in grads.items():
      mu, nu = moments[(layer, name)]
      mu[...] = 0.9 * mu + 0.1 * g
      nu[...] = 0.999 * nu + 0.001 * g * g
      upd = lr * (mu / (1 - 0.9 ** t)) / (np.sqrt(nu / (1 - 0.999 ** t)) + 1e-8)
      leaf = params[layer] if name in ("kernel", "scale", "bias") else params[layer]["DuQ_0"]
      leaf[name] = (np.asarray(leaf[name], F64) - upd.reshape(np.shape(leaf[name]))).astype(F32)
  return losses
