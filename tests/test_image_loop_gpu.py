"""Image sources through the input pipeline, train.train_and_evaluate and the eval harness on the
GPU, on the fixture of tests/encode_cases.py (8 x 8 images of two classes, DenseSNN with 32 hidden
units, T = 8, 64 training images in batches of 16: 4 steps an epoch): the iterator against the
reference encoding, that the loop learns, that an interrupted run ends at the same bits, that an
evaluation repeats itself, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import encode_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = ec.N_TRAIN // ec.BATCH          # steps per epoch


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
  return tmp_path_factory.mktemp("image_loop")


_src = {}


def _sources():
  if not _src:
    _src["train"], _src["test"] = ec.sources()
  return _src["train"], _src["test"]


_done = {}


def _train(dev, root, name, stages, **cfg_kw):
  """One workdir per name, trained once: train_and_evaluate per stage, each stage a dict of config
  keys laid over cfg_kw (an interrupted run is two stages) -> (workdir, final state, last config)."""
  if name not in _done:
    from snnquantprune_amd import train
    workdir = str(root / name)
    src, test = _sources()
    for stage in stages:
      cfg = ec.make_config(**dict(cfg_kw, **stage))
      state = train.train_and_evaluate(cfg, workdir, source=src, eval_source=test, device=dev)
    _done[name] = (workdir, state, cfg)
  return _done[name]


def _records(workdir, which):
  with open(os.path.join(workdir, which, "metrics.jsonl")) as f:
    return [json.loads(line) for line in f]


def _ckpt(path):
  from snnquantprune_amd import checkpoint
  from snnquantprune_amd import train_utils as tu
  with open(path, "rb") as f:
    return {"/".join(p): v for p, v in tu._flatten(checkpoint.msgpack_restore(f.read()))}


# ---- 1. the iterator against the reference -----------------------------------------------------------

@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_iterator_matches_reference(dev, train, rank, world):
  from snnquantprune_amd import input_pipeline as ip
  src = _sources()[0]
  cfg = ec.make_config()
  steps = 2 * (ec.N_TRAIN // ec.BATCH) + 1                   # into the third pass of the rank's slice
  want = ec.plan_batches(src, cfg, steps, train, rank, world)
  it = ip.create_input_iter(src, cfg, train=train, cache=True, rank=rank, world=world, device=dev)
  draws = []
  for x, y, idx, draw in want:
    b = next(it)
    assert b["dvs_matrix"].dtype == torch.uint8 and b["dvs_matrix"].is_cuda and b["label"].dtype == torch.int8
    assert tuple(b["dvs_matrix"].shape) == (ec.BATCH // world, ec.T_STEPS, ec.SIDE * ec.SIDE)
    np.testing.assert_array_equal(b["dvs_matrix"].cpu().numpy(), x)
    np.testing.assert_array_equal(b["label"].cpu().numpy(), y)
    draws.append(draw)
  assert draws == ([1] * 4 + [2] * 4 + [3] if train else [0] * 9)
  # a resumed run: from the sixth batch on, nothing launched for the five skipped
  it = ip.create_input_iter(src, cfg, train=train, cache=True, rank=rank, world=world, device=dev, skip=5)
  for x, y, _, _ in want[5:8]:
    b = next(it)
    np.testing.assert_array_equal(b["dvs_matrix"].cpu().numpy(), x)
    np.testing.assert_array_equal(b["label"].cpu().numpy(), y)


def test_frames_layout_and_bits_feed(dev):
  from snnquantprune_amd import input_pipeline as ip
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  src = _sources()[1]
  cfg = ec.make_config()
  flat = next(ip.create_input_iter(src, cfg, train=False, cache=True, device=dev))
  # the same bytes seen as [B, T, H, W, 2]
  as_frames = dict(src, image=src["image"].reshape(ec.N_TEST, ec.SIDE, ec.SIDE // 2, 2))
  fr = next(ip.create_input_iter(as_frames, ec.make_config(image_layout="frames"), train=False, cache=True, device=dev))
  assert tuple(fr["dvs_matrix"].shape) == (ec.BATCH, ec.T_STEPS, ec.SIDE, ec.SIDE // 2, 2)
  assert fr["dvs_matrix"].is_contiguous()
  assert torch.equal(fr["dvs_matrix"].reshape(ec.BATCH, ec.T_STEPS, -1), flat["dvs_matrix"])
  assert torch.equal(fr["label"], flat["label"])
  # bits: batch-major PackedSpikes of the uint8 batch
  bern = nn.ConfigDict(kind="bernoulli", gain=0.8)
  u8 = next(ip.create_input_iter(src, ec.make_config(encoding=bern), train=False, cache=True, device=dev))
  packed = next(ip.create_input_iter(src, ec.make_config(encoding=bern, feed_format="bits"), train=False,
                                     cache=True, device=dev))
  x = packed["dvs_matrix"]
  assert isinstance(x, ops.PackedSpikes) and x.shape == (ec.BATCH, ec.T_STEPS, ec.SIDE * ec.SIDE)
  assert torch.equal(x.bits, ops.pack_bits(u8["dvs_matrix"]).bits)
  with pytest.raises(ValueError, match="the training split needs feed_format 'u8'"):
    ip.create_input_iter(src, ec.make_config(encoding=bern, feed_format="bits"), train=True, cache=True, device=dev)


# ---- 2. the loop runs, and learns --------------------------------------------------------------------

def _whole(dev, root):
  return _train(dev, root, "whole", [{}])


def test_fixture_can_be_learnt_from_the_loops_own_start(dev):
  """Established first, without the kernels under test: the float64 model of tests/train_reference.py
  on the batches the loop will draw (encoded by the reference), from the weights the loop starts
  from, takes the epoch-mean loss down."""
  from snnquantprune_amd import models
  from snnquantprune_amd import train_utils as tu
  from snnquantprune_amd.eval import initialized
  cfg = ec.make_config()
  model = tu.create_model(model_cls=models.DenseSNN, num_classes=cfg.num_classes, config=cfg)
  key = torch.Generator()
  key.manual_seed(int(cfg.seed))
  params, _ = initialized(key, None, model, cfg.num_frames, dev, input_shape=(1, ec.T_STEPS, ec.SIDE * ec.SIDE))
  tree = {name: {"kernel": leaf["kernel"].cpu().numpy(),
                 "DuQ_0": {k: v.cpu().numpy() for k, v in leaf["DuQ_0"].items()}}
          for name, leaf in params.items()}
  assert tree["QuantDense_0"]["kernel"].shape == (ec.SIDE * ec.SIDE, ec.HIDDEN)
  batches = [(x, y) for x, y, _, _ in ec.plan_batches(_sources()[0], cfg, S * cfg.num_epochs, train=True)]
  losses = ec.reference_losses(tree, batches, tu.create_learning_rate_fn(cfg, cfg.learning_rate, S))
  first, last = np.mean(losses[:S]), np.mean(losses[-S:])
  print("reference losses", [round(l, 4) for l in losses], "first epoch", first, "last epoch", last)
  assert np.isfinite(losses).all() and last < first


def test_loop_runs_and_learns(dev, root):
  workdir, state, cfg = _whole(dev, root)
  assert state.step == 3 * S == 12
  assert sorted(f for f in os.listdir(workdir) if f.startswith("checkpoint")) == [
      "checkpoint_12", "checkpoint_4", "checkpoint_8"]
  ev = _records(workdir, "eval")
  assert [(r["step"], r["epoch"]) for r in ev] == [(0, 0), (4, 1), (8, 2), (12, 3)]
  assert all(r["samples"] == ec.N_TEST and r["steps"] == 2 for r in ev)
  loss = [r["loss"] for r in _records(workdir, "train")]
  assert len(loss) == 3 * S
  first, last = np.mean(loss[:S]), np.mean(loss[-S:])
  print("eval records", ev)
  print("training losses", loss, "first epoch", first, "last epoch", last)
  assert np.isfinite(loss).all() and last < first
  assert ev[-1]["loss"] < ev[0]["loss"]


# ---- 3. an interrupted run ends at the same bits -----------------------------------------------------

def test_resume_is_exact(dev, root):
  """Stopped after epoch 1 (4 of 12 steps) and continued in the same workdir."""
  a, state_a, _ = _whole(dev, root)
  b, state_b, _ = _train(dev, root, "resumed", [dict(num_train_steps=S), dict(num_train_steps=-1)])
  assert state_a.step == state_b.step == 12
  got, want = _ckpt(os.path.join(b, "checkpoint_12")), _ckpt(os.path.join(a, "checkpoint_12"))
  assert set(got) == set(want)
  assert any(k.startswith("opt_state/0/nu/") for k in want) and any(k.startswith("params/") for k in want)
  for k, v in want.items():
    np.testing.assert_array_equal(got[k], v, err_msg=k)
  ea, eb = _records(a, "eval"), _records(b, "eval")
  assert len(ea) == 4 and eb[-4:] == ea
  strip = lambda rs: [{k: v for k, v in r.items() if k != "steps_per_second"} for r in rs]   # noqa: E731
  assert strip(_records(b, "train")) == strip(_records(a, "train"))
  # the records are worth comparing: the numbers move after the interruption
  assert len({r["loss"] for r in _records(a, "train")[S:]}) > S and len({r["loss"] for r in ea}) >= 3


# ---- 4. an evaluation repeats itself, and is the loop's ----------------------------------------------

def test_eval_is_reproducible_and_the_loops(dev, root):
  from snnquantprune_amd import eval as ev
  workdir, _, cfg = _whole(dev, root)
  test = _sources()[1]
  _, s1, p1 = ev.evaluate_metrics(cfg, workdir, source=test, device=dev)
  _, s2, p2 = ev.evaluate_metrics(cfg, workdir, source=test, device=dev)
  assert torch.equal(p1["loss"], p2["loss"]) and torch.equal(p1["accuracy"], p2["accuracy"])
  assert p1["loss"].numel() == 2 and p1["accuracy"].numel() == ec.N_TEST
  last = _records(workdir, "eval")[-1]
  assert (s1["loss"], s1["accuracy"], s1["samples"]) == (last["loss"], last["accuracy"], last["samples"])
  assert s1 == s2
  # without a checkpoint: the model is initialised from the image source's [1, T, K]
  _, s0, _ = ev.evaluate_metrics(cfg, str(root / "nothing-here"), source=test, device=dev)
  assert s0["samples"] == ec.N_TEST and s0["loss"] == _records(workdir, "eval")[0]["loss"]


# ---- 5. the command line ---------------------------------------------------------------------------------

def test_cli(dev, root, capsys):
  """`-m snnquantprune_amd.train` (its main(), in this process) on image .npz files, then
  `-m snnquantprune_amd.eval` as a command on the checkpoint it wrote."""
  from snnquantprune_amd import train
  work = root / "cli"
  work.mkdir()
  src, test = _sources()
  np.savez(str(work / "images.npz"), **src)
  np.savez(str(work / "test.npz"), **test)
  for name, dataset in (("train_config.py", "images.npz"), ("eval_config.py", "test.npz")):
    (work / name).write_text(
        "from tests import encode_cases as ec\n\n\n"
        "def get_config():\n"
        "  return ec.make_config(num_epochs=1, dataset=%r, eval_dataset=%r)\n"
        % (str(work / dataset), str(work / "test.npz")))
  capsys.readouterr()
  train.main(["--config", str(work / "train_config.py"), "--workdir", str(work / "run")])
  lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
  assert len(lines) == 1, lines
  result = json.loads(lines[0])
  assert result["eval"]["step"] == S and result["eval"]["epoch"] == 1
  assert result["eval"] == _records(str(work / "run"), "eval")[-1]
  assert os.path.isfile(work / "run" / ("checkpoint_%d" % S))

  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  out = subprocess.run([sys.executable, "-m", "snnquantprune_amd.eval", "--config", str(work / "eval_config.py"),
                        "--workdir", str(work / "run")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
  assert out.returncode == 0, out.stderr[-4000:]
  lines = [l for l in out.stdout.splitlines() if l.strip()]
  assert len(lines) == 1, out.stdout
  summary = json.loads(lines[0])
  last = result["eval"]
  assert (summary["loss"], summary["accuracy"], summary["samples"], summary["steps"]) == (
      last["loss"], last["accuracy"], last["samples"], last["steps"])
