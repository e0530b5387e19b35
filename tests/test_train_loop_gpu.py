"""train.train_and_evaluate on the GPU, on the fixture of tests/train_loop_cases.py (two-block
ConvDenseSNN, 8 x 8 sensor, 3 frames, 16 training recordings in batches of 4: 4 steps an epoch):
what a run leaves behind, that an interrupted run ends at the same bits, that the loop's evaluation
is eval.evaluate's, the quantisation start, pretrained + prune, that it learns, and the CLI."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import train_loop_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = lc.N_TRAIN // lc.BATCH          # steps per epoch


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
  return tmp_path_factory.mktemp("train_loop")


_src = {}


def _sources():
  if not _src:
    _src["train"], _src["test"] = lc.sources()
  return _src["train"], _src["test"]


_done = {}


def _train(dev, root, name, stages, **cfg_kw):
  """One workdir per name, trained once (nothing modifies it afterwards): train_and_evaluate per
  stage, each stage a dict of config keys laid over cfg_kw (an interrupted run is two stages).
  -> (workdir, final state, config of the last stage)."""
  if name not in _done:
    from snnquantprune_amd import train
    workdir = str(root / name)
    src, test = _sources()
    for stage in stages:
      cfg = lc.make_config(**dict(cfg_kw, **stage))
      state = train.train_and_evaluate(cfg, workdir, source=src, eval_source=test, device=dev)
    _done[name] = (workdir, state, cfg)
  return _done[name]


def _records(workdir, which):
  with open(os.path.join(workdir, which, "metrics.jsonl")) as f:
    return [json.loads(line) for line in f]


def _ckpt(path):
  """{path: leaf} of a checkpoint file, every leaf of the TrainState tree."""
  from snnquantprune_amd import checkpoint
  from snnquantprune_amd import train_utils as tu
  with open(path, "rb") as f:
    return {"/".join(p): v for p, v in tu._flatten(checkpoint.msgpack_restore(f.read()))}


def _assert_same_checkpoint(got, want):
  assert set(got) == set(want)
  assert any(k.startswith("opt_state/0/nu/") for k in want) and any(k.startswith("batch_stats/") for k in want)
  for k, v in want.items():
    np.testing.assert_array_equal(got[k], v, err_msg=k)


def _pretrained(root):
  path = str(root / "pretrained_0")
  return path if os.path.exists(path) else lc.write_flax_file(path, lc.pretrained_tree())


def _fires(root, **kw):
  """Config keys of a run whose numbers move: it starts from weights that fire, pruned and quantised
  on loading, at the learning rate of "it learns".  (From model.init the read-out of this small net
  stays silent for the first steps: logits 0 and loss 0.5 whatever the batch, which would let a
  resumed run's records agree for free.)"""
  return dict(pretrained=_pretrained(root), learning_rate=lc.LEARN["learning_rate"], **kw)


def _whole(dev, root, split_by="number", **kw):
  return _train(dev, root, "whole-" + split_by, [{}], split_by=split_by, **_fires(root, **kw))


# ---- 1. what a run leaves behind --------------------------------------------------------------------

def test_end_to_end(dev, root):
  from snnquantprune_amd import train_utils as tu
  workdir, state, cfg = _train(dev, root, "from-init", [{}])         # model.init with config.seed
  assert state.step == 2 * S == 8
  assert sorted(f for f in os.listdir(workdir) if f.startswith("checkpoint")) == ["checkpoint_4", "checkpoint_8"]
  rec = _records(workdir, "train")
  lr = tu.create_learning_rate_fn(cfg, cfg.learning_rate, S)
  assert [r["step"] for r in rec] == list(range(1, 9))
  assert [r["learning_rate"] for r in rec] == [lr(s) for s in range(8)]
  assert all(np.isfinite(r["loss"]) and 0 <= r["accuracy"] <= 1 and r["steps_per_second"] > 0 for r in rec)
  ev = _records(workdir, "eval")
  assert [(r["step"], r["epoch"]) for r in ev] == [(0, 0), (4, 1), (8, 2)]
  assert all(r["samples"] == lc.N_TEST and r["steps"] == 2 for r in ev)
  print("eval records", ev)
  beat = any(r["accuracy"] > 0 for r in ev[1:])
  best = os.path.join(workdir, "best")
  assert (os.path.isdir(best) and len(os.listdir(best)) > 0) == beat
  if beat:
    assert [r["best"] for r in ev].count(True) == len(os.listdir(best)) <= 2
  # the final checkpoint is the state that was returned
  got = _ckpt(os.path.join(workdir, "checkpoint_8"))
  assert got["step"] == 8 and got["opt_state/0/count"] == 8
  for path, p in tu._flatten(state.params["params"]):
    np.testing.assert_array_equal(got["params/params/" + "/".join(path)], p.cpu().numpy())


# ---- 2. an interrupted run ends at the same bits ----------------------------------------------------

@pytest.mark.parametrize("split_by,kw", [("number", {}), ("time", dict(steps_per_eval=1))], ids=["number", "time"])
def test_resume_is_exact(dev, root, split_by, kw):
  """Stopped after 5 of 8 steps (inside the second epoch) and continued in the same workdir.  In the
  time case an evaluation is half a pass of the test split, so the resumed run also has to find its
  place in the eval stream."""
  a, state_a, _ = _whole(dev, root, split_by, **kw)
  b, state_b, _ = _train(dev, root, "resumed-" + split_by, [dict(num_train_steps=5), dict(num_train_steps=-1)],
                         split_by=split_by, **_fires(root, **kw))
  assert state_a.step == state_b.step == 8
  _assert_same_checkpoint(_ckpt(os.path.join(b, "checkpoint_8")), _ckpt(os.path.join(a, "checkpoint_8")))
  ea, eb = _records(a, "eval"), _records(b, "eval")
  assert len(ea) == 3 and eb[-3:] == ea
  ta, tb = _records(a, "train"), _records(b, "train")
  strip = lambda rs: [{k: v for k, v in r.items() if k != "steps_per_second"} for r in rs]   # noqa: E731
  assert strip(tb) == strip(ta)
  # the records are worth comparing: the loss moves from step to step and from evaluation to evaluation
  assert len({r["loss"] for r in ta}) == 8 and len({r["loss"] for r in ea}) == 3


# ---- 3. the loop's evaluation is evaluate's ---------------------------------------------------------

def test_loop_eval_is_evaluate(dev, root):
  from snnquantprune_amd import eval as ev
  workdir, _, cfg = _whole(dev, root)
  _, summary, _ = ev.evaluate_metrics(cfg, workdir, source=_sources()[1], device=dev)
  last = _records(workdir, "eval")[-1]
  assert (summary["loss"], summary["accuracy"]) == (last["loss"], last["accuracy"])
  assert summary["samples"] == last["samples"] == lc.N_TEST


# ---- 4. the quantisation start ----------------------------------------------------------------------

def _quant_layers(ck):
  return sorted(k[:-len("/DuQ_0/a")] for k in ck if k.startswith("params/") and k.endswith("/DuQ_0/a"))


def test_quantisation_starts_once_at_its_epoch(dev, root):
  from snnquantprune_amd import checkpoint, input_pipeline, models, prune_utils
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import train, train_utils as tu
  # the reference's workflow: pretrained weights, pruned on loading, a = c = -1 until the start epoch
  workdir, _, cfg = _train(dev, root, "quant-start", [{}], **_fires(root, quant_start_epoch=1))
  c4, c8 = _ckpt(os.path.join(workdir, "checkpoint_4")), _ckpt(os.path.join(workdir, "checkpoint_8"))
  layers = _quant_layers(c4)
  assert len(layers) == 3
  for l in layers:
    assert c4[l + "/DuQ_0/a"] == -1 and c4[l + "/DuQ_0/c"] == -1
    assert c8[l + "/DuQ_0/a"] > 0 and c8[l + "/DuQ_0/c"] > 0
  assert [r for r in _records(workdir, "train") if "event" in r] == [{"step": 4, "event": "quant_start"}]

  # replay: checkpoint_4, the switch by hand, four steps with the loop's batches and seeds
  replay = str(root / "quant-replay")
  os.makedirs(replay)
  shutil.copy(os.path.join(workdir, "checkpoint_4"), replay)
  model = models.ConvDenseSNN(num_classes=cfg.num_classes, config=cfg)
  variables = nn.tree_from_numpy(checkpoint.load_flax_checkpoint(os.path.join(replay, "checkpoint_4")), dev)
  variables = nn.tree_map(torch.zeros_like, variables)               # (the restore has to fill them)
  state = tu.restore_checkpoint(tu.create_train_state(variables, cfg, model), replay)
  assert state.step == 4
  new = prune_utils.update_quant_params(state.params["params"], cfg.quant.init_fn, cfg.quant.bits)
  for name, leaf in state.params["params"].items():
    if "kernel" in leaf:
      for k in ("a", "c"):
        leaf["DuQ_0"][k].copy_(new[name]["DuQ_0"][k])
  it = input_pipeline.create_input_iter(_sources()[0], cfg, train=True, cache=True, device=dev, skip=4)
  lr = tu.create_learning_rate_fn(cfg, cfg.learning_rate, S)
  for step in range(4, 8):
    state, _ = tu.train_step(state, next(it), train.step_rng(cfg.seed, 0, step), lr, cfg.weight_decay,
                             cfg.smoothing, tu.mse_loss)
  got = {"/".join(p): v for p, v in tu._flatten(tu.state_dict(state))}
  _assert_same_checkpoint(got, c8)

  # and a run resumed after the switch does not switch again
  resumed, _, _ = _train(dev, root, "quant-resumed", [dict(num_train_steps=6), dict(num_train_steps=-1)],
                         **_fires(root, quant_start_epoch=1))
  assert os.path.exists(os.path.join(resumed, "checkpoint_6"))
  _assert_same_checkpoint(_ckpt(os.path.join(resumed, "checkpoint_8")), c8)
  assert [r for r in _records(resumed, "train") if "event" in r] == [{"step": 4, "event": "quant_start"}]


# ---- 5. pretrained + prune, and it learns -----------------------------------------------------------

def _pretrained_run(dev, root):
  return _train(dev, root, "pretrained", [{}], pretrained=_pretrained(root), quant_prune_global=True,
                weight_decay=0.0, **lc.LEARN)


def test_pretrained_is_pruned_globally_and_stays_so(dev, root):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import prune_utils
  workdir, state, cfg = _pretrained_run(dev, root)
  assert state.step == S * cfg.num_epochs
  ck = _ckpt(os.path.join(workdir, "checkpoint_%d" % state.step))
  want = prune_utils.update_global_prune_mask(nn.tree_from_numpy(lc.pretrained_tree()["params"], "cpu"), 0.9)
  zeros = total = 0
  for l in _quant_layers(ck):
    mask = ck[l + "/prune_0/mask"]
    np.testing.assert_array_equal(mask, want[l.split("/")[-1]]["prune_0"]["mask"].numpy(), err_msg=l)
    zeros, total = zeros + int((mask == 0).sum()), total + mask.size
    assert set(np.unique(mask)) <= {0.0, 1.0}
    # quantised from the first step on (no start_epoch): a, c were set from the kernels, and trained
    assert ck[l + "/DuQ_0/a"] > 0 and ck[l + "/DuQ_0/c"] > 0
  assert zeros == int(total * 0.9)


def test_it_learns(dev, root):
  """The mean training loss of the last epoch is below the first epoch's, on the settings with which
  the float64 reference shows it (test_train_loop_cpu: 0.38 -> 0.17 .. 0.20)."""
  workdir, _, cfg = _pretrained_run(dev, root)
  loss = [r["loss"] for r in _records(workdir, "train")]
  assert len(loss) == S * cfg.num_epochs
  first, last = np.mean(loss[:S]), np.mean(loss[-S:])
  print("training losses", loss, "first epoch", first, "last epoch", last)
  assert np.isfinite(loss).all() and last < first


# ---- 6. the command line ----------------------------------------------------------------------------

def test_cli(root):
  work = root / "cli"
  work.mkdir()
  src, test = _sources()
  np.savez(str(work / "train.npz"), **src)
  np.savez(str(work / "test.npz"), **test)
  (work / "config.py").write_text(
      "from tests import train_loop_cases as lc\n\n\n"
      "def get_config():\n"
      "  return lc.make_config(num_epochs=1, dataset=%r, eval_dataset=%r)\n"
      % (str(work / "train.npz"), str(work / "test.npz")))
  env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
  out = subprocess.run([sys.executable, "-m", "snnquantprune_amd.train", "--config", str(work / "config.py"),
                        "--workdir", str(work / "run")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
  assert out.returncode == 0, out.stderr[-4000:]
  lines = [l for l in out.stdout.splitlines() if l.strip()]
  assert len(lines) == 1, out.stdout
  result = json.loads(lines[0])
  assert set(result) == {"eval", "best_accuracy"} and result["eval"]["step"] == S and result["eval"]["epoch"] == 1
  assert result["eval"] == _records(str(work / "run"), "eval")[-1]
  assert os.path.isfile(work / "run" / ("checkpoint_%d" % S))
