"""Gradual pruning inside train.train_and_evaluate, on the fixture of
tests/train_loop_cases.py: 3 epochs of 4 steps from the pretrained weights, events at steps 0, 3
and 6 (start_epoch 0, end_epoch 2 = step 8, every 3 steps: t1 = 6) from 30 % to 90 % sparsity."""
import json
import os

import numpy as np
import pytest
import torch

from tests import train_loop_cases as lc

pytestmark = pytest.mark.gpu

S = lc.N_TRAIN // lc.BATCH          # steps per epoch
SCHEDULE = dict(start_epoch=0, end_epoch=2, every_steps=3, initial=0.3)
EVENTS, T1, FINAL = (0, 3, 6), 6, 0.9


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
  return tmp_path_factory.mktemp("prune_schedule")


_src, _done = {}, {}


def _sources():
  if not _src:
    _src["train"], _src["test"] = lc.sources()
  return _src["train"], _src["test"]


def _train(dev, root, name, stages, **cfg_kw):
  """One workdir per name, trained once: train_and_evaluate per stage (an interrupted run is two)."""
  if name not in _done:
    from snnquantprune_amd import train
    workdir = str(root / name)
    path = str(root / "pretrained_0")
    if not os.path.exists(path):
      lc.write_flax_file(path, lc.pretrained_tree())
    src, test = _sources()
    for stage in stages:
      cfg = lc.make_config(**{**lc.LEARN, "pretrained": path, "num_epochs": 3, **cfg_kw, **stage})
      state = train.train_and_evaluate(cfg, workdir, source=src, eval_source=test, device=dev)
    _done[name] = (workdir, state, cfg)
  return _done[name]


def _scheduled(dev, root):
  return _train(dev, root, "scheduled", [{}], quant_prune_schedule=SCHEDULE)


def _records(workdir, which):
  with open(os.path.join(workdir, which, "metrics.jsonl")) as f:
    return [json.loads(line) for line in f]


def _ckpt(path):
  from snnquantprune_amd import checkpoint
  from snnquantprune_amd import train_utils as tu
  with open(path, "rb") as f:
    return {"/".join(p): v for p, v in tu._flatten(checkpoint.msgpack_restore(f.read()))}


def _masks(ck):
  return {k: v for k, v in ck.items() if k.startswith("params/") and k.endswith("/prune_0/mask")}


def test_events_fall_on_the_schedule(dev, root):
  from snnquantprune_amd import prune_utils as pu
  workdir, state, cfg = _scheduled(dev, root)
  assert state.step == 3 * S
  sched = pu.resolve_prune_schedule(cfg.quant, S)
  assert sched == pu.PruneSchedule(0, T1, 3, 0.3)
  events = [r for r in _records(workdir, "train") if "event" in r]
  total = sum(int(l["prune_0"]["mask"].numel()) for l in pu._layers(state.params["params"]))
  assert len(pu._layers(state.params["params"])) == 3 and total > 1000
  want = [{"step": t, "event": "prune", "sparsity": pu.sparsity_at(t, sched, FINAL),
           "zeros": int(total * pu.sparsity_at(t, sched, FINAL)), "weights": total} for t in EVENTS]
  assert events == want
  assert [e["sparsity"] for e in events] == [0.3, 0.9 + (0.3 - 0.9) * 0.5 ** 3, 0.9]
  # the record sits in front of its step's metrics
  rec = _records(workdir, "train")
  for t in EVENTS:
    i = rec.index(next(e for e in events if e["step"] == t))
    assert rec[i + 1]["step"] == t + 1 and "loss" in rec[i + 1]


def test_masks_hold_the_scheduled_zeros_and_only_grow(dev, root):
  from snnquantprune_amd import prune_utils as pu
  workdir, state, cfg = _scheduled(dev, root)
  sched = pu.resolve_prune_schedule(cfg.quant, S)
  cks = [_masks(_ckpt(os.path.join(workdir, "checkpoint_%d" % s))) for s in (S, 2 * S, 3 * S)]
  total = sum(v.size for v in cks[0].values())
  # checkpoint_4 lies behind the event at 3, the other two behind the last one
  for ck, t in zip(cks, (3, 6, 6)):
    assert sum(int((v == 0).sum()) for v in ck.values()) == int(total * pu.sparsity_at(t, sched, FINAL))
    assert all(set(np.unique(v)) <= {0.0, 1.0} for v in ck.values())
  for a, b in zip(cks, cks[1:]):
    for k in a:
      assert not ((a[k] == 0) & (b[k] != 0)).any(), k              # no weight comes back
  for k, v in cks[2].items():
    np.testing.assert_array_equal(v, cks[1][k])                     # nothing moves after t1
  # the global cut is uneven over the layers (or the test would not tell global from per layer)
  fractions = [float((v == 0).mean()) for v in cks[2].values()]
  print("pruned fraction per layer", fractions)
  assert max(fractions) - min(fractions) > 0.01


def test_resume_across_an_event_is_exact(dev, root):
  """Stopped at step 5, between the events at 3 and 6, and continued in the same workdir."""
  a, state_a, _ = _scheduled(dev, root)
  b, state_b, _ = _train(dev, root, "resumed", [dict(num_train_steps=5), dict(num_train_steps=-1)],
                         quant_prune_schedule=SCHEDULE)
  assert state_a.step == state_b.step == 3 * S
  assert os.path.exists(os.path.join(b, "checkpoint_5"))
  ca, cb = _ckpt(os.path.join(a, "checkpoint_%d" % (3 * S))), _ckpt(os.path.join(b, "checkpoint_%d" % (3 * S)))
  assert set(ca) == set(cb) and _masks(ca) and any(k.startswith("opt_state/0/nu/") for k in ca)
  for k, v in ca.items():
    np.testing.assert_array_equal(cb[k], v, err_msg=k)
  strip = lambda rs: [{k: v for k, v in r.items() if k != "steps_per_second"} for r in rs]   # noqa: E731
  assert strip(_records(b, "train")) == strip(_records(a, "train"))
  assert _records(b, "eval")[-4:] == _records(a, "eval")
  # and a run resumed AT an event step repeats that event once
  c, state_c, _ = _train(dev, root, "resumed-at-event", [dict(num_train_steps=6), dict(num_train_steps=-1)],
                         quant_prune_schedule=SCHEDULE)
  cc = _ckpt(os.path.join(c, "checkpoint_%d" % (3 * S)))
  for k, v in ca.items():
    np.testing.assert_array_equal(cc[k], v, err_msg=k)
  assert strip(_records(c, "train")) == strip(_records(a, "train"))
  assert len({r["loss"] for r in _records(a, "train") if "loss" in r}) == 3 * S     # the numbers do move


def test_best_waits_for_the_final_sparsity(dev, root):
  workdir, _, _ = _scheduled(dev, root)
  ev = _records(workdir, "eval")
  assert [(r["step"], r["epoch"]) for r in ev] == [(0, 0), (S, 1), (2 * S, 2), (3 * S, 3)]
  print("eval records", ev)
  assert not any(r["best"] for r in ev if r["step"] <= T1)
  # the same run without the wait would have taken the first epoch's model whenever it scores
  best = os.path.join(workdir, "best")
  saved = sorted(os.listdir(best)) if os.path.isdir(best) else []
  assert len(saved) == [r["best"] for r in ev].count(True)
  assert all(int(f.split("_")[-1]) > T1 for f in saved)


def test_the_loops_evaluation_uses_the_pruned_kernels(dev, root):
  """The last record of the loop, whose packs were made before, between and after the events, is
  what a fresh model computes from the final checkpoint."""
  from snnquantprune_amd import eval as ev
  workdir, _, cfg = _scheduled(dev, root)
  _, summary, _ = ev.evaluate_metrics(cfg, workdir, source=_sources()[1], device=dev)
  last = _records(workdir, "eval")[-1]
  assert (summary["loss"], summary["accuracy"]) == (last["loss"], last["accuracy"])


@pytest.mark.parametrize("global_", [True, False], ids=["global", "per-layer"])
def test_an_evaluation_right_after_an_event_sees_it(dev, root, global_):
  """Evaluate (the packs of the current masks are cached), prune further in place, evaluate again:
  the logits are those of a freshly constructed model on copies of the leaves."""
  from snnquantprune_amd import input_pipeline, models, prune_utils as pu
  from snnquantprune_amd import linen as nn
  _, state, cfg = _scheduled(dev, root)
  params = nn.tree_map(lambda t: t.detach().clone(), state.params["params"])     # (the shared run's state stays as it is)
  stats = nn.tree_map(lambda t: t.detach().clone(), state.batch_stats)
  batch = next(input_pipeline.create_input_iter(_sources()[1], cfg, train=False, cache=True, device=dev))

  def logits(model, p, s):
    (out, _), _ = model.apply({"params": p, "batch_stats": s}, batch["dvs_matrix"], trgt=batch["label"], train=False,
                              online=False, rng=None, mutable=["batch_stats"], rngs={"dropout": None})
    return out.detach().clone()

  model = models.ConvDenseSNN(num_classes=cfg.num_classes, config=cfg)
  before = logits(model, params, stats)
  assert torch.equal(before, logits(model, params, stats))          # (served from the caches)
  pu.prune_event(params, 0.97, global_)
  after = logits(model, params, stats)
  fresh = logits(models.ConvDenseSNN(num_classes=cfg.num_classes, config=cfg),
                 nn.tree_map(lambda t: t.detach().clone(), params), nn.tree_map(lambda t: t.detach().clone(), stats))
  assert torch.equal(after, fresh)
  zeros, weights = pu.mask_zeros(params)
  assert int(zeros) >= int(weights * 0.97) - (0 if global_ else 3)
  print("logits before", before.tolist(), "after", after.tolist())
  assert not torch.equal(before, after)                             # the event changed what the net computes


def test_no_schedule_no_event(dev, root):
  workdir, state, _ = _train(dev, root, "unscheduled", [{}], num_epochs=1)
  rec = _records(workdir, "train")
  assert state.step == S and not [r for r in rec if r.get("event") == "prune"]
  # the one-shot masks of the load are there instead
  ck = _masks(_ckpt(os.path.join(workdir, "checkpoint_%d" % S)))
  total = sum(v.size for v in ck.values())
  assert sum(int((v == 0).sum()) for v in ck.values()) == int(total * FINAL)


def test_refusals_come_before_anything_is_written(dev, root):
  from snnquantprune_amd import train
  src, test = _sources()
  workdir = str(root / "refused")
  for sched, kw in ((dict(SCHEDULE, until=3), {}), (dict(SCHEDULE, every_steps=0), {}), (dict(SCHEDULE, initial=0.95), {}),
                    (dict(SCHEDULE, end_epoch=-1), {}), (SCHEDULE, dict(quant_prune_percentage=0.0))):
    with pytest.raises(ValueError, match="prune_schedule"):
      train.train_and_evaluate(lc.make_config(quant_prune_schedule=sched, **kw), workdir, source=src, eval_source=test,
                               device=dev)
  assert not os.path.exists(workdir)
