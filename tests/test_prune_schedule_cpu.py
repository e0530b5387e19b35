"""The prune schedule's host logic that runs without a GPU: what
train.train_and_evaluate refuses before it loads or writes anything, and the bookkeeping of the
events -- which steps, which sparsity, which target count -- on the loop's own fixture sizes.  The
loop itself needs the training kernels: tests/test_prune_schedule_gpu.py."""
import os

import pytest
import torch

from tests import train_loop_cases as lc

SCHEDULE = dict(start_epoch=0, end_epoch=2, every_steps=3, initial=0.3)


@pytest.mark.parametrize("sched,kw", [
    (dict(SCHEDULE, until=3), {}), (dict(SCHEDULE, every_steps=0), {}), (dict(SCHEDULE, every_steps=-2), {}),
    (dict(SCHEDULE, initial=-0.01), {}), (dict(SCHEDULE, initial=0.95), {}), (dict(SCHEDULE, end_epoch=-1), {}),
    (dict(SCHEDULE, start_epoch=3), {}), (SCHEDULE, dict(quant_prune_percentage=0.0)),
    (SCHEDULE, dict(quant_prune_percentage=-1.0))])
def test_the_loop_refuses_a_bad_schedule_before_it_touches_anything(tmp_path, sched, kw):
  from snnquantprune_amd import train
  src, test = lc.sources()
  workdir = str(tmp_path / "run")
  with pytest.raises(ValueError, match="prune_schedule"):
    train.train_and_evaluate(lc.make_config(quant_prune_schedule=sched, **kw), workdir, source=src, eval_source=test)
  assert not os.path.exists(workdir) and not torch.distributed.is_initialized()


def test_event_bookkeeping_on_the_loops_fixture():
  from snnquantprune_amd import prune_utils as pu
  S = lc.N_TRAIN // lc.BATCH
  cfg = lc.make_config(quant_prune_schedule=SCHEDULE, num_epochs=3)
  sched = pu.resolve_prune_schedule(cfg.quant, S)
  assert sched == pu.PruneSchedule(0, 6, 3, 0.3)
  steps = [t for t in range(3 * S) if sched.is_event(t)]
  assert steps == [0, 3, 6]
  assert [pu.sparsity_at(t, sched, cfg.quant.prune_percentage) for t in steps] == [0.3, 0.9 + (0.3 - 0.9) * 0.5 ** 3, 0.9]
  # a config without the key has no schedule to resolve, and an unscheduled load prunes as before
  assert "prune_schedule" not in lc.make_config().quant
  tree = {"QuantDense_0": {"kernel": torch.arange(1.0, 21.0).reshape(4, 5)}}
  one_shot = pu.prepare_params(tree, lc.make_config())
  assert int((one_shot["QuantDense_0"]["prune_0"]["mask"] == 0).sum()) == 18
  scheduled = pu.prepare_params(tree, cfg, prune=False)
  assert bool((scheduled["QuantDense_0"]["prune_0"]["mask"] == 1).all())
  assert set(scheduled["QuantDense_0"]) == set(one_shot["QuantDense_0"])       # the quantiser part is unchanged
  for k in ("a", "c"):
    assert torch.equal(scheduled["QuantDense_0"]["DuQ_0"][k], one_shot["QuantDense_0"]["DuQ_0"][k])
