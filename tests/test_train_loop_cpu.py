"""The training loop, host side (snnquantprune_amd/train.py and what it stands on): the
learning-rate schedules against their formulas, the checkpoint tree and its restore, retention,
the resumable event plan, the step rng, sync_batch_stats over two gloo ranks, the loop's refusals,
and the float64 replay that shows the GPU tests' fixture can be learnt."""
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import train_loop_cases as lc
from tests.test_dense_train_cpu import _free_port

RTOL = 1e-12        # both sides are float64


def close(got, want):
  assert got == pytest.approx(want, rel=RTOL, abs=0 if want else 1e-300), (got, want)


# ---- schedules -------------------------------------------------------------------------------------

def _linear(step, init, end, n):
  if n == 0:
    return init
  c = min(max(step, 0), n)
  return (init - end) * (1 - c / n) + end


def _cosine(step, init, n):
  return init * 0.5 * (1 + math.cos(math.pi * min(step, n) / n))


def test_schedule_primitives_follow_their_formulas():
  from snnquantprune_amd import train_utils as tu
  lin = tu.linear_schedule(0.25, 2.0, 10)
  for step in (0, 5, 9, 10, 25):
    close(lin(step), _linear(step, 0.25, 2.0, 10))
  assert lin(0) == 0.25 and lin(10) == 2.0 and lin(25) == 2.0
  assert [tu.linear_schedule(0.7, 0.1, 0)(s) for s in (0, 1, 100)] == [0.7] * 3
  cos = tu.cosine_decay_schedule(0.3, 12)
  for step in (0, 6, 11, 12, 40):
    close(cos(step), _cosine(step, 0.3, 12))
  assert cos(0) == 0.3 and cos(12) == 0.0 and cos(40) == 0.0
  # join: schedule i + 1 counts from its boundary
  joined = tu.join_schedules([lin, cos, tu.linear_schedule(1.0, 0.0, 4)], [10, 22])
  for step, want in ((0, _linear(0, 0.25, 2.0, 10)), (9, _linear(9, 0.25, 2.0, 10)), (10, 0.3),
                     (16, _cosine(6, 0.3, 12)), (21, _cosine(11, 0.3, 12)), (22, 1.0), (24, 0.5), (99, 0.0)):
    close(joined(step), want)
  # sgdr: a cosine per cycle, restarted
  sg = tu.sgdr_schedule([dict(init_value=0.2, peak_value=0.2, warmup_steps=0, decay_steps=8)] * 2)
  for step, want in ((0, 0.2), (4, _cosine(4, 0.2, 8)), (7, _cosine(7, 0.2, 8)), (8, 0.2),
                     (15, _cosine(7, 0.2, 8)), (16, 0.0), (30, 0.0)):
    close(sg(step), want)


def test_piecewise_constant_away_from_and_at_the_boundaries():
  """The scale of a boundary holds from the step after it (step > boundary)."""
  from snnquantprune_amd import train_utils as tu
  pw = tu.piecewise_constant_schedule(0.1, {10: 0.5, 20: 0.2})
  for step, want in ((0, 0.1), (5, 0.1), (15, 0.1 * 0.5), (25, 0.1 * 0.5 * 0.2), (1000, 0.1 * 0.5 * 0.2)):
    close(pw(step), want)
  close(pw(10), 0.1)
  close(pw(11), 0.1 * 0.5)
  close(pw(20), 0.1 * 0.5)
  close(pw(21), 0.1 * 0.5 * 0.2)


def _cfg(**kw):
  from snnquantprune_amd import synthetic as syn
  cfg = syn.make_config()
  for k, v in kw.items():
    cfg[k] = v
  return cfg


def test_plain_warmup_cosine():
  from snnquantprune_amd import train_utils as tu
  S, base = 7, 0.05
  f = tu.create_learning_rate_fn(_cfg(num_epochs=10, warmup_epochs=0), base, S)
  for step in (0, 35, 69, 70, 200):
    close(f(step), _cosine(step, base, 10 * S))
  f = tu.create_learning_rate_fn(_cfg(num_epochs=10, warmup_epochs=2), base, S)
  for step in (0, 7, 13):
    close(f(step), base * step / (2 * S))
  for step in (14, 42, 69, 70, 200):
    close(f(step), _cosine(step - 2 * S, base, 8 * S))
  assert f(0) == 0.0 and f(14) == base and f(70) == 0.0


def test_t_max_restarts():
  from snnquantprune_amd import train_utils as tu
  S, base = 5, 0.4
  f = tu.create_learning_rate_fn(_cfg(num_epochs=7, warmup_epochs=2, t_max=3), base, S)   # 3 cycles of 15 steps
  for cycle in range(3):
    for k in (0, 7, 14):
      close(f(15 * cycle + k), _cosine(k, base, 15))
  for restart in (15, 30):
    assert f(restart - 1) < f(restart) == base
    close(f(restart - 1), _cosine(14, base, 15))
  assert f(45) == 0.0 and f(100) == 0.0


def test_lr_boundaries_scale_branch_comes_first():
  from snnquantprune_amd import train_utils as tu
  S = 4
  cfg = _cfg(num_epochs=9, warmup_epochs=1, t_max=3, learning_rate=0.2, lr_boundaries_scale={"2": 0.1, "5": 0.5})
  f = tu.create_learning_rate_fn(cfg, 123.0, S)                    # (config.learning_rate is what it scales)
  for step, want in ((0, 0.2), (7, 0.2), (8, 0.2), (9, 0.02), (19, 0.02), (20, 0.02), (21, 0.01), (99, 0.01)):
    close(f(step), want)


def test_start_epoch_cascade():
  from snnquantprune_amd import train_utils as tu
  S, base = 6, 0.08
  cfg = _cfg(num_epochs=50, warmup_epochs=2)
  cfg.quant.start_epoch = -1                                       # the shipped joint config
  f = tu.create_learning_rate_fn(cfg, base, S)
  for step in (0, 1, S - 1):
    close(f(step), base * (S + step) / (2 * S))
  for step in (S, S + 10, 30 * S, 50 * S - 1, 50 * S, 60 * S):
    close(f(step), _cosine(step - S, base, 49 * S))
  close(f(0), base / 2)
  close(f(S), base)
  close(f(S + 49 * S // 2), base / 2)
  assert f(50 * S) == 0.0 and f(50 * S + 17) == 0.0

  # start_epoch = 3, warmup 2, 10 epochs: boundaries 2 S, (1 S + 2 S) = 3 S, 5 S.  By hand:
  # warm-up on [0, 2 S); cosine over max(3 - 2, 1) S from 2 S on; a second warm-up from 3 S; a
  # cosine over max(10 - 3 - 2, 1) = 5 S from 5 S on
  cfg = _cfg(num_epochs=10, warmup_epochs=2)
  cfg.quant.start_epoch = 3
  f = tu.create_learning_rate_fn(cfg, base, S)
  for step in (0, 5, 2 * S - 1):
    close(f(step), base * step / (2 * S))
  for step in (2 * S, 2 * S + 3, 3 * S - 1):
    close(f(step), _cosine(step - 2 * S, base, S))
  for step in (3 * S, 4 * S, 5 * S - 1):
    close(f(step), base * (step - 3 * S) / (2 * S))
  for step in (5 * S, 7 * S, 10 * S - 1, 10 * S, 12 * S):
    close(f(step), _cosine(step - 5 * S, base, 5 * S))
  # no warm-up: two cosines joined at the start epoch
  cfg = _cfg(num_epochs=10, warmup_epochs=0)
  cfg.quant.start_epoch = 3
  f = tu.create_learning_rate_fn(cfg, base, S)
  for step, want in ((0, base), (S, _cosine(S, base, 3 * S)), (3 * S - 1, _cosine(3 * S - 1, base, 3 * S)),
                     (3 * S, base), (6 * S, _cosine(3 * S, base, 7 * S)), (10 * S, 0.0)):
    close(f(step), want)


# ---- the checkpoint tree ---------------------------------------------------------------------------

def _at(tree, path):
  for k in path:
    tree = tree[k]
  return tree


def _tree_keys(t):
  return {k: _tree_keys(v) for k, v in t.items()} if isinstance(t, dict) else None


def test_checkpoint_tree_after_three_adam_steps(tmp_path):
  from snnquantprune_amd import checkpoint
  from snnquantprune_amd import train_utils as tu
  state = lc.toy_state("adam")
  for _ in range(3):
    state = lc.toy_step(state)
  path = tu.save_checkpoint(state, str(tmp_path))
  assert path == str(tmp_path / "checkpoint_3") and os.listdir(tmp_path) == ["checkpoint_3"]
  with open(path, "rb") as f:
    tree = checkpoint.msgpack_restore(f.read())
  ptree = {"QuantDense_0": {"kernel": None, "DuQ_0": {"a": None, "c": None}, "prune_0": {"mask": None}},
           "BatchNorm_0": {"scale": None, "bias": None}}
  assert _tree_keys(tree) == {
      "step": None, "params": {"params": ptree}, "batch_stats": {"BatchNorm_0": {"mean": None, "var": None}},
      "opt_state": {"0": {"count": None, "mu": {"params": ptree}, "nu": {"params": ptree}}, "1": {"count": None}}}
  assert tree["step"] == 3 and tree["opt_state"]["0"]["count"] == 3 and tree["opt_state"]["1"]["count"] == 3
  for path_, p in tu._flatten(state.params["params"]):
    got = _at(tree["params"]["params"], path_)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, p.numpy())
    np.testing.assert_array_equal(_at(tree["opt_state"]["0"]["mu"]["params"], path_), state.tx.state[p]["exp_avg"].numpy())
    np.testing.assert_array_equal(_at(tree["opt_state"]["0"]["nu"]["params"], path_), state.tx.state[p]["exp_avg_sq"].numpy())
  # the readers of the reference's files take it as it is
  loaded = checkpoint.load_flax_checkpoint(path)
  for path_, p in tu._flatten(state.params["params"]):
    np.testing.assert_array_equal(_at(loaded["params"], path_), p.numpy())
  for path_, p in tu._flatten(state.batch_stats):
    np.testing.assert_array_equal(_at(loaded["batch_stats"], path_), p.numpy())


def test_untouched_optimiser_is_written_as_zeros(tmp_path):
  from snnquantprune_amd import checkpoint
  from snnquantprune_amd import train_utils as tu
  for opt, kw, first in (("adam", {}, {"count", "mu", "nu"}), ("sgd", dict(momentum=0.9), {"trace"}), ("sgd", {}, set())):
    state = lc.toy_state(opt, **kw)
    with open(tu.save_checkpoint(state, str(tmp_path / (opt + str(len(kw))))), "rb") as f:
      opt_state = checkpoint.msgpack_restore(f.read())["opt_state"]
    assert set(opt_state) == {"0", "1"} and set(opt_state["0"]) == first and set(opt_state["1"]) == {"count"}
    assert opt_state["1"]["count"] == 0
    for m in first - {"count"}:
      for _, a in tu._flatten(opt_state["0"][m]["params"]):
        assert a.dtype == np.float32 and not a.any()


@pytest.mark.parametrize("opt,kw", [("adam", {}), ("sgd", dict(momentum=0.9, nesterov=True)), ("sgd", {})],
                         ids=["adam", "sgd-nesterov", "sgd-plain"])
def test_restore_then_two_steps_equals_five(tmp_path, opt, kw):
  from snnquantprune_amd import train_utils as tu
  whole = lc.toy_state(opt, **kw)
  for _ in range(5):
    whole = lc.toy_step(whole)
  first = lc.toy_state(opt, **kw)
  for _ in range(3):
    first = lc.toy_step(first)
  tu.save_checkpoint(first, str(tmp_path))
  state = lc.toy_state(opt, seed=99, **kw)                          # other values: the restore has to replace them
  tensors = [p for _, p in tu._flatten(state.params["params"])]
  restored = tu.restore_checkpoint(state, str(tmp_path))
  assert restored is state and state.step == 3
  assert all(a is b for a, b in zip(tensors, (p for _, p in tu._flatten(state.params["params"]))))
  assert all(a is b for a, b in zip(tensors, state.tx.param_groups[0]["params"]))
  for k, v in lc.state_arrays(first).items():
    np.testing.assert_array_equal(lc.state_arrays(state)[k], v, err_msg=k)
  for _ in range(2):
    state = lc.toy_step(state)
  want, got = lc.state_arrays(whole), lc.state_arrays(state)
  assert set(got) == set(want) and got["step"] == 5
  if opt == "adam":
    assert any(k.startswith("opt/exp_avg_sq/") for k in want)
  elif kw:
    assert any(k.startswith("opt/momentum_buffer/") for k in want)
  for k, v in want.items():
    np.testing.assert_array_equal(got[k], v, err_msg=k)


def test_restore_at_step_zero_is_a_fresh_optimiser(tmp_path):
  from snnquantprune_amd import train_utils as tu
  tu.save_checkpoint(lc.toy_state("adam"), str(tmp_path))
  state = tu.restore_checkpoint(lc.toy_state("adam", seed=5), str(tmp_path))
  whole = lc.toy_state("adam")
  for _ in range(2):
    state, whole = lc.toy_step(state), lc.toy_step(whole)
  for k, v in lc.state_arrays(whole).items():
    np.testing.assert_array_equal(lc.state_arrays(state)[k], v, err_msg=k)


def test_retention_overwrite_and_latest(tmp_path):
  from snnquantprune_amd import checkpoint, eval as ev
  from snnquantprune_amd import train_utils as tu
  state = lc.toy_state("adam")
  for _ in range(5):
    state = lc.toy_step(state)
    tu.save_checkpoint(state, str(tmp_path))
  assert sorted(os.listdir(tmp_path)) == ["checkpoint_3", "checkpoint_4", "checkpoint_5"]
  assert ev.latest_checkpoint(str(tmp_path)) == str(tmp_path / "checkpoint_5")
  for _ in range(7):                                                # natural order: 12 is newer than 9
    state = lc.toy_step(state)
    tu.save_checkpoint(state, str(tmp_path), keep=2)
  assert sorted(os.listdir(tmp_path)) == ["checkpoint_11", "checkpoint_12"]
  # a save of the same step replaces the file
  before = checkpoint.load_flax_checkpoint(str(tmp_path / "checkpoint_12"))["params"]["BatchNorm_0"]["bias"]
  with torch.no_grad():
    state.params["params"]["BatchNorm_0"]["bias"] += 1.0
  tu.save_checkpoint(state, str(tmp_path), keep=2)
  after = checkpoint.load_flax_checkpoint(str(tmp_path / "checkpoint_12"))["params"]["BatchNorm_0"]["bias"]
  np.testing.assert_array_equal(after, before + np.float32(1))
  assert sorted(os.listdir(tmp_path)) == ["checkpoint_11", "checkpoint_12"]


def test_restore_refuses_another_tree_and_passes_a_missing_workdir(tmp_path):
  from snnquantprune_amd import train_utils as tu
  state = lc.toy_state("adam")
  before = lc.state_arrays(state)
  for workdir in (str(tmp_path / "nowhere"), str(tmp_path), ""):
    assert tu.restore_checkpoint(state, workdir) is state
  for k, v in before.items():
    np.testing.assert_array_equal(lc.state_arrays(state)[k], v)
  bad = lc.toy_step(lc.toy_state("adam"))                           # a file with one leaf of another shape
  bad.params["params"]["QuantDense_0"]["DuQ_0"]["c"] = torch.ones(2)
  tu.save_checkpoint(bad, str(tmp_path / "bad"))
  with pytest.raises(ValueError, match="params/params/QuantDense_0/DuQ_0/c"):
    tu.restore_checkpoint(lc.toy_state("adam"), str(tmp_path / "bad"))
  tu.save_checkpoint(lc.toy_step(state), str(tmp_path))
  other = lc.toy_state("adam")
  del other.batch_stats["BatchNorm_0"]["var"]
  with pytest.raises(ValueError, match="batch_stats/BatchNorm_0/var"):
    tu.restore_checkpoint(other, str(tmp_path))
  with pytest.raises(ValueError, match="opt_state/0/trace"):
    tu.restore_checkpoint(lc.toy_state("sgd", momentum=0.9), str(tmp_path))


# ---- the resumable plan ----------------------------------------------------------------------------

@pytest.mark.parametrize("split_by", ["number", "time"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_skip_continues_the_plan(split_by, train):
  from snnquantprune_amd import input_pipeline as ip
  cfg = lc.make_config(split_by)
  n = 18                                                            # 4 batches an epoch, 2 recordings dropped
  t_min = np.arange(n, dtype=np.int64) * 7
  t_max = t_min + 20000 + 100 * np.arange(n)

  def take(skip, k):
    plan = ip.EventPlan(cfg, (lc.H, lc.W), n, train=train)
    it = plan.batches(t_min, t_max, skip) if skip is not None else plan.batches(t_min, t_max)
    return [next(it) for _ in range(k)]

  epoch = n // lc.BATCH
  fresh = take(None, 3 * epoch)
  if split_by == "time":
    assert len({tuple(s) for _, s in fresh[:epoch]}) == epoch     # origins do get drawn
  for k in (0, 1, epoch, epoch + 1):
    got = take(k, epoch + 2)
    for (ia, sa), (ib, sb) in zip(got, fresh[k:]):
      np.testing.assert_array_equal(ia, ib)
      if split_by == "time":
        np.testing.assert_array_equal(sa, sb)
      else:
        assert sa is None and sb is None
  with pytest.raises(ValueError, match="skip"):
    take(-1, 1)


# ---- the step rng ----------------------------------------------------------------------------------

def test_step_rng_is_a_function_of_seed_rank_and_step():
  from snnquantprune_amd.train import step_rng
  base = step_rng(5, 0, 7)
  assert isinstance(base, int) and 0 <= base < 2 ** 63
  assert step_rng(5, 0, 7) == base                                  # no state between calls
  others = [step_rng(6, 0, 7), step_rng(5, 1, 7), step_rng(5, 0, 8), step_rng(7, 0, 5), step_rng(0, 5, 7)]
  assert len({base, *others}) == 6
  assert len({step_rng(5, 0, s) for s in range(1000)}) == 1000
  g = torch.Generator()
  g.manual_seed(base)                                               # a seed torch takes


# ---- two ranks -------------------------------------------------------------------------------------

def _sync_worker(rank, world, port, workdir, out):
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from snnquantprune_amd import train_utils as tu
    state = lc.toy_state("adam")
    with torch.no_grad():
      for _, t in tu._flatten(state.batch_stats):
        t.mul_(rank + 1)                                            # rank 1 holds twice rank 0's
    assert tu.sync_batch_stats(state) is state
    out[rank] = {"/".join(p): t.tolist() for p, t in tu._flatten(state.batch_stats)}
    out["path%d" % rank] = tu.save_checkpoint(state, workdir)
    dist.barrier()
  finally:
    dist.destroy_process_group()


def test_gloo_world2_sync_batch_stats_and_rank0_writes(tmp_path):
  from snnquantprune_amd import train_utils as tu
  port = _free_port()
  with mp.Manager() as m:
    out = m.dict()
    mp.spawn(_sync_worker, args=(2, port, str(tmp_path), out), nprocs=2, join=True)
    want = {"/".join(p): (t * 1.5).tolist() for p, t in tu._flatten(lc.toy_state("adam").batch_stats)}
    assert out[0] == want and out[1] == want
    assert out["path0"] == str(tmp_path / "checkpoint_0") and out["path1"] is None
  assert os.listdir(tmp_path) == ["checkpoint_0"]


def test_sync_batch_stats_without_distributed_is_identity():
  from snnquantprune_amd import train_utils as tu
  state = lc.toy_state("adam")
  before = lc.state_arrays(state)
  assert tu.sync_batch_stats(state) is state
  for k, v in before.items():
    np.testing.assert_array_equal(lc.state_arrays(state)[k], v)


# ---- what the loop refuses before it touches a device ----------------------------------------------

def test_loop_refusals(tmp_path, monkeypatch):
  from snnquantprune_amd import train
  src, test = lc.sources()
  with pytest.raises(NotImplementedError, match="online"):
    train.train_and_evaluate(lc.make_config(online=True), str(tmp_path), source=src, eval_source=test)
  frames = {"dvs_matrix": np.zeros((16, lc.T, lc.H, lc.W, 2), np.uint8), "label": np.arange(16) % 2}
  with pytest.raises(NotImplementedError, match="event source"):
    train.train_and_evaluate(lc.make_config(), str(tmp_path), source=frames, eval_source=test)
  path = str(tmp_path / "frames.npz")
  np.savez(path, **frames)
  with pytest.raises(NotImplementedError, match="event source"):
    train.train_and_evaluate(lc.make_config(dataset=path), str(tmp_path))
  monkeypatch.setenv("WORLD_SIZE", "3")
  for kw, size in ((dict(batch_size=4, eval_batch_size=6), 4), (dict(batch_size=6, eval_batch_size=4), 4)):
    with pytest.raises(ValueError) as e:
      train.train_and_evaluate(lc.make_config(**kw), str(tmp_path), source=src, eval_source=test)
    assert str(e.value) == "Batch size (%d) must be divisible by the number of devices (3)." % size
  assert not dist.is_initialized() and os.listdir(tmp_path) == ["frames.npz"]


# ---- the fixture of the GPU tests can be learnt ----------------------------------------------------

def test_float64_reference_lowers_its_loss_on_the_fixture(oracle):
  """What test_train_loop_gpu's "it learns" stands on: TorchConvDenseSNN64, started from the
  pretrained weights the loop loads and prepares (global 90 % masks, DuQ scalars), on the loop's own
  batches, learning rates and Adam, ends its last epoch with a lower mean loss than its first."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import prune_utils
  from snnquantprune_amd import train_utils as tu
  cfg = lc.make_config(**lc.LEARN)
  src, _ = lc.sources()
  S = lc.N_TRAIN // lc.BATCH
  steps = S * cfg.num_epochs
  variables = nn.tree_from_numpy(lc.pretrained_tree(), "cpu")
  params = prune_utils.prepare_params(variables["params"], cfg)
  variables = {"params": nn.tree_map(lambda t: t.numpy(), params), "batch_stats": {}}
  losses = lc.reference_losses(variables, lc.host_batches(src, cfg, steps), tu.create_learning_rate_fn(cfg, cfg.learning_rate, S))
  first, last = np.mean(losses[:S]), np.mean(losses[-S:])
  print("float64 reference losses", losses, "first epoch", first, "last epoch", last)
  # by a margin the dropout draws do not decide (the device draws other masks than these)
  assert np.isfinite(losses).all() and last < 0.7 * first
