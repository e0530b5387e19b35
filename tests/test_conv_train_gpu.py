"""ConvDenseSNN training on the GPU, on the two-block fixture of tests/conv_train_reference.py
(channels 16, 8x8x2 frames, T = 3, B = 2; tests/test_conv_train_reference_cpu.py checks through the
oracle that it fires and has gradients): the saved forward against the oracle stepped with the
sown batch statistics, the statistics against float64, and the HIP backward against torch.autograd
on the float64 forward fed the saved float32 spikes (TorchConvDenseSNN64)."""
import numpy as np
import pytest
import torch

from tests import conv_train_reference as cr
from tests.train_helpers import _grad_tree, _np, _run_train

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
CASES = [(q, d) for q in (True, False) for d in ("uint8", "float32")]
_ids = ["%s-%s" % ("q4p90" if q else "float", d) for q, d in CASES]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _setup(dev, quantized, dtype="uint8", **fx):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  v, x = cr.fixture(quantized, dtype, **fx)
  cfg = syn.make_config(bits=cr.BITS, prune_percentage=0.9 if quantized else -1.0, channels=cr.CHANNELS,
                        tau=cr.TAU, quantized=quantized, num_conv_blocks=cr.NBLOCKS, dropout=cr.KEEP)
  model = models.ConvDenseSNN(num_classes=cr.CLASSES, config=cfg)
  return model, v, nn.tree_from_numpy(v, dev), torch.from_numpy(x).to(dev)


_runs = {}


def _run(dev, quantized, dtype):
  """One training forward and backward per case, shared by the checks (nothing modifies it)."""
  key = (quantized, dtype)
  if key not in _runs:
    from snnquantprune_amd import train_utils as tu
    model, v, variables, x = _setup(dev, quantized, dtype)
    params, logits, inter, stats = _run_train(model, variables, x, rng=11)
    labels = torch.arange(x.shape[0], device=dev) % cr.CLASSES
    tu.mse_loss(logits, labels).backward()
    torch.cuda.synchronize()
    _runs[key] = dict(model=model, v=v, variables=variables, x=x, params=params, logits=logits,
                      inter=inter, stats=stats, labels=labels, grads=_grad_tree(params))
  return _runs[key]


def _sown_stats(inter):
  return {i: (_np(inter["bn%d_mean" % i]), _np(inter["bn%d_var" % i])) for i in range(cr.NBLOCKS)}


# ---- 1. the saved forward is the oracle's, given the sown statistics -----------------------------

@pytest.mark.parametrize("quantized,dtype", CASES, ids=_ids)
def test_saved_state_bit_equal_oracle(dev, oracle, quantized, dtype):
  r = _run(dev, quantized, dtype)
  inter = r["inter"]
  assert set(inter) >= {"dropout_0", "conv0_h", "conv0_out", "bn0_mean", "bn0_var", "conv1_h", "conv1_out"}
  T, B, C = cr.T_STEPS, cr.BATCH, cr.CHANNELS
  assert tuple(inter["bn0_mean"].shape) == (T, C) and tuple(inter["bn1_var"].shape) == (T, C)
  assert tuple(inter["conv0_h"].shape) == (T, B, 8, 8, C) and tuple(inter["conv1_out"].shape) == (T, B, 4, 4, C)
  mask = _np(inter["dropout_0"])
  assert set(np.unique(mask)) <= {0.0, 1.0} and 0.7 < mask.mean() < 1.0
  fwd = cr.oracle_forward(r["v"]["params"], _np(r["x"]), mask, quantized, stats=_sown_stats(inter))
  for i in range(cr.NBLOCKS):
    rate = float(_np(inter["conv%d_out" % i]).mean())
    print("block", i, "rate", rate)
    assert 0.02 <= rate <= 0.30
    np.testing.assert_array_equal(_np(inter["conv%d_h" % i]), fwd["h%d" % i])
    np.testing.assert_array_equal(_np(inter["conv%d_out" % i]), fwd["s%d" % i])
  rate = float(_np(inter["dense_out"]).mean())
  print("read-out rate", rate)
  assert 0.02 <= rate <= 0.30
  np.testing.assert_array_equal(_np(inter["dense_h"]), fwd["hd"])
  np.testing.assert_array_equal(_np(inter["dense_out"]), fwd["sd"])
  np.testing.assert_allclose(_np(r["logits"]).astype(F64), fwd["logits"], rtol=1e-6)


# ---- 2. the statistics, and the running ones -----------------------------------------------------

@pytest.mark.parametrize("quantized,dtype", CASES, ids=_ids)
def test_batch_statistics_within_bound_of_float64(dev, oracle, quantized, dtype):
  """mean and var are float64 accumulations rounded once: within u of the float64 value, plus the
  float64 accumulation's own error (N 2^-53 of the mean magnitude, charged 1e-12)."""
  r = _run(dev, quantized, dtype)
  inter = r["inter"]
  fwd = cr.oracle_forward(r["v"]["params"], _np(r["x"]), _np(inter["dropout_0"]), quantized,
                          stats=_sown_stats(inter))
  for i in range(cr.NBLOCKS):
    cur = fwd["cur%d" % i].astype(F64)                       # [T, B, H, W, C], the float32 currents
    flat = cur.reshape(cur.shape[0], -1, cur.shape[-1])
    mean64 = flat.mean(1)
    ex2 = (flat * flat).mean(1)
    var64 = ex2 - mean64 * mean64
    mean, var = _sown_stats(inter)[i]
    assert mean.dtype == F32 and var.dtype == F32
    assert (np.abs(mean - mean64) <= U * np.abs(mean64) + 1e-12 * np.abs(flat).mean(1) + 2.0 ** -149).all()
    assert (np.abs(var - var64) <= U * np.abs(var64) + 1e-12 * ex2 + 2.0 ** -149).all()
    assert (var >= 0).all()


@pytest.mark.parametrize("quantized,dtype", CASES[:1] + CASES[2:3], ids=_ids[:1] + _ids[2:3])
def test_running_statistics_are_the_t_fold_recurrence(dev, quantized, dtype):
  r = _run(dev, quantized, dtype)
  m, k = F32(0.9), F32(1) - F32(0.9)
  for i in range(cr.NBLOCKS):
    old = r["v"]["batch_stats"]["BatchNorm_%d" % i]
    new = r["stats"]["BatchNorm_%d" % i]
    for name, sown in zip(("mean", "var"), _sown_stats(r["inter"])[i]):
      ra = old[name].astype(F32)
      for t in range(cr.T_STEPS):
        ra = (m * ra + k * sown[t]).astype(F32)
      np.testing.assert_array_equal(_np(new[name]), ra)
      assert not np.array_equal(ra, old[name])
      # the tree the apply was given is untouched
      np.testing.assert_array_equal(_np(r["variables"]["batch_stats"]["BatchNorm_%d" % i][name]), old[name])


def test_batch_stats_immutable_without_mutable(dev):
  model, v, variables, x = _setup(dev, True)
  (logits, _), mut = model.apply({"params": variables["params"], "batch_stats": variables["batch_stats"]},
                                 x, train=True, rng=11, mutable=["intermediates"])
  assert "batch_stats" not in mut
  assert torch.equal(logits, _run(dev, True, "uint8")["logits"])


# ---- 3. gradients against the float64 yardstick --------------------------------------------------

@pytest.mark.parametrize("quantized,dtype", CASES, ids=_ids)
def test_gradients_match_float64_autograd(dev, quantized, dtype):
  """Every parameter gradient within relative L2 1e-5 of TorchConvDenseSNN64 (the figure the dense
  model is held to).

  One kind of parameter cannot meet a relative figure: DuQ's c of a conv layer.  BatchNorm on batch
  statistics is invariant to the scale of its input, so dL/dc = sum_k g_k wq_k / c is zero but for
  eps: the terms cancel to some 1e-7 of their magnitude, and the float32 rounding of the terms
  (each inside 1e-6 of its own value) is as large as what is left.  Measured on MI355X:
  QuantConv_0/DuQ_0/c relative 0.371 at 4-bit / 90 % pruned, while QuantConv_0/kernel is 5.0e-7
  and QuantConv_0/DuQ_0/a 5.6e-7.  There the element-wise gamma bound of the weight gradient's
  chain decides (TorchConvDenseSNN64.c_gamma_bound): |got - ref| <= sum_k |wq_k / c| gamma(Rn)
  (|A|^T |gI|)_k."""
  from snnquantprune_amd import train_utils as tu
  r = _run(dev, quantized, dtype)
  inter = r["inter"]
  saved = {"hd": _np(inter["dense_h"]), "sd": _np(inter["dense_out"])}
  for i in range(cr.NBLOCKS):
    saved["h%d" % i], saved["s%d" % i] = _np(inter["conv%d_h" % i]), _np(inter["conv%d_out" % i])
  m = cr.TorchConvDenseSNN64(r["v"]["params"])
  lg = m.forward(_np(r["x"]), _np(inter["dropout_0"]), saved)
  np.testing.assert_allclose(lg.detach().numpy(), _np(r["logits"]).astype(F64), rtol=1e-6, atol=1e-7)
  assert m.h_gap < 1e-4, m.h_gap
  tu.mse_loss(lg, _np(r["labels"])).backward()
  ref = m.grads()
  got = r["grads"]
  worst = 0.0
  for (layer, name), want in ref.items():
    path = (layer, name) if layer.startswith("BatchNorm") else (
        (layer, "kernel") if name == "kernel" else (layer, "DuQ_0", name))
    g = got[path]
    if name in ("a", "c") and not quantized:
      assert g is None or np.abs(g).max() == 0.0             # a == -1: pass-through
      continue
    assert g is not None and np.abs(g).max() > 0, path
    rel = np.linalg.norm(g.astype(F64) - want) / np.linalg.norm(want)
    print("%-28s relative L2 %.3g" % ("/".join(path), rel))
    if rel > 1e-5 and name == "c" and layer.startswith("QuantConv"):
      bound = m.c_gamma_bound(int(layer.split("_")[1]))
      err = float(np.abs(g.astype(F64) - want).max())
      print("%-28s |got - ref| %.3g, gamma bound %.3g, |ref| %.3g" % ("/".join(path), err, bound,
                                                                      float(np.abs(want).max())))
      assert err <= bound, "%s: |got - ref| %.3g over the gamma bound %.3g" % ("/".join(path), err, bound)
      continue
    worst = max(worst, rel)
    assert rel <= 1e-5, "%s: relative L2 %.3g" % ("/".join(path), rel)
  for path, g in got.items():
    if path[-1] == "mask":
      assert g is None or np.abs(g).max() == 0.0
  print("worst relative L2 %.3g" % worst)


# ---- 4. reproducible -------------------------------------------------------------------------------

def test_backward_bitwise_reproducible(dev):
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _setup(dev, True, "uint8", B=8)
  labels = torch.arange(8, device=dev) % cr.CLASSES
  runs = []
  for _ in range(2):
    params, logits, _, _ = _run_train(model, variables, x, rng=7)
    tu.cross_entropy_loss(logits, labels).backward()
    runs.append(_grad_tree(params))
  for path, g in runs[0].items():
    if g is None:
      assert runs[1][path] is None
    else:
      assert g.tobytes() == runs[1][path].tobytes(), path


# ---- 5. one Adam step ------------------------------------------------------------------------------

def test_train_step_adam_matches_torch(dev):
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _setup(dev, True)
  cfg = model.config
  cfg.optimizer = "adam"
  labels = torch.arange(x.shape[0], device=dev) % cr.CLASSES
  before = tu._flatten(variables["params"])
  ref_params = [p.detach().clone() for _, p in before]
  params, logits, inter, stats = _run_train(model, variables, x, rng=21)
  loss = tu.mse_loss(logits, labels) + 1e-4 * tu.weight_decay_fn(params)
  loss.backward()
  ref_grads = [(p.grad if p.grad is not None else torch.zeros_like(p)) for _, p in tu._flatten(params)]
  state = tu.create_train_state(variables, cfg, model)
  old_stats = {k: {n: t.clone() for n, t in s.items()} for k, s in state.batch_stats.items()}
  state, metrics, grads = tu.train_step(state, {"dvs_matrix": x, "label": labels}, 21,
                                        lambda step: 1e-3, 1e-4, 0.0, tu.mse_loss, return_grads=True)
  assert state.step == 1 and metrics["learning_rate"] == 1e-3
  for (path, g), rg in zip(tu._flatten(grads), ref_grads):
    assert torch.equal(g, rg), path
  leaves = [p.clone().requires_grad_(False) for p in ref_params]
  opt = torch.optim.Adam(leaves, lr=1e-3, eps=1e-8)
  for p, g in zip(leaves, ref_grads):
    p.grad = g.clone()
  opt.step()
  for (path, p), want in zip(tu._flatten(state.params["params"]), leaves):
    assert not p.requires_grad
    assert torch.equal(p, want), path
  # the step stored the running statistics the apply returned
  for k, s in stats.items():
    for n in ("mean", "var"):
      assert torch.equal(state.batch_stats[k][n], s[n]), (k, n)
      assert not torch.equal(state.batch_stats[k][n], old_stats[k][n]), (k, n)
  # and eval runs on the updated state
  new = tu.eval_step(state, {"dvs_matrix": x, "label": labels}, None, 0.0, tu.mse_loss)
  assert new["loss"].shape == () and bool(torch.isfinite(new["loss"]))


# ---- 6. it learns ----------------------------------------------------------------------------------

def test_twenty_steps_lower_the_loss(dev):
  """Twenty Adam steps on one fixed batch of 16 class-dependent samples (class c lights half c of
  the frame)."""
  from snnquantprune_amd import train_utils as tu
  model, v, variables, _ = _setup(dev, True)
  cfg = model.config
  cfg.optimizer = "adam"
  g = torch.Generator(device=dev)
  g.manual_seed(1234)
  B = 16
  labels = torch.arange(B, device=dev) % cr.CLASSES
  rates = torch.full((cr.CLASSES, cr.HW, cr.HW, cr.CIN), 0.1, device=dev)
  rates[0, :, :cr.HW // 2] = 0.8
  rates[1, :, cr.HW // 2:] = 0.8
  x = (torch.rand((B, cr.T_STEPS, cr.HW, cr.HW, cr.CIN), generator=g, device=dev)
       < rates[labels][:, None]).to(torch.uint8)
  state = tu.create_train_state(variables, cfg, model)
  losses = []
  for step in range(20):
    state, m = tu.train_step(state, {"dvs_matrix": x, "label": labels}, step, lambda s: 1e-2, 0.0, 0.0,
                             tu.mse_loss)
    losses.append(float(m["loss"]))
  print("losses", losses)
  assert np.isfinite(losses).all()
  assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
