"""DenseSNN training on the GPU: the training forward against the eval forward and the oracle,
and the HIP backward against two float64 yardsticks fed the saved float32 forward values (h, s,
masks): the reference's VJP rules written out by hand, and torch.autograd on the literal forward
(tests/train_reference.py; tests/test_train_reference_cpu.py holds the two to each other)."""
from functools import partial

import numpy as np
import pytest
import torch

from tests import cases
from tests import train_reference as tr
from tests.helpers import qweight_of
from tests.train_helpers import _np, _run_train as _run_train_stats
from tests.train_reference import duq_vjp as _duq_vjp, scan_vjp as _scan_vjp  # noqa: F401

pytestmark = pytest.mark.gpu

F64 = np.float64
_run_train = partial(_run_train_stats, batch_stats=False)     # -> (params, logits, sown values)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _setup(dev, quantized=True, T=6, B=4, K=256, hidden=96, out=110, tau=2.0, v_reset=0.0,
           surrogate="atan", counts=False, dropout=1.0, seed=941, v_threshold=1.0):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, spiking_learning as sl, synthetic as syn
  v = syn.dense_net_variables(K, hidden, out, quantized, 0.5 if quantized else -1.0)
  if counts:
    x = syn.poisson_counts((B, T, K), 0.5, seed=seed)
  else:
    x = syn.poisson_spikes((B, T, K), 0.2, seed=seed)
  cfg = syn.make_config(bits=8, prune_percentage=0.5 if quantized else -1.0, hidden=hidden,
                        dropout=dropout)
  cfg.neuron_dynamics = partial(sl.multi_step_LIF, spike_fn=getattr(sl, surrogate), tau=tau,
                                v_reset=v_reset, v_threshold=v_threshold)
  model = models.DenseSNN(num_classes=out // 10, config=cfg)
  return model, v, nn.tree_from_numpy(v, dev), torch.from_numpy(x).to(dev)


def _dense(s):
  return s.to_dense() if hasattr(s, "to_dense") else s


# ---- float64 yardstick -------------------------------------------------------------------------

def _saved(x_bt, inter):
  """The forward's saved values as tr.hand_gradients / tr.TorchDenseSNN64.forward take them."""
  return (x_bt, _np(inter["dropout_0"]), _np(inter["dropout_1"]), _np(inter["dense1_h"]),
          _np(inter["dense1_out"]), _np(inter["dense2_h"]), _np(_dense(inter["dense2_out"])))


def _yardstick(v, x_bt, inter, logits, labels, loss, tau, vth, name, quantized, o):
  p = v["params"]
  lg = torch.from_numpy(_np(logits).astype(F64)).requires_grad_(True)
  loss(lg, torch.from_numpy(labels)).backward()
  wq2 = qweight_of(o, p["QuantDense_1"], 8, quantized).w_fq.astype(F64)
  return tr.hand_gradients(p, *_saved(x_bt, inter), lg.grad.numpy(), wq2, tau, vth, name,
                           quantized)


def _autograd_yardstick(v, x_bt, inter, logits, labels, loss, tau, vth, vr, name):
  """The same gradients by torch.autograd on the literal float64 forward."""
  m = tr.TorchDenseSNN64(v["params"], tau, vth, vr, name)
  lg = m.forward(*_saved(x_bt, inter))
  np.testing.assert_allclose(lg.detach().numpy(), _np(logits).astype(F64), rtol=1e-6, atol=1e-7)
  loss(lg, torch.from_numpy(labels)).backward()
  return m.grads()


def _close(got, ref, what):
  got, ref = np.asarray(got, F64).reshape(-1), np.asarray(ref, F64).reshape(-1)
  scale = np.abs(ref).max()
  if scale == 0:
    assert np.abs(got).max() == 0, what
    return
  rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
  assert rel <= 1e-5, "%s: relative L2 %.3g" % (what, rel)
  assert np.abs(got - ref).max() <= 1e-4 * scale, "%s: max abs %.3g of %.3g" % (
      what, np.abs(got - ref).max(), scale)


# ---- 1. training forward == eval forward at dropout 1 ------------------------------------------

@pytest.mark.parametrize("quantized", [False, True], ids=["c1", "c2"])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_train_forward_bit_equal_eval(dev, quantized, dtype):
  model, v, variables, x = _setup(dev, quantized)
  if dtype == "float32":
    x = x.to(torch.float32)
  (want, _), mut = model.apply(variables, x, train=False, rng=None, mutable=["intermediates"])
  want_s2 = _np(_dense(mut["intermediates"]["dense2_out"][0])).astype(np.float32)
  _, logits, inter = _run_train(model, variables, x, rng=3)
  assert np.array_equal(_np(logits), _np(want))
  assert np.array_equal(_np(inter["dense2_out"]), want_s2)
  assert float(_np(inter["dropout_0"]).min()) == 1.0 and float(_np(inter["dropout_1"]).min()) == 1.0


# ---- 2. saved h and s against the oracle -------------------------------------------------------

@pytest.mark.parametrize("quantized", [False, True], ids=["c1", "c2"])
def test_saved_state_bit_equal_oracle(dev, oracle, quantized):
  model, v, variables, x = _setup(dev, quantized, tau=3.0, v_reset=0.1, dropout=0.8)
  _, _, inter = _run_train(model, variables, x, rng=5)
  p = v["params"]
  mode = "int" if quantized else "fseq"
  x0 = np.swapaxes(_np(x).astype(np.float32) * _np(inter["dropout_0"]), 0, 1)
  for i, (xin, hk, sk) in enumerate(((x0, "dense1_h", "dense1_out"), (None, "dense2_h", "dense2_out"))):
    if xin is None:
      xin = _np(inter["dense1_out"]) * _np(inter["dropout_1"])
    cur = oracle.quant_dense(xin, qweight_of(oracle, p["QuantDense_%d" % i], 8, quantized), mode)
    u = np.zeros(cur.shape[1:], np.float32)
    hs, ss = [], []
    for t in range(cur.shape[0]):
      tau, vr = np.float32(3.0), np.float32(0.1)
      hs.append((u + (cur[t] - (u - vr)) / tau).astype(np.float32))
      u, s = oracle.multi_step_lif(u, cur[t], tau=3.0, v_reset=0.1)
      ss.append(s)
    assert np.array_equal(_np(inter[hk]), np.stack(hs)), hk
    assert np.array_equal(_np(inter[sk]), np.stack(ss).astype(np.float32)), sk


# ---- 3. gradients against the float64 yardstick ------------------------------------------------

GRID = [
    dict(surrogate=s) for s in ("fast_sigmoid", "atan", "slayer", "smooth_step", "piecewise_linear")
] + [
    dict(tau=3.0), dict(v_reset=0.1, tau=3.0), dict(loss="ce"), dict(quantized=False),
    dict(counts=True, loss="ce"),
    dict(K=100, hidden=96, out=110, B=7, T=5, surrogate="fast_sigmoid"),
    dict(K=2048, hidden=512, out=110, B=64, T=20, loss="ce", counts=True),
    dict(v_threshold=0.7), dict(v_threshold=0.7, tau=3.0, surrogate="smooth_step"),
    dict(dropout=1.0), dict(T=1), dict(T=1, surrogate="piecewise_linear", loss="ce"),
    dict(hidden=100, out=30, B=3, T=7), dict(quantized=False, v_reset=0.1),
]


def _gid(c):
  return "-".join("%s=%s" % kv for kv in sorted(c.items()))


def _grads(params):
  out = {}
  for i in (0, 1):
    leaf = params["QuantDense_%d" % i]
    out[i] = (_np(leaf["kernel"].grad), float(_np(leaf["DuQ_0"]["a"].grad)[0]),
              float(_np(leaf["DuQ_0"]["c"].grad)[0]),
              None if "prune_0" not in leaf else leaf["prune_0"]["mask"].grad)
  return out


@pytest.mark.parametrize("case", GRID, ids=_gid)
def test_gradients_match_yardstick(dev, oracle, case):
  from snnquantprune_amd import train_utils as tu
  case = dict(case)
  loss_name = case.pop("loss", "mse")
  quantized = case.pop("quantized", True)
  tau, vr = case.get("tau", 2.0), case.get("v_reset", 0.0)
  vth = case.get("v_threshold", 1.0)
  name = case.get("surrogate", "atan")
  case.setdefault("dropout", 0.8)
  model, v, variables, x = _setup(dev, quantized, **case)
  loss = tu.mse_loss if loss_name == "mse" else tu.cross_entropy_loss
  B = x.shape[0]
  labels = (np.arange(B) * 7 % (model.num_classes)).astype(np.int64)
  params, logits, inter = _run_train(model, variables, x, rng=11)
  loss(logits, torch.from_numpy(labels).to(dev)).backward()
  torch.cuda.synchronize()
  got = _grads(params)
  if case["dropout"] == 1.0:
    assert float(_np(inter["dropout_1"]).min()) == 1.0
  assert 0.01 < float(_np(inter["dense1_out"]).mean()) < 0.99            # a layer that spikes
  ref = _yardstick(v, _np(x), inter, logits, labels, loss, tau, vth, name, quantized, oracle)
  auto = _autograd_yardstick(v, _np(x), inter, logits, labels, loss, tau, vth, vr, name)
  for i in (0, 1):
    for what, yard in (("hand", ref), ("autograd", auto)):
      _close(got[i][0], yard[i][0], "kernel %d (%s)" % (i, what))
      _close(got[i][1], yard[i][1], "a %d (%s)" % (i, what))
      _close(got[i][2], yard[i][2], "c %d (%s)" % (i, what))
    if got[i][3] is not None:
      assert float(got[i][3].abs().max()) == 0.0


# ---- 4. reproducible -----------------------------------------------------------------------------

def test_backward_bitwise_reproducible(dev):
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _setup(dev, True, K=512, hidden=256, B=32, T=8, dropout=0.9, counts=True)
  labels = torch.arange(32, device=dev) % model.num_classes
  runs = []
  for _ in range(2):
    params, logits, _ = _run_train(model, variables, x, rng=7)
    tu.cross_entropy_loss(logits, labels).backward()
    runs.append(_grads(params))
  for i in (0, 1):
    assert np.array_equal(runs[0][i][0], runs[1][i][0])
    assert runs[0][i][1] == runs[1][i][1] and runs[0][i][2] == runs[1][i][2]


# ---- 5. one Adam step ----------------------------------------------------------------------------

def test_train_step_adam_matches_torch(dev, oracle):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _setup(dev, True, dropout=0.9)
  cfg = model.config
  cfg.optimizer = "adam"
  B = x.shape[0]
  labels = torch.arange(B, device=dev) % model.num_classes
  before = tu._flatten(variables["params"])
  ref_params = [p.detach().clone() for _, p in before]
  # the step's gradients, stated independently by the model's backward on copies
  params, logits, _ = _run_train(model, variables, x, rng=21)
  loss = tu.mse_loss(logits, labels) + 1e-4 * tu.weight_decay_fn(params)
  loss.backward()
  ref_grads = [(p.grad if p.grad is not None else torch.zeros_like(p))
               for _, p in tu._flatten(params)]
  # eval once first, so that the packed caches hold the old weights
  (old, _) = model.apply(variables, x, train=False, rng=None)
  state = tu.create_train_state(variables, cfg, model)
  state, metrics, grads = tu.train_step(state, {"dvs_matrix": x, "label": labels}, 21,
                                        lambda step: 1e-3, 1e-4, 0.0, tu.mse_loss,
                                        return_grads=True)
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
  # after the in-place update, eval sees the new weights: same logits as a fresh tree
  new = tu.eval_step(state, {"dvs_matrix": x, "label": labels}, None, 0.0, tu.mse_loss)
  fresh = nn.tree_from_numpy(tu._unflatten([(path, p.cpu().numpy()) for path, p in
                                            tu._flatten(state.params["params"])]), dev)
  (want, _) = model.apply({"params": fresh, "batch_stats": {}}, x, train=False, rng=None)
  (got, _) = model.apply(variables, x, train=False, rng=None)
  assert torch.equal(got, want)
  assert not torch.equal(got, old)
  assert new["loss"].shape == ()


# ---- 6. it learns --------------------------------------------------------------------------------

def test_fifty_steps_lower_the_loss(dev):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import train_utils as tu
  from snnquantprune_amd import synthetic as syn
  model, v, variables, _ = _setup(dev, True, K=128, hidden=160, out=40, T=10, B=64, dropout=0.9)
  cfg = model.config
  cfg.optimizer = "adam"
  g = torch.Generator(device=dev)
  g.manual_seed(1234)
  C, K, T = 4, 128, 10
  rates = torch.full((C, K), 0.05, device=dev)
  for c in range(C):
    rates[c, c * 32:(c + 1) * 32] = 0.5                       # class-dependent Poisson rates
  state = tu.create_train_state(variables, cfg, model)
  losses = []
  for step in range(50):
    labels = torch.randint(0, C, (64,), generator=g, device=dev)
    x = (torch.rand((64, T, K), generator=g, device=dev) < rates[labels][:, None, :]).to(torch.uint8)
    state, m = tu.train_step(state, {"dvs_matrix": x, "label": labels}, step, lambda s: 1e-2, 0.0,
                             0.0, tu.cross_entropy_loss)
    losses.append(float(m["loss"]))
  assert np.isfinite(losses).all()
  assert np.mean(losses[-10:]) < 0.8 * np.mean(losses[:10]), losses
