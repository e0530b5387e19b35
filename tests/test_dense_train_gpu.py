"""DenseSNN training on the GPU: the training forward against the eval forward and the oracle,
and the HIP backward against a float64 statement of the reference's VJP rules applied to the
saved float32 forward values (h, s, masks, kernel_fwd)."""
from functools import partial

import numpy as np
import pytest
import torch

from tests import cases
from tests.helpers import qweight_of

pytestmark = pytest.mark.gpu

F64 = np.float64


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _np(t):
  return t.detach().cpu().numpy()


def _setup(dev, quantized=True, T=6, B=4, K=256, hidden=96, out=110, tau=2.0, v_reset=0.0,
           surrogate="atan", counts=False, dropout=1.0, seed=941):
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
                                v_reset=v_reset)
  model = models.DenseSNN(num_classes=out // 10, config=cfg)
  return model, v, nn.tree_from_numpy(v, dev), torch.from_numpy(x).to(dev)


def _leaves(variables):
  return {k: {kk: ({kkk: t.detach().clone().requires_grad_(True) for kkk, t in vv.items()}
                   if isinstance(vv, dict) else vv.detach().clone().requires_grad_(True))
              for kk, vv in leaf.items()}
          for k, leaf in variables["params"].items()}


def _run_train(model, variables, x, rng=0):
  params = _leaves(variables)
  (logits, _), mut = model.apply({"params": params, "batch_stats": {}}, x, train=True, rng=rng,
                                 mutable=["intermediates"])
  return params, logits, {k: v[0] for k, v in mut["intermediates"].items()}


def _dense(s):
  return s.to_dense() if hasattr(s, "to_dense") else s


# ---- float64 yardstick -------------------------------------------------------------------------

def _sg(name, x):                               # spiking_learning.py:139-241
  if name == "fast_sigmoid":
    return 1.0 / (10.0 * np.abs(x) + 1.0) ** 2
  if name == "atan":
    return 1.0 / (1.0 + (np.pi * x) ** 2)
  if name == "slayer":
    return np.exp(-5.0 * np.abs(x))
  if name == "smooth_step":
    return ((x < 0.5) & (x >= -0.5)).astype(F64)
  return np.maximum(1.0 - 2.0 * np.abs(x), 0.0)


def _scan_vjp(h, s, gs, tau, vth, name):
  """spiking_learning.py:410-414 differentiated: no gradient through the reset condition."""
  T = h.shape[0]
  gI = np.zeros_like(gs)
  gu = np.zeros_like(gs[0])
  for t in range(T - 1, -1, -1):
    gh = gs[t] * _sg(name, h[t].astype(F64) - vth) + gu * (1.0 - s[t])
    gI[t] = gh / tau
    gu = gh * (1.0 - 1.0 / tau)
  return gI


def _duq_vjp(g, leaf, bits, quantized):
  """quant.py:428-491: prune's grad_zero, DuQ with a straight-through round."""
  w = leaf["kernel"].astype(F64)
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  mask = leaf.get("prune_0", {}).get("mask")
  if mask is not None:
    g = g * mask
  if not quantized or a == -1.0:
    return g, 0.0, 0.0
  L = 2 ** (bits - 1) - 1
  x = leaf["kernel"] / np.float32(a)
  inside = np.abs(x.astype(F64)) <= 1
  r = np.round(np.clip(x, -1, 1) * np.float32(L)).astype(F64) / L
  gc = float((g * r).sum())
  gw = np.where(inside, g * c / a, 0.0)
  ga = float(-np.where(inside, g * c * w / (a * a), 0.0).sum())
  return gw, ga, gc


def _yardstick(v, x_bt, inter, logits, labels, loss, tau, vth, name, quantized, o):
  p = v["params"]
  lg = torch.from_numpy(_np(logits).astype(F64)).requires_grad_(True)
  from snnquantprune_amd import train_utils as tu
  loss(lg, torch.from_numpy(labels)).backward()
  gL = lg.grad.numpy()
  m0, m1 = _np(inter["dropout_0"]).astype(F64), _np(inter["dropout_1"]).astype(F64)
  h1, h2 = _np(inter["dense1_h"]), _np(inter["dense2_h"])
  s1, s2 = _np(inter["dense1_out"]).astype(F64), _np(_dense(inter["dense2_out"])).astype(F64)
  T, B, N = s2.shape
  gs2 = np.repeat(gL, 10, axis=1)[None].repeat(T, 0) / (10 * T)       # models.py:253-255
  gI2 = _scan_vjp(h2, s2, gs2, tau, vth, name)
  x1 = s1 * m1
  gwq2 = np.einsum("tbk,tbn->kn", x1, gI2)
  wq2 = qweight_of(o, p["QuantDense_1"], 8, quantized).w_fq.astype(F64)
  gs1 = np.einsum("tbn,kn->tbk", gI2, wq2) * m1
  gI1 = _scan_vjp(h1, s1, gs1, tau, vth, name)
  x0 = np.swapaxes(x_bt.astype(F64) * m0, 0, 1)
  gwq1 = np.einsum("tbk,tbn->kn", x0, gI1)
  out = {}
  for i, g in ((0, gwq1), (1, gwq2)):
    gw, ga, gc = _duq_vjp(g, p["QuantDense_%d" % i], 8, quantized)
    out[i] = (gw, ga, gc)
  return out


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
  name = case.get("surrogate", "atan")
  model, v, variables, x = _setup(dev, quantized, dropout=0.8, **case)
  loss = tu.mse_loss if loss_name == "mse" else tu.cross_entropy_loss
  B = x.shape[0]
  labels = (np.arange(B) * 7 % (model.num_classes)).astype(np.int64)
  params, logits, inter = _run_train(model, variables, x, rng=11)
  loss(logits, torch.from_numpy(labels).to(dev)).backward()
  torch.cuda.synchronize()
  got = _grads(params)
  ref = _yardstick(v, _np(x), inter, logits, labels, loss, tau, 1.0, name, quantized, oracle)
  for i in (0, 1):
    _close(got[i][0], ref[i][0], "kernel %d" % i)
    _close(got[i][1], ref[i][1], "a %d" % i)
    _close(got[i][2], ref[i][2], "c %d" % i)
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
