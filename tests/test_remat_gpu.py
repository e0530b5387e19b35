"""ConvDenseSNN training with rematerialised blocks on the GPU (config.remat = W), on
the two-block fixture of tests/conv_train_reference.py at T = 6 with W in {1, 2, 4, 6, 7}: the
forward and every element-sized gradient are those of the call without the key bit for bit, the
parameter gradients are the float64 model's by the rule of DESIGN.md 11.4 and reproducible, a
window of a StreamState and train_step behave as without the key, it learns, and a block keeps no
image-sized float32 tensor between its forward and its backward."""
import numpy as np
import pytest
import torch

from tests import conv_train_reference as cr
from tests import neuron_train_reference as nr
from tests import remat_cases as rc
from tests.train_helpers import _grad_tree, _leaves, _np, _run_train

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
T = rc.MODEL_T
CASES = [(q, d) for q in (True, False) for d in ("uint8", "float32")]
_ids = ["%s-%s" % ("q4p90" if q else "float", d) for q, d in CASES]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


class _block0_gx:
  """While active, records the gradient block 1 hands to block 0: a hook on conv block 0's output."""

  def __enter__(self):
    from snnquantprune_amd import train_forward as fw
    self.fw, self.orig, self.got = fw, fw.conv_block, []

    def conv_block(mod, x, i, *a, **kw):
      y = self.orig(mod, x, i, *a, **kw)
      if i == 0:
        y.register_hook(lambda g: self.got.append(g.detach().clone()))
      return y

    fw.conv_block = conv_block
    return self.got

  def __exit__(self, *exc):
    self.fw.conv_block = self.orig


def _train(dev, quantized, dtype, W, neuron="msl", rng=11):
  """One training forward and backward -> dict; W None: without the key."""
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = rc.conv_setup(dev, quantized, dtype, neuron, remat=W)
  labels = torch.arange(x.shape[0], device=dev) % cr.CLASSES
  with _block0_gx() as gx:
    params, logits, inter, stats = _run_train(model, variables, x, rng=rng)
    tu.mse_loss(logits, labels).backward()
  torch.cuda.synchronize()
  assert len(gx) == 1
  return dict(model=model, v=v, x=x, logits=logits, inter=inter, stats=stats, labels=labels,
              grads=_grad_tree(params), gx=gx[0])


_runs = {}


def _run(dev, quantized, dtype, W, neuron="msl"):
  """Shared by the checks (nothing modifies it)."""
  key = (quantized, dtype, W, neuron)
  if key not in _runs:
    _runs[key] = _train(dev, quantized, dtype, W, neuron)
  return _runs[key]


def _same_bits(a, b):
  assert set(a) == set(b)
  for path, g in a.items():
    if g is None:
      assert b[path] is None, path
    else:
      assert b[path] is not None and g.tobytes() == b[path].tobytes(), path


# ---- 1. forward and element-sized gradients ----------------------------------------------------------

@pytest.mark.parametrize("quantized,dtype", CASES, ids=_ids)
def test_forward_and_element_gradients_are_the_call_without_the_key(dev, quantized, dtype):
  base = _run(dev, quantized, dtype, None)
  names = {"dropout_0", "dense_h", "dense_out"}
  for i in range(cr.NBLOCKS):
    names |= {"conv%d_h" % i, "conv%d_out" % i, "bn%d_mean" % i, "bn%d_var" % i}
    rate = float(_np(base["inter"]["conv%d_out" % i]).mean())
    assert 0.02 <= rate <= 0.30, rate
  assert set(base["inter"]) >= names
  assert bool(base["gx"].abs().max() > 0)
  for W in rc.MODEL_W:
    r = _run(dev, quantized, dtype, W)
    assert torch.equal(r["logits"], base["logits"]), W
    assert set(r["inter"]) == set(base["inter"])
    for n, t in base["inter"].items():
      assert r["inter"][n].shape == t.shape and torch.equal(r["inter"][n], t), (W, n)
    for name, leaf in base["stats"].items():
      for k, t in leaf.items():
        assert torch.equal(r["stats"][name][k], t), (W, name, k)
    assert r["gx"].shape == base["gx"].shape and torch.equal(r["gx"], base["gx"]), W
    if W >= T:                                           # one chunk: every reduction is the plain call's
      _same_bits(r["grads"], base["grads"])


# ---- 2. parameter gradients against float64 ----------------------------------------------------------

def _check_against_float64(m, r, quantized):
  """The rule of tests/test_conv_train_gpu.py: relative L2 1e-5 for every
  parameter; DuQ's c of a conv layer, whose gradient BatchNorm cancels to rounding, inside the
  element-wise gamma bound of the weight gradient's chain where it misses the relative figure."""
  got, worst = r["grads"], 0.0
  for (layer, name), want in m.grads().items():
    path = (layer, name) if name in ("scale", "bias", "tau") else (
        (layer, "kernel") if name == "kernel" else (layer, "DuQ_0", name))
    g = got[path]
    if name in ("a", "c") and not quantized:
      assert g is None or np.abs(g).max() == 0.0
      continue
    assert g is not None and np.abs(g).max() > 0, path
    rel = float(np.linalg.norm(g.astype(F64).reshape(want.shape) - want) / np.linalg.norm(want))
    print("%-28s relative L2 %.3g" % ("/".join(path), rel))
    if rel > 1e-5 and name == "c" and layer.startswith("QuantConv"):
      bound = m.c_gamma_bound(int(layer.split("_")[1]))
      err = float(np.abs(g.astype(F64) - want).max())
      print("%-28s |got - ref| %.3g, gamma bound %.3g" % ("/".join(path), err, bound))
      assert err <= bound, (path, err, bound)
      continue
    worst = max(worst, rel)
    assert rel <= 1e-5, (path, rel)
  return worst


def _float64_model(r, m):
  from snnquantprune_amd import train_utils as tu
  inter = r["inter"]
  saved = {"hd": _np(inter["dense_h"]), "sd": _np(inter["dense_out"])}
  for i in range(cr.NBLOCKS):
    saved["h%d" % i], saved["s%d" % i] = _np(inter["conv%d_h" % i]), _np(inter["conv%d_out" % i])
  lg = m.forward(_np(r["x"]), _np(inter["dropout_0"]), saved)
  np.testing.assert_allclose(lg.detach().numpy(), _np(r["logits"]).astype(F64), rtol=1e-6, atol=1e-7)
  assert m.h_gap < 1e-4, m.h_gap
  tu.mse_loss(lg, _np(r["labels"])).backward()
  return m


@pytest.mark.parametrize("quantized,dtype", CASES, ids=_ids)
def test_parameter_gradients_match_float64_and_repeat(dev, quantized, dtype):
  """For every W: within relative L2 1e-5 of TorchConvDenseSNN64 (the forward is the same for
  every W, test 1, so one float64 backward serves them all); a second run gives the same bits."""
  m = _float64_model(_run(dev, quantized, dtype, None), cr.TorchConvDenseSNN64(
      _run(dev, quantized, dtype, None)["v"]["params"]))
  for W in rc.MODEL_W:
    r = _run(dev, quantized, dtype, W)
    print("W = %d: worst relative L2 %.3g" % (W, _check_against_float64(m, r, quantized)))
    _same_bits(_train(dev, quantized, dtype, W)["grads"], r["grads"])


def test_plif_tau_gradient_under_learn_neuron_params(dev):
  """W = 2 with PLIF: the unfused scans chunk by chunk; every parameter gradient and `tau` by the
  same rule; the forward is the call's without the key."""
  base, r = _run(dev, True, "uint8", None, "plif"), _run(dev, True, "uint8", 2, "plif")
  assert torch.equal(r["logits"], base["logits"]) and torch.equal(r["gx"], base["gx"])
  for n, t in base["inter"].items():
    assert torch.equal(r["inter"][n], t), n
  m = _float64_model(r, nr.TorchConvDenseSNN64Neuron(nr.PLIF, r["v"]["params"]))
  taus = [p for p in r["grads"] if p[-1] == "tau"]
  assert len(taus) == cr.NBLOCKS + 1 and all(r["grads"][p] is not None for p in taus)
  print("worst relative L2 %.3g" % _check_against_float64(m, r, True))
  _same_bits(_train(dev, True, "uint8", 2, "plif")["grads"], r["grads"])
  # one chunk: the parameter sums are the plain call's
  _same_bits(_train(dev, True, "uint8", T, "plif")["grads"], base["grads"])


# ---- 3. a window of a StreamState -------------------------------------------------------------------------

def test_a_window_of_a_stream_state_with_the_key(dev):
  """Two windows (2 steps, then 4: with W = 3 a ragged chunk inside the window): after each the
  state, the logits and the sown values, and for the second the gx into block 0, are those of the
  same windows without the key."""
  from snnquantprune_amd import models
  from snnquantprune_amd import train_utils as tu
  out = []
  for W in (None, 3):
    model, v, variables, x = rc.conv_setup(dev, True, "uint8", remat=W)
    labels = torch.arange(x.shape[0], device=dev) % cr.CLASSES
    state, got = models.StreamState(), []
    for t0, t1 in ((0, 2), (2, 6)):
      params = _leaves(variables["params"])
      with _block0_gx() as gx:
        (logits, st), mut = model.apply({"params": params, "batch_stats": variables["batch_stats"]}, x[:, t0:t1],
                                        train=True, rng=5, u_state=state, mutable=["intermediates", "batch_stats"])
        assert st is state
        tu.mse_loss(logits, labels).backward()
      got.append(dict(logits=logits, inter={k: t[0] for k, t in mut["intermediates"].items()}, gx=gx[0],
                      state=[t.clone() for t in state._tensors()], steps=state.steps,
                      grads=_grad_tree(params)))
    out.append(got)
  for a, b in zip(*out):
    assert a["steps"] == b["steps"] and torch.equal(a["logits"], b["logits"])
    assert len(a["state"]) == len(b["state"]) and all(torch.equal(s, t) for s, t in zip(a["state"], b["state"]))
    assert any(bool(s.any()) for s in a["state"])
    for n, t in a["inter"].items():
      assert torch.equal(b["inter"][n], t), n
    assert torch.equal(a["gx"], b["gx"])
  _same_bits(out[0][0]["grads"], out[1][0]["grads"])         # the first window is one chunk of W = 3


# ---- 4. train_step ------------------------------------------------------------------------------------------

def _step(dev, W, return_grads=False):
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = rc.conv_setup(dev, True, "uint8", remat=W)
  model.config.optimizer = "adam"
  labels = torch.arange(x.shape[0], device=dev) % cr.CLASSES
  state = tu.create_train_state(variables, model.config, model)
  return tu.train_step(state, {"dvs_matrix": x, "label": labels}, 21, lambda step: 1e-3, 1e-4, 0.0, tu.mse_loss,
                       return_grads=return_grads)


def test_train_step_equals_the_step_without_the_key(dev):
  """W = 6: the parameters after one Adam step, bit for bit.  W = 2: the gradients -- Adam's first
  step is sign(g) at small |g|, which would amplify an order-of-summation difference near zero --
  equal behind the conv blocks, where no reduction is chunked; elsewhere within relative L2 2e-5:
  both sides are held to 1e-5 of the float64 model (test 2), so they are that close to each other
  (DuQ's c of a conv layer, which cancels to rounding, has its own rule there and none here)."""
  from snnquantprune_amd import train_utils as tu
  base, _, base_grads = _step(dev, None, True)
  one, metrics = _step(dev, 6)
  assert one.step == 1
  for (path, p), (_, want) in zip(tu._flatten(one.params["params"]), tu._flatten(base.params["params"])):
    assert torch.equal(p, want), path
  for k, s in base.batch_stats.items():
    for n in ("mean", "var"):
      assert torch.equal(one.batch_stats[k][n], s[n]), (k, n)
  two, _, grads = _step(dev, 2, True)
  for (path, g), (_, want) in zip(tu._flatten(grads), tu._flatten(base_grads)):
    if path[0] == "QuantDense_0":                        # behind the conv blocks: no chunked reduction
      assert torch.equal(g, want), path
    elif float(want.abs().max()) > 0 and path[-1] != "c":
      rel = float((g.double() - want.double()).norm() / want.double().norm())
      print("%-28s relative L2 %.3g" % ("/".join(path), rel))
      assert rel <= 2e-5, (path, rel)


def test_twenty_steps_lower_the_loss(dev):
  """tests/test_conv_train_gpu.py's twenty Adam steps on one fixed batch of 16 class-dependent
  samples, at W = 2."""
  from snnquantprune_amd import train_utils as tu
  model, v, variables, _ = rc.conv_setup(dev, True, "uint8", remat=2)
  cfg = model.config
  cfg.optimizer = "adam"
  g = torch.Generator(device=dev)
  g.manual_seed(1234)
  B = 16
  labels = torch.arange(B, device=dev) % cr.CLASSES
  rates = torch.full((cr.CLASSES, cr.HW, cr.HW, cr.CIN), 0.1, device=dev)
  rates[0, :, :cr.HW // 2] = 0.8
  rates[1, :, cr.HW // 2:] = 0.8
  x = (torch.rand((B, T, cr.HW, cr.HW, cr.CIN), generator=g, device=dev) < rates[labels][:, None]).to(torch.uint8)
  state = tu.create_train_state(variables, cfg, model)
  losses = []
  for step in range(20):
    state, m = tu.train_step(state, {"dvs_matrix": x, "label": labels}, step, lambda s: 1e-2, 0.0, 0.0, tu.mse_loss)
    losses.append(float(m["loss"]))
  print("losses", losses)
  assert np.isfinite(losses).all()
  assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses


# ---- 5. what a block keeps ---------------------------------------------------------------------------------

def _forward_growth(dev, W):
  """memory_allocated() after the training forward minus before it, with the logits alive."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  C, HW, B, steps = 32, 32, 2, 8
  v = syn.conv_net_variables(C, 2, 2, HW, 20, True, 0.9, gains=(4.0, 5.0, 8.0), random_bn=True)
  extra = {} if W is None else {"remat": W}
  cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=C, num_conv_blocks=2, dropout=0.9, **extra)
  model = models.ConvDenseSNN(num_classes=2, config=cfg)
  variables = nn.tree_from_numpy(v, dev)
  rng = np.random.default_rng(3)
  x = torch.from_numpy(np.minimum(rng.poisson(0.6, (B, steps, HW, HW, 2)), 255).astype(np.uint8)).to(dev)
  params = _leaves(variables["params"])
  model.apply({"params": params, "batch_stats": variables["batch_stats"]}, x, train=True, rng=1)   # packs, warms up
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()
  logits, _ = model.apply({"params": params, "batch_stats": variables["batch_stats"]}, x, train=True, rng=1)
  torch.cuda.synchronize()
  growth = torch.cuda.memory_allocated() - before
  logits.sum().backward()                                # (and the graph is whole)
  assert all(p.grad is not None for p in (params["QuantConv_0"]["kernel"], params["BatchNorm_1"]["scale"]))
  return growth


def test_a_block_keeps_no_image_sized_float32_tensor(dev):
  """Two blocks of 32 channels on 32 x 32 frames, B = 2, T = 8.  Without the key a block keeps cur
  and h, [8, 2, 32, 32, 32] and [8, 2, 16, 16, 32] float32 each, and block 1 its float32 input:
  about 5.5 MB.  With remat = 2: three boundary membranes per block, 0.98 MB, the packed input of
  block 1 (16 KB) and the frames; the read-out's residuals (0.13 MB and its scan's) are the same on
  both sides -- about 1.3 MB, a ratio near 0.25.  The cap of one half is a condition, not a
  measurement: it leaves room for the allocator's rounding and fails if cur or h of either block
  survives the forward (2 MB or 0.5 MB each)."""
  plain = _forward_growth(dev, None)
  remat = _forward_growth(dev, 2)
  print("kept after the forward: %.3f MB without the key, %.3f MB with remat = 2, ratio %.3f"
        % (plain / 1e6, remat / 1e6, remat / plain))
  assert plain > 4.5e6, plain
  assert remat <= 0.5 * plain, (remat, plain)
