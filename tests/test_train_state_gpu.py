"""DenseSNN and ConvDenseSNN training over windows of a recording on the GPU, on the
fixtures of tests/train_state_cases.py: the windowed training forward against the whole-run one bit
for bit, every window's gradients against the float64 models that start from constant membranes
(tests/train_state_reference.py), two windows chained through autograd at block level, the dropout
masks, train_step(u_state=) and train_step_windows."""
import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from tests import conv_train_reference as cr
from tests import train_reference as tr
from tests import train_state_cases as sc
from tests import train_state_reference as sr
from tests.train_helpers import _grad_tree, _leaves, _np

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
T = sc.MODEL_T
MODELS = [("dense", True, "msl"), ("dense", False, "msl"), ("dense", True, "plif"),
          ("conv", True, "msl"), ("conv", False, "msl"), ("conv", True, "plif")]
_mids = ["%s-%s-%s" % (m, "quant" if q else "float", n) for m, q, n in MODELS]
GRAD_MODELS = [m for m in MODELS if m != ("dense", True, "plif")]      # (no float64 DenseSNN with PLIF)
_gids = ["%s-%s-%s" % (m, "quant" if q else "float", n) for m, q, n in GRAD_MODELS]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _setup(dev, which, quantized, neuron, **kw):
  fn = sc.dense_setup if which == "dense" else sc.conv_setup
  return fn(dev, quantized, neuron, **kw)


def _blocks(which):
  """[(name of the sown h, of the sown spikes)] in model order."""
  if which == "dense":
    return [("dense1_h", "dense1_out"), ("dense2_h", "dense2_out")]
  return [("conv%d_h" % i, "conv%d_out" % i) for i in range(cr.NBLOCKS)] + [("dense_h", "dense_out")]


def _apply(model, params, stats, x, rng, state=None):
  """One training forward -> (logits, returned state, sown values, new batch_stats)."""
  kw = {} if state is None else {"u_state": state}
  (logits, st), mut = model.apply({"params": params, "batch_stats": stats}, x, train=True, rng=rng,
                                  mutable=["intermediates", "batch_stats"], **kw)
  inter = {k: v[0] for k, v in mut.get("intermediates", {}).items()}
  return logits, st, inter, mut.get("batch_stats", stats)


def _stats_of(variables):
  return variables.get("batch_stats", {})


_whole = {}


def _whole_run(dev, key):
  """The whole-run training forward of a model case, shared (nothing modifies it)."""
  if key not in _whole:
    model, v, variables, x = _setup(dev, *key)
    logits, st, inter, stats = _apply(model, variables["params"], _stats_of(variables), x, 3)
    assert st is None
    _whole[key] = dict(model=model, v=v, variables=variables, x=x, logits=logits, inter=inter, stats=stats)
  return _whole[key]


# ---- 1. the windowed forward is the whole-run forward --------------------------------------------------

@pytest.mark.parametrize("key", MODELS, ids=_mids)
def test_windowed_training_forward_is_the_whole_run(dev, key):
  """For every split and every sown tensor (h, spikes, per-step statistics): the windows'
  concatenation is the whole run's, bit for bit; so are the running statistics, the state's
  membranes (the carried state of the last h) and its vote.  In every window after the first a
  fresh state gives other spikes in every block: the equality cannot hold for scans from zero."""
  from snnquantprune_amd import models
  w = _whole_run(dev, key)
  model, variables, x, inter = w["model"], w["variables"], w["x"], w["inter"]
  blocks = _blocks(key[0])
  names = [n for pair in blocks for n in pair] + [n for n in inter if n.startswith("bn")]
  for _, sname in blocks:
    rate = float(_np(inter[sname]).mean())
    assert 0.02 <= rate <= 0.30, (sname, rate)
  vth, vr = 1.0, 0.0
  for split in sc.MODEL_SPLITS:
    state, stats = models.StreamState(), _stats_of(variables)
    got = {n: [] for n in names}
    for t0, t1 in sr.windows(T, split):
      xw = x[:, t0:t1]
      before = state.clone()
      logits, st, wi, stats = _apply(model, variables["params"], stats, xw, 3, state)
      assert st is state and tuple(logits.shape) == tuple(w["logits"].shape)
      if t1 == t0:
        assert not wi and not _np(logits).any()
        if before.counts is not None:
          assert all(torch.equal(a, b) for a, b in zip(before._tensors(), state._tensors()))
        continue
      for n in names:
        got[n].append(wi[n])
      # the window's logits are the vote over the window
      s_out = wi[blocks[-1][1]]
      want = s_out.mean(0).reshape(s_out.shape[1], -1, 10).mean(-1)
      np.testing.assert_allclose(_np(logits), _np(want), rtol=1e-6, atol=1e-7)
      if t0 > 0:
        _, _, fresh, _ = _apply(model, variables["params"], stats, xw, 3, models.StreamState())
        for _, sname in blocks:
          assert not torch.equal(fresh[sname], wi[sname]), (split, t0, sname)
    for n in names:
      assert torch.equal(torch.cat(got[n]), inter[n]), (split, n)
    for name, leaf in w["stats"].items():
      for k, t in leaf.items():
        assert torch.equal(stats[name][k], t), (split, name, k)
    for u, (hname, _) in zip(state.membranes, blocks):
      np.testing.assert_array_equal(_np(u), sr.last_state(_np(inter[hname]), vth, vr).reshape(u.shape))
    assert state.steps == T and torch.equal(state.logits(), w["logits"]), split


# ---- 2. every window's gradients against float64 ---------------------------------------------------------

def _rel(got, want):
  return float(np.linalg.norm(np.asarray(got, F64) - want) / np.linalg.norm(want))


def _check_dense(w, params, xw, wi, u0s, logits, labels, quantized):
  from snnquantprune_amd import train_utils as tu
  m = sr.DenseSNN64State(w["v"]["params"], 2.0, 1.0, 0.0, "atan", u0s)
  lg = m.forward(_np(xw), _np(wi["dropout_0"]), _np(wi["dropout_1"]), _np(wi["dense1_h"]), _np(wi["dense1_out"]),
                 _np(wi["dense2_h"]), _np(wi["dense2_out"]))
  np.testing.assert_allclose(lg.detach().numpy(), _np(logits).astype(F64), rtol=1e-6, atol=1e-7)
  tu.mse_loss(lg, labels).backward()
  worst = 0.0
  for i, (gw, ga, gc) in m.grads().items():
    leaf = params["QuantDense_%d" % i]
    pairs = [("kernel", leaf["kernel"].grad, gw)]
    if quantized:
      pairs += [("a", leaf["DuQ_0"]["a"].grad, ga), ("c", leaf["DuQ_0"]["c"].grad, gc)]
    for name, g, want in pairs:
      rel = _rel(_np(g).reshape(-1), np.asarray(want, F64).reshape(-1))
      print("QuantDense_%d/%s relative L2 %.3g" % (i, name, rel))
      worst = max(worst, rel)
      assert rel <= 1e-5, (i, name, rel)
  return worst


def _check_conv(w, params, xw, wi, u0s, logits, labels, quantized, neuron):
  """The rule of tests/test_conv_train_gpu.py: relative L2 1e-5 for every
  parameter; DuQ's c of a conv layer, whose gradient BatchNorm cancels to rounding, inside the
  element-wise gamma bound of the weight gradient's chain where it misses the relative figure."""
  from snnquantprune_amd import train_utils as tu
  saved = {"hd": _np(wi["dense_h"]), "sd": _np(wi["dense_out"])}
  for i in range(cr.NBLOCKS):
    saved["h%d" % i], saved["s%d" % i] = _np(wi["conv%d_h" % i]), _np(wi["conv%d_out" % i])
  if neuron == "plif":
    m = sr.ConvDenseSNN64NeuronState(sr.PLIF, w["v"]["params"], u0s)
  else:
    m = sr.ConvDenseSNN64State(w["v"]["params"], u0s)
  lg = m.forward(_np(xw), _np(wi["dropout_0"]), saved)
  np.testing.assert_allclose(lg.detach().numpy(), _np(logits).astype(F64), rtol=1e-6, atol=1e-7)
  assert m.h_gap < 1e-4, m.h_gap
  tu.mse_loss(lg, labels).backward()
  got = _grad_tree(params)
  worst = 0.0
  for (layer, name), want in m.grads().items():
    path = (layer, name) if name in ("scale", "bias", "tau") else (
        (layer, "kernel") if name == "kernel" else (layer, "DuQ_0", name))
    g = got[path]
    if name in ("a", "c") and not quantized:
      assert g is None or np.abs(g).max() == 0.0
      continue
    assert g is not None and np.abs(g).max() > 0, path
    rel = _rel(g.reshape(want.shape), want)
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


@pytest.mark.parametrize("key", GRAD_MODELS, ids=_gids)
def test_every_windows_gradients_match_float64(dev, key):
  """Per window of (2, 2, 2) and (1, 5): every parameter gradient of the window's loss (and `tau`
  with PLIF) within relative L2 1e-5 of the float64 model whose blocks start from the window's
  membranes as constants."""
  from snnquantprune_amd import models
  from snnquantprune_amd import train_utils as tu
  which, quantized, neuron = key
  w = _whole_run(dev, key)
  model, variables, x = w["model"], w["variables"], w["x"]
  labels = torch.arange(x.shape[0], device=dev) % model.num_classes
  worst = 0.0
  for split in ((2, 2, 2), (1, 5)):
    state, stats = models.StreamState(), _stats_of(variables)
    for k, (t0, t1) in enumerate(sr.windows(T, split)):
      params = _leaves(variables["params"])
      shapes = [tuple(u.shape) for u in state.membranes]
      u0s = [_np(u).copy() for u in state.membranes]
      xw = x[:, t0:t1]
      logits, _, wi, stats = _apply(model, params, stats, xw, 11, state)
      if k == 0:
        u0s = [np.zeros(tuple(u.shape), F32) for u in state.membranes]
      else:
        assert any(u.any() for u in u0s) and shapes == [tuple(u.shape) for u in state.membranes]
      tu.mse_loss(logits, labels).backward()
      torch.cuda.synchronize()
      if which == "dense":
        worst = max(worst, _check_dense(w, params, xw, wi, u0s, logits, _np(labels), quantized))
      else:
        worst = max(worst, _check_conv(w, params, xw, wi, u0s, logits, _np(labels), quantized, neuron))
  print("worst relative L2 %.3g" % worst)


# ---- 3. two windows chained through autograd, at block level --------------------------------------------

@pytest.mark.parametrize("tau,vr", [(2.0, 0.0), (3.0, 0.1)])
def test_two_windows_chained_through_autograd(dev, tau, vr):
  """A hidden DenseBlock over T = 6 as windows (3, 3) with u_T of the first the differentiable u0
  of the second, from a non-zero u0 leaf: spikes and h are the whole run's, and the gradients of
  the weights and of u0 are within relative L2 1e-5 of float64 autograd over the whole run (the
  saved spikes replayed); the truncated chain (u0 detached) is not."""
  from snnquantprune_amd import dense_train as dt
  from snnquantprune_amd import ops, packing
  B, K, N, vth = 5, 40, 33, 1.0
  rng = np.random.default_rng(int(tau * 10))
  x = (rng.random((T, B, K)) < 0.3).astype(F32)
  wnp = (rng.standard_normal((K, N)) * 0.35).astype(F32)
  u0np = (rng.random((B, N)) * 0.8).astype(F32)
  G = rng.standard_normal((T, B, N)).astype(F32)
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, tau, vth, vr)
  xt, Gt = torch.from_numpy(x).to(dev), torch.from_numpy(G).to(dev)

  def run(cuts, detach):
    wq = torch.from_numpy(wnp).to(dev).requires_grad_(True)
    u = u0 = torch.from_numpy(u0np).to(dev).requires_grad_(True)
    pk = packing.PackedKernel(wq.detach(), None, None)
    ss, hs = [], []
    for t0, t1 in sr.windows(T, cuts):
      s, _, h, u = dt.DenseBlock.apply(xt[t0:t1], wq, None, pk, nrn, L.SURR_ATAN, None, True, False, None,
                                       u.detach() if detach and t0 else u)
      ss.append(s)
      hs.append(h)
    s = torch.cat(ss)
    (s * Gt).sum().backward()
    return s.detach(), torch.cat(hs), _np(wq.grad), _np(u0.grad)

  s1, h1, gw1, gu1 = run((6,), False)
  s2, h2, gw2, gu2 = run((3, 3), False)
  _, _, gw3, _ = run((3, 3), True)
  assert torch.equal(s1, s2) and torch.equal(h1, h2)
  assert 0.02 <= float(s1.mean()) <= 0.5
  # float64 autograd over the whole run
  w64 = torch.from_numpy(wnp.astype(F64)).requires_grad_(True)
  u64 = torch.from_numpy(u0np.astype(F64)).requires_grad_(True)
  h32 = _np(h1)
  dsig = torch.from_numpy(tr.sg64("atan", (h32 - F32(vth)).astype(F64)))
  ssv = torch.from_numpy(_np(s1).astype(F64))
  u, out = u64, []
  for t in range(T):
    h = u + (torch.from_numpy(x[t].astype(F64)) @ w64 - (u - float(F32(vr)))) / tau
    s = tr._SavedSpike.apply(h - vth, ssv[t], dsig[t])
    u = torch.where(s.bool(), torch.full_like(h, float(F32(vr))), h)
    out.append(s)
  (torch.stack(out) * torch.from_numpy(G.astype(F64))).sum().backward()
  for what, got, want in (("whole gw", gw1, w64.grad.numpy()), ("chained gw", gw2, w64.grad.numpy()),
                          ("whole gu0", gu1, u64.grad.numpy()), ("chained gu0", gu2, u64.grad.numpy())):
    rel = _rel(got, want)
    print("%s relative L2 %.3g" % (what, rel))
    assert rel <= 1e-5, (what, rel)
  assert _rel(gw3, w64.grad.numpy()) > 1e-3           # truncation is not the whole-run gradient


# ---- 4. dropout -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["dense", "conv"])
def test_dropout_masks_are_drawn_per_window(dev, which):
  from snnquantprune_amd import models
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _setup(dev, which, True, "msl", dropout=0.9)
  name = "dropout_1" if which == "dense" else "dropout_0"

  def masks(split, seed):
    state, stats, out = models.StreamState(), _stats_of(variables), []
    for k, (t0, t1) in enumerate(sr.windows(T, split)):
      _, _, wi, stats = _apply(model, variables["params"], stats, x[:, t0:t1], tu.window_rng(seed, k), state)
      m = wi[name]
      assert m.shape[0] == t1 - t0 and set(np.unique(_np(m))) <= {0.0, 1.0}
      out.append(m)
    return torch.cat(out)

  a, b = masks((2, 2, 2), 5), masks((2, 2, 2), 5)
  assert torch.equal(a, b) and 0.8 < float(a.mean()) < 0.97
  assert not torch.equal(a[:2], a[2:4])                       # window 1 has its own seed
  assert not torch.equal(a, masks((3, 3), 5))                 # another split, other masks
  assert not torch.equal(a, masks((2, 2, 2), 6))


# ---- 5. train_step and train_step_windows --------------------------------------------------------------------

def _state_of(dev, which, **kw):
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _setup(dev, which, True, "msl", dropout=0.9, **kw)
  model.config.optimizer = "adam"
  return tu.create_train_state(variables, model.config, model), model, x


@pytest.mark.parametrize("which", ["dense", "conv"])
def test_train_step_windows_reproducible_and_one_window_is_train_step(dev, which):
  from snnquantprune_amd import train_utils as tu
  args = (lambda step: 1e-3, 1e-4, 0.0, tu.mse_loss)
  flat = lambda st: [p.clone() for _, p in tu._flatten(st.params["params"])] + [
      t.clone() for _, t in tu._flatten(st.batch_stats)]     # noqa: E731
  runs = []
  for _ in range(2):
    st, model, x = _state_of(dev, which)
    batch = {"dvs_matrix": x, "label": torch.arange(x.shape[0], device=dev) % model.num_classes}
    st, ms, u = tu.train_step_windows(st, batch, 21, *args, window=2)
    assert st.step == 3 and len(ms) == 3 and u.steps == T
    runs.append((flat(st), [m["loss"].clone() for m in ms], u.logits().clone()))
  assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
  assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1])) and torch.equal(runs[0][2], runs[1][2])
  for window in (T, T + 3):
    st, model, x = _state_of(dev, which)
    batch = {"dvs_matrix": x, "label": torch.arange(x.shape[0], device=dev) % model.num_classes}
    st, ms, u = tu.train_step_windows(st, batch, 21, *args, window=window)
    ref, _, _ = _state_of(dev, which)
    ref, m = tu.train_step(ref, batch, 21, *args)
    assert st.step == ref.step == 1 and len(ms) == 1
    assert all(torch.equal(a, b) for a, b in zip(flat(st), flat(ref)))
    assert torch.equal(ms[0]["logits"], m["logits"]) and torch.equal(u.logits(), m["logits"])


def test_twenty_recordings_in_windows_of_two_lower_the_loss(dev):
  """The fixture and criterion of tests/test_conv_train_gpu.py's test_twenty_steps_lower_the_loss
  (one fixed batch of 16 class-dependent samples, T = 3; the mean loss of the last five recordings
  below that of the first five), each recording trained as windows of 2 + 1 steps; a recording's
  loss is that of its vote over the whole recording."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  from snnquantprune_amd import train_utils as tu
  v, _ = cr.fixture(True, "uint8")
  cfg = syn.make_config(bits=cr.BITS, prune_percentage=0.9, channels=cr.CHANNELS, tau=cr.TAU, quantized=True,
                        num_conv_blocks=cr.NBLOCKS, dropout=cr.KEEP)
  cfg.optimizer = "adam"
  model = models.ConvDenseSNN(num_classes=cr.CLASSES, config=cfg)
  variables = nn.tree_from_numpy(v, dev)
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
    state, ms, u = tu.train_step_windows(state, {"dvs_matrix": x, "label": labels}, step, lambda s: 1e-2, 0.0,
                                         0.0, tu.mse_loss, window=2)
    assert len(ms) == 2 and u.steps == cr.T_STEPS
    losses.append(float(tu.mse_loss(u.logits(), labels)))
  print("losses", losses)
  assert state.step == 40 and np.isfinite(losses).all()
  assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses


# ---- 6. refusals -----------------------------------------------------------------------------------------

def test_refusals_on_the_gpu(dev, monkeypatch):
  from snnquantprune_amd import conv_train, dense_train, models, synthetic as syn

  def no_launch(*a, **k):
    raise AssertionError("a launch before the refusal")

  for which in ("dense", "conv"):
    model, v, variables, x = _setup(dev, which, True, "msl")
    state = models.StreamState()
    _apply(model, variables["params"], _stats_of(variables), x[:, :2], 3, state)
    before = state.clone()
    monkeypatch.setattr(conv_train, "conv_currents", no_launch)
    monkeypatch.setattr(dense_train, "conv_currents", no_launch)
    xb = torch.cat([x, x[:1]])[:, :2]
    with pytest.raises(ValueError, match="batch rows"):
      _apply(model, variables["params"], _stats_of(variables), xb, 3, state)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(before._tensors(), state._tensors())) and state.steps == 2
  cext = models.CextNet(num_classes=2, config=syn.make_config(dropout=0.9))
  xc = torch.zeros((2, 3, 32, 32, 2), dtype=torch.uint8, device=dev)
  st = models.StreamState()
  with pytest.raises(NotImplementedError, match="TCJA"):
    cext.apply({"params": {}, "batch_stats": {}}, xc, train=True, rng=0, u_state=st)
  assert st.counts is None and st.membranes == []
