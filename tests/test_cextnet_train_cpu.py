"""CextNet training without a GPU: the references of tests/cextnet_train_reference.py are what they
claim to be (the hand-derived backward of a gated stage against float64 autograd, with and without
ties), the two entry points of csrc/train_gate.hip and the model refuse on the host what they do not
serve, and the model fixture fires, gates and has gradients everywhere."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import cextnet_train_reference as xr

F32, F64 = np.float32, np.float64


# ---- the references --------------------------------------------------------------------------------

def test_fma_rounds_once():
  """Cases where rounding a b + c to float64 first and then to float32 lands on the wrong side."""
  from fractions import Fraction
  # a b = 1 - 2^-46 and c = 2^24 + 2: the exact sum lies 2^-46 below the midpoint 2^24 + 3 of two
  # float32 values; float64 cannot hold the 2^-46, rounds to the midpoint, and the tie goes the wrong way
  a = np.array([1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23)], F32)
  b = np.array([1.0 - 2.0 ** -23, 1.0 - 2.0 ** -23], F32)
  c = np.array([2.0 ** 24 + 2, -(2.0 ** 24 + 2)], F32)
  naive = (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)
  got = xr.fma(a, b, c)
  assert got.tolist() == [2.0 ** 24 + 2, -(2.0 ** 24 + 2)] and naive.tolist() == [2.0 ** 24 + 4, -(2.0 ** 24 + 4)]
  rng = np.random.default_rng(0)
  a, b, c = (rng.standard_normal(20000).astype(F32) for _ in range(3))
  got = xr.fma(a, b, c)
  for i in range(0, 20000, 97):
    exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
    err = abs(Fraction(float(got[i])) - exact)
    for nb in (np.nextafter(got[i], F32(-np.inf)), np.nextafter(got[i], F32(np.inf))):
      assert err <= abs(Fraction(float(F32(nb))) - exact)


def _stage_inputs(seed, T=3, B=2, H=5, W=6, C=4, spikes=False):
  rng = np.random.default_rng(seed)
  if spikes:
    x = (rng.random((T, B, H, W, C)) < 0.4).astype(F64)
  else:
    x = rng.standard_normal((T, B, H, W, C)) + 0.3
  wt = rng.standard_normal((4, T, T)) * 0.8
  wc = rng.standard_normal((4, C, C)) * 0.8
  gp = rng.standard_normal((T, B, H // 2, W // 2, C))
  return x, wt, wc, gp


def _autograd(x, wt, wc, gp, first_max):
  tx, twt, twc = (torch.from_numpy(v.copy()).requires_grad_(True) for v in (x, wt, wc))
  p = xr.stage64(tx, twt, twc, first_max=first_max)
  p.backward(torch.from_numpy(gp))
  return p.detach().numpy(), tx.grad.numpy(), twt.grad.numpy(), twc.grad.numpy()


def _close(got, want, what):
  assert got.shape == want.shape, what
  if want.size == 0:
    return
  err = np.abs(got - want).max()
  assert err <= 1e-12 * max(1.0, np.abs(want).max()), (what, err)


@pytest.mark.parametrize("shape", [(3, 2, 5, 6, 4), (2, 1, 2, 2, 1), (4, 2, 8, 8, 3), (2, 2, 3, 1, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_stage_backward_is_autograd_without_ties(shape):
  """Real-valued x without ties: the hand-derived ggate -> gx and the 1-D kernel gradients against
  float64 autograd of p = maxpool(x * sigmoid(conv_c(mean x) * conv_t(mean x))), to 1e-12."""
  T, B, H, W, C = shape
  x, wt, wc, gp = _stage_inputs(5, T, B, H, W, C)
  p, gx, gwt, gwc = _autograd(x, wt, wc, gp, first_max=False)
  f = xr.stage_forward_ref(x, wt, wc)
  _close(f["p"], p, "p")
  assert 0 < f["gate"].min() and f["gate"].max() < 1
  r = xr.stage_backward_ref(x, wt, wc, gp)
  _close(r["gx"], gx, "gx")
  _close(r["gwt"], gwt, "gwt")
  _close(r["gwc"], gwc, "gwc")
  # ggate alone: the derivative of sum(gp * maxpool(x * g)) in g at the forward's gate
  if min(H, W) < 2:
    assert not r["ggate"].any()                                  # no window
    return
  tg = torch.from_numpy(f["gate"].copy()).requires_grad_(True)
  y = torch.from_numpy(x) * tg[:, :, None, None, :]
  pool = torch.nn.functional.max_pool2d(y.reshape(T * B, H, W, C).permute(0, 3, 1, 2), 2)
  (pool.permute(0, 2, 3, 1).reshape(gp.shape) * torch.from_numpy(gp)).sum().backward()
  _close(r["ggate"], tg.grad.numpy(), "ggate")


def test_stage_backward_with_planted_ties():
  """0/1 rasters (every window ties), all-equal and all-zero windows: autograd's pool is replaced by
  the stated first-maximum rule on y, the rest of the chain stays autograd's."""
  x, wt, wc, gp = _stage_inputs(9, 3, 2, 6, 6, 4, spikes=True)
  x[0, 0, 0:2, 0:2, :] = 1.0                  # an all-equal window
  x[1, 1, 2:4, 2:4, :] = 0.0                  # an all-zero window
  x[2, 0, 4:6, 0:2, 1] = 0.7                  # all equal and real-valued
  p, gx, gwt, gwc = _autograd(x, wt, wc, gp, first_max=True)
  r = xr.stage_backward_ref(x, wt, wc, gp)
  _close(r["gx"], gx, "gx")
  _close(r["gwt"], gwt, "gwt")
  _close(r["gwc"], gwc, "gwc")
  # the all-equal windows sent their gradient to position (0, 0) only
  g = xr.stage_forward_ref(x, wt, wc)["gate"]
  route = r["gx"] - (r["gm"] / (6 * 6))[:, :, None, None, :]
  np.testing.assert_allclose(route[0, 0, 0, 0], gp[0, 0, 0, 0] * g[0, 0], rtol=1e-12)
  assert np.abs(route[0, 0, 0:2, 0:2].reshape(4, -1)[1:]).max() < 1e-15


def test_gate_zero_against_autograd_with_the_rule_substituted():
  """gate == 0 for one channel, the gate a leaf: ggate and the routed part of gx against float64
  autograd of sum(gp * pool(x * gate)) with the pool's gradient routed by the first maximum of y."""
  rng = np.random.default_rng(12)
  T, B, H, W, C = 2, 2, 6, 5, 3
  x = rng.standard_normal((T, B, H, W, C))
  gate = 1.0 / (1.0 + np.exp(-rng.standard_normal((T, B, C))))
  gate[:, :, 1] = 0.0
  gp = rng.standard_normal((T, B, H // 2, W // 2, C))
  tx = torch.from_numpy(x.copy()).requires_grad_(True)
  tg = torch.from_numpy(gate.copy()).requires_grad_(True)
  xr.FirstMaxPool.apply(tx * tg[:, :, None, None, :]).backward(torch.from_numpy(gp))
  x4, g2, gp4 = x.reshape(T * B, H, W, C), gate.reshape(T * B, C), gp.reshape(T * B, H // 2, W // 2, C)
  _close(xr.gate_grad_gate_ref(x4, g2, gp4).reshape(T, B, C), tg.grad.numpy(), "ggate")
  _close(xr.gate_grad_input_ref(x4, g2, gp4, np.zeros((T * B, C))).reshape(x.shape), tx.grad.numpy(), "gx")
  # the channel with gate == 0 collected x at position (0, 0) of every window, whatever x held elsewhere
  want = (gp[..., 1] * x[:, :, 0:2 * (H // 2):2, 0:2 * (W // 2):2, 1]).sum((2, 3))
  np.testing.assert_allclose(tg.grad.numpy()[..., 1], want, rtol=1e-12)
  assert not tx.grad.numpy()[..., 1].any()


def test_gate_zero_routes_to_the_first_position():
  """gate == 0 for one channel: every y_i is +0, the first position wins although x differs -- a
  rule on x would pick the window's largest x and change ggate."""
  rng = np.random.default_rng(2)
  x = rng.standard_normal((2, 4, 4, 3)).astype(F32)
  gate = np.array([[0.5, 0.0, 0.25], [0.0, 1.0, 0.5]], F32)
  gp = rng.standard_normal((2, 2, 2, 3)).astype(F32)
  best = xr.first_max_gated(x, gate)
  assert (best[0, :, :, 1] == 0).all() and (best[1, :, :, 0] == 0).all()
  by_x = xr.first_max_gated(x, np.ones_like(gate))
  assert (by_x[0, :, :, 1] != 0).any()
  gg = xr.gate_grad_gate_ref(x, gate, gp)
  want = F32(0)
  for ph in range(2):
    for pw in range(2):
      want = xr.fma(gp[0, ph, pw, 1], x[0, 2 * ph, 2 * pw, 1], want)
  assert gg[0, 1] == want
  gx = xr.gate_grad_input_ref(x, gate, gp, np.zeros((2, 3), F32))
  assert (gx[0, :, :, 1] == 0).all()          # route = gp * 0


def test_odd_edges_get_the_mean_term_only():
  rng = np.random.default_rng(3)
  x = rng.standard_normal((1, 3, 5, 2)).astype(F32)
  gate = np.full((1, 2), 0.5, F32)
  gp = rng.standard_normal((1, 1, 2, 2)).astype(F32)
  gm = rng.standard_normal((1, 2)).astype(F32)
  gx = xr.gate_grad_input_ref(x, gate, gp, gm)
  term = (gm / F32(15)).astype(F32)
  np.testing.assert_array_equal(gx[0, 2], np.broadcast_to(term[0], (5, 2)))
  np.testing.assert_array_equal(gx[0, :, 4], np.broadcast_to(term[0], (3, 2)))
  assert xr.gate_grad_gate_ref(x[:, :1], gate, gp[:, :0]).tolist() == [[0.0, 0.0]]


# ---- host refusals -----------------------------------------------------------------------------------

def test_entry_points_refuse_on_the_host():
  lib = L.lib()
  one = ctypes.c_void_p(8)
  gg, gi = lib.snnqp_gate_pool_grad_gate, lib.snnqp_gate_pool_grad_input
  assert gg(None, None, None, 1, 4, 4, 3, None, None) == L.EINVAL           # null tensors
  assert gg(one, one, one, 1, 4, 4, 3, None, None) == L.EINVAL              # null output
  assert gg(one, one, None, 1, 4, 4, 3, one, None) == L.EINVAL              # gp is read at 4 x 4
  assert gg(one, one, one, 1, 4, 4, 0, one, None) == L.EINVAL               # C
  assert gg(one, one, one, 1, 4, 4, -3, one, None) == L.EINVAL
  assert gg(one, one, one, 1, 0, 4, 3, one, None) == L.EINVAL
  assert gg(one, one, one, -1, 4, 4, 3, one, None) == L.EINVAL
  assert gg(one, one, one, 1 << 40, 4, 4, 256, one, None) == L.EINVAL       # grid beyond the limit
  assert gg(None, None, None, 0, 4, 4, 3, None, None) == L.OK               # nothing to do
  assert gi(None, None, None, None, 1, 4, 4, 3, None, None) == L.EINVAL
  assert gi(one, one, one, None, 1, 4, 4, 3, one, None) == L.EINVAL         # gm
  assert gi(one, one, one, one, 1, 4, 4, 3, None, None) == L.EINVAL
  assert gi(one, one, one, one, 1, 4, 4, 0, one, None) == L.EINVAL
  assert gi(one, one, one, one, 1, 4, -4, 3, one, None) == L.EINVAL
  assert gi(one, one, one, one, 1 << 40, 4, 4, 256, one, None) == L.EINVAL
  assert gi(one, one, one, one, 1, 1 << 16, 1 << 16, 1, one, None) == L.EINVAL   # H W past int32
  assert gi(None, None, None, None, 0, 4, 4, 3, None, None) == L.OK
  assert b"gate_pool_grad" in lib.snnqp_last_error()


def test_weight_grad_f64_refuses_on_the_host():
  lib = L.lib()
  one = ctypes.c_void_p(8)
  ok = ops.ConvGeom(4, 4, 2, 3, 3, 3, (1, 1), ((1, 1), (1, 1))).struct()
  f, nb = lib.snnqp_conv_weight_grad_f64, lib.snnqp_conv_weight_grad_f64_workspace_bytes
  assert f(None, None, 2, ctypes.byref(ok), None, None, None) == L.EINVAL          # null tensors
  assert f(one, one, 2, ctypes.byref(ok), None, one, None) == L.EINVAL             # no workspace
  assert f(one, one, 2, ctypes.byref(ok), one, None, None) == L.EINVAL
  assert f(one, one, -1, ctypes.byref(ok), one, one, None) == L.EINVAL
  assert f(one, one, 2, None, one, one, None) == L.EINVAL
  dil = ops.ConvGeom(4, 4, 2, 3, 3, 3, (1, 1), ((1, 1), (1, 1)), (1, 1), (2, 2)).struct()
  assert f(one, one, 2, ctypes.byref(dil), one, one, None) == L.EUNSUPPORTED
  assert nb(ctypes.byref(dil), 2) == L.EUNSUPPORTED and nb(None, 2) == L.EINVAL
  assert nb(ctypes.byref(ok), 2) == 3 * 3 * 2 * 3 * 8                               # 32 rows: one range
  assert nb(ctypes.byref(ok), 0) == 3 * 3 * 2 * 3 * 8
  assert nb(ctypes.byref(ok), 65) == 2 * 3 * 3 * 2 * 3 * 8                          # 1040 rows: two
  assert nb(ctypes.byref(ok), 1 << 10) == 16 * 3 * 3 * 2 * 3 * 8                    # 16384 rows: sixteen
  assert nb(ctypes.byref(ok), 1 << 20) == 1024 * 3 * 3 * 2 * 3 * 8                  # at most 1024
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.conv_weight_grad_f64(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, 3),
                             ops.ConvGeom(4, 4, 2, 3, 3, 3, (1, 1), ((1, 1), (1, 1))))


def test_weight_grad_f64_reference_ranges_and_value():
  assert xr.wgrad_f64_ranges(0) == [(0, 0)] and xr.wgrad_f64_ranges(1024) == [(0, 1024)]
  assert xr.wgrad_f64_ranges(1140) == [(0, 570), (570, 1140)]
  r = xr.wgrad_f64_ranges(1 << 22)
  assert len(r) == 1024 and r[-1] == (1023 * 4096, 1 << 22)
  assert xr.wgrad_f64_ranges(1024 * 1024 + 1)[-1] == (1023 * 1025, 1024 * 1024 + 1)  # a short last range
  assert len(xr.wgrad_f64_ranges(64 * 1024 + 1)) == 65
  from tests import conv_train_reference as cr
  rng = np.random.default_rng(1)
  x = rng.poisson(0.6, (3, 20, 19, 2)).astype(F32)
  gI = rng.standard_normal((3, 20, 19, 4)).astype(F32)
  gI -= gI.mean((0, 1, 2), keepdims=True)                                           # a sum that cancels
  got = xr.wgrad_f64_ref(x, gI, (3, 3), (1, 1), ((1, 1), (1, 1)))
  a, b = cr.wgrad_matrices(x, gI, (3, 3), (1, 1), ((1, 1), (1, 1)))
  exact = (a.astype(F64).T @ b.astype(F64)).reshape(got.shape)
  assert (np.abs(got - exact) <= 2.0 ** -24 * np.abs(exact) + 1e-12).all()


def test_ops_refuse_cpu_tensors():
  x, g, gp = torch.zeros(1, 4, 4, 2), torch.zeros(1, 2), torch.zeros(1, 2, 2, 2)
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.gate_pool_grad_gate(x, g, gp)
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.gate_pool_grad_input(x, g, gp, g)


# ---- the model's refusals ------------------------------------------------------------------------------

def _model(**cfg_extra):
  from snnquantprune_amd import models, synthetic as syn
  cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=16, **cfg_extra)
  return models.CextNet(num_classes=2, config=cfg)


def test_train_refusals_without_gpu():
  from snnquantprune_amd import models
  from snnquantprune_amd import spiking_learning as sl
  from snnquantprune_amd.quant import uniform_static
  x = torch.zeros((2, 3, 64, 64, 2), dtype=torch.uint8)
  v = {"params": {}, "batch_stats": {}}
  with pytest.raises(NotImplementedError, match="rng"):
    _model(dropout=0.9).apply(v, x, train=True, rng=None)
  with pytest.raises(NotImplementedError, match="online"):
    _model(dropout=0.9).apply(v, x, train=True, rng=0, online=True)
  with pytest.raises(NotImplementedError, match="carried state"):
    _model(dropout=0.9).apply(v, x, train=True, rng=0, u_state=[0])
  with pytest.raises(NotImplementedError, match="density probes"):
    _model(dropout=0.9, density_probes=True).apply(v, x, train=True, rng=0, mutable=["intermediates"])
  with pytest.raises(ValueError, match="dropout"):
    _model().apply(v, x, train=True, rng=0)
  m = _model(dropout=0.9)
  m.config.quant.weight = partial(uniform_static)
  with pytest.raises(NotImplementedError, match="DuQ"):
    m.apply(v, x, train=True, rng=0)
  # the input comes first: before the rng, the config or the parameters are looked at
  bad = [torch.zeros((2, 3, 64), dtype=torch.uint8), torch.zeros((2, 3, 64, 64, 2), dtype=torch.float64),
         np.zeros((2, 3, 64, 64, 2), np.uint8),
         ops.PackedSpikes(torch.zeros((3, 2, 64, 64, 1), dtype=torch.int32), 2)]
  for xb in bad:
    with pytest.raises(NotImplementedError, match="uint8 or float32"):
      models.CextNet(num_classes=2, config=None).apply({}, xb, train=True, rng=None)
  # ... and so do the two small-image cases: five 2x2 pools need 32 x 32
  for hw in ((8, 8), (31, 64), (64, 16)):
    with pytest.raises(NotImplementedError, match="32 x 32"):
      models.CextNet(num_classes=2, config=None).apply(
          {}, torch.zeros((2, 3) + hw + (2,), dtype=torch.uint8), train=True, rng=None)


def test_training_is_no_longer_refused():
  """A 64 x 64 float32 CPU input and a valid config get past every input and config check; what
  stops the step is the first kernel's refusal of a CPU tensor."""
  from snnquantprune_amd import linen as nn
  v, x = xr.fixture(True, "float32")
  m = _model(dropout=0.9)
  with pytest.raises(RuntimeError, match="GPU only") as e:
    m.apply(nn.tree_from_numpy(v), torch.from_numpy(x), train=True, rng=0)
  assert not isinstance(e.value, NotImplementedError)


# ---- the model fixture -----------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[True, False], ids=["q4p90", "float"])
def trained(request):
  """The oracle's training forward of the fixture and the float64 yardstick's backward on it."""
  from snnquantprune_amd import train_utils as tu
  quantized = request.param
  v, x = xr.fixture(quantized)
  rng = np.random.default_rng(4)
  T, B, C = xr.T_STEPS, xr.BATCH, xr.CHANNELS
  masks = ((rng.random((T, B, 4 * C)) < xr.KEEP).astype(F32), (rng.random((T, B, 4 * C)) < xr.KEEP).astype(F32))
  fwd = xr.oracle_forward(v["params"], x, masks, quantized)
  saved = {k: fwd[k] for k in fwd if k[0] in "hs" and k[1:].isdigit()}
  saved.update({k: fwd[k] for k in ("hd1", "sd1", "hd2", "sd2")})
  m = xr.TorchCextNet64(v["params"])
  lg = m.forward(x, masks, saved)
  tu.mse_loss(lg, np.arange(B) % xr.CLASSES).backward()
  return dict(quantized=quantized, fwd=fwd, model=m, logits=lg.detach().numpy())


def test_fixture_fires_and_gates(trained):
  fwd = trained["fwd"]
  for i in range(xr.NCONV):
    rate = float(fwd["s%d" % i].mean())
    print("conv block", i, "rate", rate)
    assert 0.02 <= rate <= 0.30, (i, rate)
  rate = float(fwd["sd1"].mean())
  print("dense1 rate", rate)
  assert 0.02 <= rate <= 0.30, rate
  for j in range(2):
    g = fwd["gate%d" % j]
    print("gate", j, "min %.4f max %.4f std over channels %.4f" % (g.min(), g.max(), g.std(-1).mean()))
    assert 0.0 < g.min() and g.max() < 1.0
    assert g.std(-1).min() > 1e-3, "the gate does not vary across channels"
  # the float64 forward sees the same gates and logits
  m = trained["model"]
  for j in range(2):
    np.testing.assert_allclose(m.gates[j], fwd["gate%d" % j], rtol=1e-4)
  np.testing.assert_allclose(trained["logits"], fwd["logits"], rtol=1e-6, atol=1e-7)
  assert m.h_gap < 1e-4


def test_fixture_has_gradients_everywhere(trained):
  ref = trained["model"].grads()
  names = {layer for layer, _ in ref}
  assert {"QuantConv_%d" % i for i in range(9)} | {"BatchNorm_%d" % i for i in range(5)} | {
      "QuantDense_0", "QuantDense_1"} == names
  for (layer, name), g in ref.items():
    if name in ("a", "c") and not trained["quantized"]:
      assert np.abs(g).max() == 0.0                      # a == -1: pass-through
      continue
    assert np.abs(g).max() > 0, (layer, name)
