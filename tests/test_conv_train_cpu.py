"""What the conv training path decides on the host: the split rule, the geometries it refuses, and
the refusals of ConvDenseSNN.apply(train=True).  No GPU."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops


def _geom(H=16, W=16, Cin=8, Cout=8, KH=3, KW=3, **kw):
  return ops.ConvGeom(H, W, Cin, Cout, KH, KW, **kw)


def test_split_rule_depends_on_shapes_only_and_is_capped():
  seen = set()
  for H, Cin, Cout, NB in [(1, 1, 1, 0), (1, 1, 1, 1), (4, 2, 16, 6), (16, 4, 8, 4), (64, 128, 128, 40),
                           (128, 2, 128, 40), (32, 128, 128, 40), (64, 128, 128, 100000), (8, 512, 512, 2)]:
    g = _geom(H, H, Cin, Cout, pad=((1, 1), (1, 1)))
    n = ops.conv_grad_splits(g, NB)
    assert 1 <= n <= 64
    assert n == ops.conv_grad_splits(_geom(H, H, Cin, Cout, pad=((1, 1), (1, 1))), NB)
    # the stated rule: tiles x splits near 1024 workgroups, no range under 16 chunks of 16 rows
    tiles = -(-9 * Cin // 64) * -(-Cout // 64)
    chunks = -(-NB * H * H // 16)
    assert n == max(1, min(-(-1024 // tiles), chunks // 16, 64))
    seen.add(n)
    ws = ops.conv_weight_grad_workspace_bytes(g, n)
    assert ws == (0 if n == 1 else n * 9 * Cin * Cout * 4)
  assert 1 in seen and 64 in seen and len(seen) > 3
  # conv1 of the C3 topology at the reference's per-device batch: 18 x 2 tiles, T B = 40 images
  assert ops.conv_grad_splits(_geom(64, 64, 128, 128, pad=((1, 1), (1, 1))), 40) == 29


def test_workspace_bytes_refuses_bad_splits():
  g = _geom()
  assert ops.conv_weight_grad_workspace_bytes(g, 1) == 0
  assert ops.conv_weight_grad_workspace_bytes(g, 64) == 64 * 9 * 8 * 8 * 4
  for bad in (0, -1, 65):
    with pytest.raises(L.SnnqpError) as e:
      ops.conv_weight_grad_workspace_bytes(g, bad)
    assert e.value.code == L.EINVAL


@pytest.mark.parametrize("kw", [dict(groups=2), dict(in_dil=(2, 1)), dict(in_dil=(1, 2)), dict(k_dil=(2, 1)),
                                dict(k_dil=(1, 3)), dict(pad=((-1, 0), (0, 0)))],
                         ids=lambda k: "%s=%s" % next(iter(k.items())))
def test_unsupported_geometry_is_refused_on_the_host(kw):
  """SNNQP_EUNSUPPORTED from every entry point, with null tensors: nothing can have been launched."""
  g = _geom(**kw)
  st = g.struct()
  lib = L.lib()
  assert lib.snnqp_conv_grad_splits(ctypes.byref(st), 4) == L.EUNSUPPORTED
  assert lib.snnqp_conv_weight_grad_workspace_bytes(ctypes.byref(st), 2) == L.EUNSUPPORTED
  assert lib.snnqp_conv_weight_grad(None, None, 4, ctypes.byref(st), 1, None, None, None) == L.EUNSUPPORTED
  assert lib.snnqp_conv_input_grad(None, None, 4, ctypes.byref(st), None, None) == L.EUNSUPPORTED
  with pytest.raises(L.SnnqpError) as e:
    ops.conv_grad_splits(g, 4)
  assert e.value.code == L.EUNSUPPORTED


def test_bad_arguments_are_einval_on_the_host():
  lib = L.lib()
  st = _geom().struct()
  assert lib.snnqp_conv_weight_grad(None, None, 4, ctypes.byref(st), 1, None, None, None) == L.EINVAL
  assert lib.snnqp_conv_weight_grad(None, None, -1, ctypes.byref(st), 1, None, None, None) == L.EINVAL
  assert lib.snnqp_conv_weight_grad(None, None, 0, ctypes.byref(st), 65, None, None, None) == L.EINVAL
  assert lib.snnqp_conv_input_grad(None, None, 4, ctypes.byref(st), None, None) == L.EINVAL
  assert lib.snnqp_conv_grad_splits(None, 4) == L.EINVAL
  assert lib.snnqp_conv_grad_splits(ctypes.byref(_geom(stride=(0, 1)).struct()), 4) == L.EINVAL
  assert lib.snnqp_maxpool2x2_backward(None, None, 1, 4, 4, 0, None, None) == L.EINVAL
  assert lib.snnqp_maxpool2x2_backward(None, None, 1, 4, 4, 3, None, None) == L.EINVAL
  assert lib.snnqp_maxpool2x2_backward(None, None, 0, 4, 4, 3, None, None) == L.OK
  # the pixel tiles of the input gradient ride on grid x: 2^31 tiles of 64 pixels is too many
  big = _geom(1 << 15, 1 << 15, 1, 1, 1, 1).struct()
  assert lib.snnqp_conv_input_grad(None, None, 1 << 8, ctypes.byref(big), None, None) == L.EINVAL


def test_ops_refuse_cpu_tensors():
  g = _geom(4, 4, 2, 3, pad=((1, 1), (1, 1)))
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.conv_weight_grad(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, 3), g)
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.conv_input_grad(torch.zeros(1, 4, 4, 3), torch.zeros(3, 3, 2, 3), g)
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.maxpool2x2_backward(torch.zeros(1, 4, 4, 2), torch.zeros(1, 2, 2, 2))


def _model(**cfg_extra):
  from snnquantprune_amd import models, synthetic as syn
  cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=16, num_conv_blocks=2, **cfg_extra)
  return models.ConvDenseSNN(num_classes=2, config=cfg)


def test_train_refusals_without_gpu():
  from snnquantprune_amd import models, synthetic as syn
  from snnquantprune_amd import spiking_learning as sl
  from snnquantprune_amd.quant import uniform_static
  x = torch.zeros((2, 3, 8, 8, 2), dtype=torch.uint8)
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
  m = _model(dropout=0.9)
  m.config.neuron_dynamics = partial(sl.parametric_leaky_IF, init_tau=2.0, spike_fn=sl.atan)
  with pytest.raises(NotImplementedError, match="multi_step_LIF"):
    m.apply(v, x, train=True, rng=0)
  # the input comes first: before the rng, the config or the parameters are looked at
  bad = [torch.zeros((2, 3, 64), dtype=torch.uint8), torch.zeros((2, 3, 8, 8, 2), dtype=torch.float64),
         torch.zeros((2, 3, 8, 8, 2), dtype=torch.int32), np.zeros((2, 3, 8, 8, 2), np.uint8),
         ops.PackedSpikes(torch.zeros((3, 2, 8, 8, 1), dtype=torch.int32), 2),
         ops.pack_frames_host(torch.zeros((2, 3, 8, 8, 2), dtype=torch.uint8), L.EV1)]
  for xb in bad:
    with pytest.raises(NotImplementedError, match="uint8 or float32"):
      models.ConvDenseSNN(num_classes=2, config=None).apply({}, xb, train=True, rng=None)
  with pytest.raises(NotImplementedError):
    models.CextNet(num_classes=2, config=syn.make_config(dropout=0.9)).apply(v, x, train=True, rng=0)


def test_bn_backward_is_autograd_of_the_stated_forward():
  """conv_train.bn_backward against float64 torch autograd of the batch-statistics BatchNorm."""
  from snnquantprune_amd import conv_train as ct
  g0 = torch.Generator().manual_seed(3)
  T, N, C = 3, 50, 5
  x = (torch.randn(T, N, C, generator=g0) * 2 + 0.5).to(torch.float32)
  g = torch.randn(T, N, C, generator=g0).to(torch.float32)
  scale = (torch.rand(C, generator=g0) + 0.5).to(torch.float32)
  bias = torch.randn(C, generator=g0).to(torch.float32)
  mean, var = ct.batch_stats(x)
  x64 = x.double().requires_grad_(True)
  s64, b64 = scale.double().requires_grad_(True), bias.double().requires_grad_(True)
  m = x64.mean(1, keepdim=True)
  v = (x64 * x64).mean(1, keepdim=True) - m * m
  y = (x64 - m) * (torch.rsqrt(v + 1e-5) * s64) + b64
  y.backward(g.double())
  np.testing.assert_allclose(mean.numpy(), m.detach()[:, 0].numpy(), rtol=2.0 ** -23)
  np.testing.assert_allclose(var.numpy(), v.detach()[:, 0].numpy(), rtol=2.0 ** -23)
  gx, gs, gb = ct.bn_backward(g, x, mean, var, scale, 1e-5)
  ref = x64.grad.numpy()
  assert np.linalg.norm(gx.numpy() - ref) <= 1e-6 * np.linalg.norm(ref)
  np.testing.assert_allclose(gs.numpy(), s64.grad.numpy(), rtol=1e-5)
  np.testing.assert_allclose(gb.numpy(), b64.grad.numpy(), rtol=1e-5)
  # the forward, given the statistics, is the eval arithmetic of the oracle
  from oracle import snn_oracle as oracle
  yy = ct.bn_normalise(x.clone(), mean, ct.bn_multiplier(var, scale, 1e-5), bias).numpy()
  for t in range(T):
    want = oracle.batchnorm_eval(x[t].numpy(), mean[t].numpy(), var[t].numpy(), scale.numpy(), bias.numpy())
    np.testing.assert_array_equal(yy[t], want)


def test_running_update_is_the_t_fold_recurrence():
  from snnquantprune_amd import conv_train as ct
  new = torch.tensor([[1.0, -2.0], [0.5, 3.0], [4.0, 0.25]])
  got = ct.running_update(torch.tensor([0.0, 1.0]), new, 0.9).numpy()
  ra = np.array([0.0, 1.0], np.float32)
  m = np.float32(0.9)
  for t in range(3):
    ra = m * ra + (np.float32(1) - m) * new[t].numpy()
  np.testing.assert_array_equal(got, ra.astype(np.float32))
