"""DenseSNN training, host side: surrogate derivatives, the DuQ / prune VJPs, the vote and loss
gradients, the gradient mean over ranks, weight decay and the refusals that need no GPU."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_surrogate_derivatives_at_points():
  from snnquantprune_amd.dense_train import surrogate_derivative as sd
  x = torch.tensor([-0.5, 0.0, 0.5, 0.25, -1.0], dtype=torch.float64)
  want = {
      "fast_sigmoid": [1 / 36, 1.0, 1 / 36, 1 / 12.25, 1 / 121],
      "atan": [1 / (1 + (math.pi / 2) ** 2), 1.0, 1 / (1 + (math.pi / 2) ** 2),
               1 / (1 + (math.pi / 4) ** 2), 1 / (1 + math.pi ** 2)],
      "slayer": [math.exp(-2.5), 1.0, math.exp(-2.5), math.exp(-1.25), math.exp(-5)],
      "smooth_step": [1.0, 1.0, 0.0, 1.0, 0.0],            # [-0.5, 0.5)
      "piecewise_linear": [0.0, 1.0, 0.0, 0.5, 0.0],
  }
  for name, w in want.items():
    np.testing.assert_allclose(sd(name, x).numpy(), w, rtol=1e-12, err_msg=name)
  with pytest.raises(NotImplementedError):
    sd("heaviside", x)


def test_surrogate_of_refuses_other_neurons_and_spike_fns():
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import spiking_learning as sl
  from snnquantprune_amd.dense_train import surrogate_of
  assert surrogate_of(sl.multi_step_LIF(tau=2.0, spike_fn=sl.slayer)) == L.SURR_SLAYER
  with pytest.raises(NotImplementedError):
    surrogate_of(sl.LIF(init_tau=2.0, spike_fn=sl.atan))
  with pytest.raises(NotImplementedError):
    surrogate_of(sl.multi_step_LIF(tau=2.0, spike_fn=lambda x: x))


def _duq_case():
  w = torch.tensor([[0.5, -1.0, 2.0], [1.0, 0.3, -0.7]], dtype=torch.float64)
  a = torch.tensor([1.0], dtype=torch.float64)
  c = torch.tensor([0.8], dtype=torch.float64)
  mask = torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 1.0]], dtype=torch.float64)
  g = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], dtype=torch.float64)
  return w, a, c, mask, g


def test_duq_and_prune_vjp():
  from snnquantprune_amd.dense_train import weight_transform_grads
  w, a, c, mask, g = _duq_case()
  L = 127.0
  gw, ga, gc, gm = weight_transform_grads(g, w, a, c, mask, L)
  gp = g * mask                                           # prune: g * mask, mask gets zero
  inside = (w / a).abs() <= 1                             # |W/a| == 1 exactly: inside
  assert inside.tolist() == [[True, True, False], [True, True, True]]
  np.testing.assert_allclose(gw.numpy(), torch.where(inside, gp * 0.8, 0.0).numpy())
  r = torch.round(torch.clamp(w, -1, 1) * L) / L
  np.testing.assert_allclose(gc.numpy(), [(gp * r).sum().item()])
  np.testing.assert_allclose(ga.numpy(), [-(torch.where(inside, gp * 0.8 * w, 0.0)).sum().item()])
  assert torch.equal(gm, torch.zeros_like(mask))


def test_duq_pass_through_and_unquantised():
  from snnquantprune_amd.dense_train import weight_transform_grads
  w, _, c, mask, g = _duq_case()
  a = torch.tensor([-1.0], dtype=torch.float64)
  gw, ga, gc, gm = weight_transform_grads(g, w, a, c, None, 127.0)
  assert torch.equal(gw, g) and float(ga) == 0.0 and float(gc) == 0.0 and gm is None
  gw, ga, gc, gm = weight_transform_grads(g, w, None, None, mask, None)
  assert torch.equal(gw, g * mask) and ga is None and gc is None


def test_weight_transform_function_reaches_the_leaves():
  from snnquantprune_amd.dense_train import _WeightTransform
  w, a, c, mask, g = _duq_case()
  leaves = [t.clone().requires_grad_(True) for t in (w, a, c, mask)]
  value = torch.zeros_like(w)
  y = _WeightTransform.apply(*leaves, value, 127.0)
  (y * g).sum().backward()
  assert all(t.grad is not None for t in leaves)
  assert float(leaves[3].grad.abs().max()) == 0.0


def test_vote_and_loss_gradients():
  """d loss / d s2 through the vote (models.py:253-255) is gLogits[b, n // 10] / (10 T)."""
  from snnquantprune_amd import train_utils as tu
  T, B, C = 3, 4, 2
  s = torch.rand((T, B, C * 10), dtype=torch.float64, requires_grad=True)
  labels = torch.tensor([0, 1, 1, 0])
  for loss in (tu.mse_loss, tu.cross_entropy_loss):
    s.grad = None
    logits = s.mean(0).reshape(B, C, 10).mean(-1)
    lg = logits.detach().clone().requires_grad_(True)
    loss(lg, labels, 0.1).backward()
    loss(logits, labels, 0.1).backward()
    want = lg.grad.repeat_interleave(10, dim=1)[None].expand(T, B, C * 10) / (10 * T)
    np.testing.assert_allclose(s.grad.numpy(), want.numpy(), rtol=1e-12)
  lg = torch.tensor([[1.0, -1.0]], dtype=torch.float64, requires_grad=True)
  tu.mse_loss(lg, torch.tensor([0])).backward()
  np.testing.assert_allclose(lg.grad.numpy(), [[0.0, -1.0]])       # 2 (x - y) / (B C)
  lg.grad = None
  tu.cross_entropy_loss(lg, torch.tensor([0])).backward()
  p = torch.softmax(lg.detach(), -1)
  np.testing.assert_allclose(lg.grad.numpy(), (p - torch.tensor([[1.0, 0.0]])).numpy())


def test_weight_decay_skips_batchnorm():
  from snnquantprune_amd import train_utils as tu
  params = {"QuantDense_0": {"kernel": torch.ones(2, 2), "DuQ_0": {"a": torch.tensor([2.0]),
                                                                  "c": torch.tensor([1.0])},
                             "prune_0": {"mask": torch.ones(2, 2)}},
            "BatchNorm_0": {"scale": torch.full((3,), 10.0)}}
  assert float(tu.weight_decay_fn(params)) == 0.5 * (4 + 4 + 1 + 4)


def test_unknown_optimizer_raises():
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import train_utils as tu
  cfg = nn.ConfigDict(optimizer="rmsprop")
  with pytest.raises(ValueError):
    tu.make_optimizer(cfg, [torch.zeros(1)])
  cfg = nn.ConfigDict(optimizer="sgd", momentum=0.9, nesterov=True)
  opt = tu.make_optimizer(cfg, [torch.zeros(1)])
  assert opt.param_groups[0]["nesterov"] and opt.param_groups[0]["momentum"] == 0.9


def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


def _mean_worker(rank, world, port, out):
  os.environ["MASTER_ADDR"] = "127.0.0.1"
  os.environ["MASTER_PORT"] = str(port)
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from snnquantprune_amd.parallel import mean_over_ranks
    ts = [torch.full((2, 3), float(rank + 1)), torch.tensor([10.0 * (rank + 1)])]
    mean_over_ranks(ts)
    out[rank] = [t.tolist() for t in ts]
  finally:
    dist.destroy_process_group()


def test_gloo_world2_gradient_mean():
  port = _free_port()
  with mp.Manager() as m:
    out = m.dict()
    mp.spawn(_mean_worker, args=(2, port, out), nprocs=2, join=True)
    for r in (0, 1):
      assert out[r][0] == [[1.5] * 3] * 2 and out[r][1] == [15.0]


def test_mean_over_ranks_without_distributed_is_identity():
  from snnquantprune_amd.parallel import mean_over_ranks
  t = [torch.ones(3)]
  assert mean_over_ranks(t)[0].tolist() == [1.0, 1.0, 1.0]


def _model(**cfg_extra):
  from snnquantprune_amd import models, synthetic as syn
  cfg = syn.make_config(bits=8, prune_percentage=0.5, hidden=32, **cfg_extra)
  return models.DenseSNN(num_classes=2, config=cfg)


def test_train_refusals_without_gpu():
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  from snnquantprune_amd import spiking_learning as sl
  from functools import partial
  x = torch.zeros((2, 3, 64), dtype=torch.uint8)
  v = {"params": {}, "batch_stats": {}}
  with pytest.raises(NotImplementedError):
    _model(dropout=0.9).apply(v, x, train=True, rng=None)
  with pytest.raises(NotImplementedError):
    _model(dropout=0.9).apply(v, x, train=True, rng=0, online=True)
  with pytest.raises(NotImplementedError):
    _model(dropout=0.9).apply(v, x, train=True, rng=0, u_state=[0])
  with pytest.raises(NotImplementedError):
    _model(dropout=0.9, density_probes=True).apply(v, x, train=True, rng=0,
                                                   mutable=["intermediates"])
  with pytest.raises(ValueError, match="dropout"):
    _model().apply(v, x, train=True, rng=0)
  from snnquantprune_amd.quant import uniform_static
  m = _model(dropout=0.9)
  m.config.quant.weight = partial(uniform_static)
  with pytest.raises(NotImplementedError):
    m.apply(v, x, train=True, rng=0)
  for cls in (models.ConvDenseSNN, models.CextNet):
    with pytest.raises(NotImplementedError):
      cls(num_classes=2, config=syn.make_config(dropout=0.9)).apply(v, x, train=True, rng=0)
