"""The references of tests/conv_train_reference.py against independent yardsticks, on the CPU:
torch.nn.functional.conv2d under float64 autograd for the two gathered products, hand-planted ties
for the pool rule, and Higham's gamma for the float32 chain."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import conv_train_reference as cr
from tests import train_reference as tr

F32, F64 = np.float32, np.float64


def _conv2d_grads(x, w, g, strides, pads):
  """float64 autograd of the NHWC / HWIO convolution: (y, gx, gw)."""
  xt = torch.from_numpy(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
  wt = torch.from_numpy(w).permute(3, 2, 0, 1).clone().requires_grad_(True)
  (pt, pb), (pl, pr) = pads
  y = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, (pl, pr, pt, pb)), wt, stride=strides)
  y.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
  return (y.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy(),
          wt.grad.permute(2, 3, 1, 0).numpy())


@pytest.mark.parametrize("geom", cases.REF_CONV_GEOMS, ids=[g[0] for g in cases.REF_CONV_GEOMS])
def test_gathered_products_are_conv2d_autograd(geom):
  name, H, W, ks, st, pad, OH, OW = geom
  pads, (oh, ow) = cr.geometry(H, W, ks, st, pad)
  assert (oh, ow) == (OH, OW)
  rng = np.random.default_rng(len(name) * 31 + H)
  NB, Cin, Cout = 2, 3, 5
  x = rng.standard_normal((NB, H, W, Cin))
  w = rng.standard_normal(ks + (Cin, Cout))
  g = rng.standard_normal((NB, OH, OW, Cout))
  y, gx, gw = _conv2d_grads(x, w, g, st, pads)
  assert y.shape == g.shape
  a, b = cr.wgrad_matrices(x, g, ks, st, pads)
  got_w = tr.gemm_f64(a, b).reshape(w.shape)
  np.testing.assert_allclose(got_w, gw, rtol=0, atol=1e-12 * max(1.0, np.abs(gw).max()))
  a, b = cr.igrad_matrices(g, w, H, W, st, pads)
  got_x = tr.gemm_f64(a, b).reshape(x.shape)
  np.testing.assert_allclose(got_x, gx, rtol=0, atol=1e-12 * max(1.0, np.abs(gx).max()))


def test_pool_rule_on_planted_ties():
  s = np.zeros((1, 5, 7, 2), F32)                 # odd H and W: row 4 and column 6 trail
  gp = np.arange(1, 1 + 2 * 3 * 2, dtype=F32).reshape(1, 2, 3, 2)
  want = np.zeros_like(s)
  # window (0, 0), channel 0: all equal -> (0, 0)
  want[0, 0, 0, 0] = gp[0, 0, 0, 0]
  # window (0, 1), channel 0: maximum at (0, 1) and (1, 0) -> (0, 1), the first in row-major order
  s[0, 0, 3, 0] = s[0, 1, 2, 0] = 1
  want[0, 0, 3, 0] = gp[0, 0, 1, 0]
  # window (0, 2), channel 0: maximum at (1, 0) and (1, 1) -> (1, 0)
  s[0, 1, 4, 0] = s[0, 1, 5, 0] = 1
  want[0, 1, 4, 0] = gp[0, 0, 2, 0]
  # window (1, 0), channel 0: a single maximum at (1, 1)
  s[0, 3, 1, 0] = 1
  want[0, 3, 1, 0] = gp[0, 1, 0, 0]
  # window (1, 1), channel 0: all ones -> (0, 0); window (1, 2): (0, 0) and (1, 1) -> (0, 0)
  s[0, 2:4, 2:4, 0] = 1
  want[0, 2, 2, 0] = gp[0, 1, 1, 0]
  s[0, 2, 4, 0] = s[0, 3, 5, 0] = 1
  want[0, 2, 4, 0] = gp[0, 1, 2, 0]
  # channel 1: the trailing row and column hold the largest values and still get nothing
  s[0, 4, :, 1] = 5
  s[0, :, 6, 1] = 5
  s[0, 1, 1, 1] = 1
  want[0, 1, 1, 1] = gp[0, 0, 0, 1]
  for ph, pw in ((0, 1), (0, 2), (1, 0), (1, 1), (1, 2)):
    want[0, 2 * ph, 2 * pw, 1] = gp[0, ph, pw, 1]
  got = cr.pool_vjp_first_max(s, gp)
  np.testing.assert_array_equal(got, want)
  # every gp element lands exactly once, and the pool's value sits where it landed
  assert got.sum() == gp.sum()
  from oracle import snn_oracle as oracle
  pooled = oracle.max_pool_2x2(s[None])[0]
  hit = got != 0
  up = np.repeat(np.repeat(pooled, 2, 1), 2, 2)
  assert (s[:, :4, :6][hit[:, :4, :6]] == up[hit[:, :4, :6]]).all()


def test_pool_rule_is_the_vjp_where_unique():
  rng = np.random.default_rng(5)
  s = rng.permutation(4 * 6 * 3 * 2).reshape(2, 4, 6, 3).astype(F64)   # no ties
  gp = rng.standard_normal((2, 2, 3, 3))
  st = torch.from_numpy(s).permute(0, 3, 1, 2).clone().requires_grad_(True)
  torch.nn.functional.max_pool2d(st, 2).backward(torch.from_numpy(gp).permute(0, 3, 1, 2))
  np.testing.assert_array_equal(cr.pool_vjp_first_max(s, gp), st.grad.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("splits", [1, 2, 3, 7])
def test_float32_chain_inside_gamma(splits):
  rng = np.random.default_rng(splits)
  pads, (OH, OW) = cr.geometry(9, 7, (3, 3), (1, 1), "SAME")
  x = (rng.standard_normal((3, 9, 7, 4)) * 2.0 ** rng.integers(-6, 7, (3, 9, 7, 4))).astype(F32)
  g = rng.standard_normal((3, OH, OW, 5)).astype(F32)
  a, b = cr.wgrad_matrices(x, g, (3, 3), (1, 1), pads)
  Rn = a.shape[0]
  got = cr.split_sum_ref(a, b, splits)
  # each range's chain has at most L roundings and the sum of the ranges splits - 1 more
  lo, hi = cr.split_ranges(Rn, splits)[0]
  bound = tr.gamma(hi - lo + splits - 1) * tr.gemm_mag(a, b)
  assert (np.abs(got.astype(F64) - tr.gemm_f64(a, b)) <= bound).all()
  assert tr.gamma(hi - lo + splits - 1) <= tr.gamma(Rn)
  if splits == 1:
    np.testing.assert_array_equal(got, tr.gemm_chain(a, b))


def test_split_ranges_cover_r_once():
  for Rn in (0, 1, 15, 16, 17, 33, 100, 1000):
    for splits in (1, 2, 3, 7, 64):
      rs = cr.split_ranges(Rn, splits)
      assert len(rs) == splits and rs[0][0] == 0 and rs[-1][1] == Rn
      assert all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
      assert all(lo % 16 == 0 or lo == Rn for lo, _ in rs)
  assert cr.split_ranges(33, 7) == [(0, 16), (16, 32), (32, 33)] + [(33, 33)] * 4


def test_batch_stats_form():
  rng = np.random.default_rng(3)
  x = rng.standard_normal((4, 5, 6, 3)) * 3 + 1
  mean, var = cr.bn_batch_stats64(x)
  np.testing.assert_allclose(mean, x.reshape(-1, 3).mean(0), rtol=1e-14)
  np.testing.assert_allclose(var, x.reshape(-1, 3).var(0), rtol=1e-12)
  y = cr.bn_train64(x, np.ones(3), np.zeros(3), eps=0.0)
  np.testing.assert_allclose(y.reshape(-1, 3).std(0), 1.0, rtol=1e-12)


@pytest.mark.parametrize("quantized", [True, False], ids=["q4p90", "float"])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_model_fixture_fires_and_has_gradients(quantized, dtype):
  """The fixture of tests/test_conv_train_gpu.py, through the oracle: every block fires inside the
  project's 2-30 % band and every parameter gets some gradient.  A silent raster would make the
  GPU checks vacuous."""
  v, x = cr.fixture(quantized, dtype)
  p = v["params"]
  rng = np.random.default_rng(1)
  K = (cr.HW >> cr.NBLOCKS) ** 2 * cr.CHANNELS
  mask = (rng.random((cr.T_STEPS, cr.BATCH, K)) < cr.KEEP).astype(F32)
  fwd = cr.oracle_forward(p, x, mask, quantized)
  for k in ("s0", "s1", "sd"):
    r = float(fwd[k].mean())
    print(k, "rate", r)
    assert 0.02 <= r <= 0.30, (k, r)
  m = cr.TorchConvDenseSNN64(p)
  logits = m.forward(x, mask, fwd)
  np.testing.assert_allclose(logits.detach().numpy(), fwd["logits"], rtol=1e-12)
  assert m.h_gap < 1e-4
  for i in range(cr.NBLOCKS):
    np.testing.assert_allclose(fwd["mean%d" % i], m.stats[i][0], rtol=0, atol=1e-5)
    np.testing.assert_allclose(fwd["var%d" % i], m.stats[i][1], rtol=1e-5, atol=1e-7)
  labels = torch.arange(cr.BATCH) % cr.CLASSES
  torch.mean(torch.square(logits - torch.nn.functional.one_hot(labels, cr.CLASSES).double())).backward()
  for (layer, name), g in m.grads().items():
    if name in ("a", "c") and not quantized:
      continue                                   # a == -1: the quantiser passes the kernel through
    print(layer, name, float(np.abs(g).max()))
    assert np.abs(g).max() > 0, (layer, name)
