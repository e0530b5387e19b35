"""The training kernels of csrc/train_conv.hip one at a time, bit for bit against the plain
references of tests/conv_train_reference.py: the gathered products at the edges of the 16 / 64
tiles and of the image, the split reduction, and the pool's gradient routing."""
import ctypes

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import cases
from tests import conv_train_reference as cr
from tests import train_reference as tr
from tests.train_helpers import _frame_untouched, _framed, _np, mixed

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _geom(H, W, Cin, Cout, ks, st, pads):
  return ops.ConvGeom(H, W, Cin, Cout, ks[0], ks[1], tuple(st), tuple(tuple(p) for p in pads))


def _run_wgrad(dev, x, g, geom, splits):
  """snnqp_conv_weight_grad on NaN-framed inputs into sentinel-framed outputs -> gw."""
  lib = L.lib()
  xw, xv = _framed(dev, x, np.nan)
  gw_, gv = _framed(dev, g, np.nan)
  st = geom.struct()
  if splits is None:
    splits = ops.conv_grad_splits(geom, x.shape[0])
  nws = ops.conv_weight_grad_workspace_bytes(geom, splits) // 4
  shape = (geom.KH, geom.KW, geom.Cin, geom.Cout)
  ow, ov = _framed(dev, np.full(shape, SENTINEL, F32), SENTINEL)
  ww, wv = _framed(dev, np.full((max(nws, 1),), SENTINEL, F32), SENTINEL)
  L.check(lib.snnqp_conv_weight_grad(ops._ptr(xv), ops._ptr(gv), x.shape[0], ctypes.byref(st),
                                     splits, ops._ptr(wv) if nws else None, ops._ptr(ov),
                                     ops._stream()))
  torch.cuda.synchronize()
  assert _frame_untouched(ow, ov.numel(), SENTINEL)
  assert _frame_untouched(ww, wv.numel(), SENTINEL)
  if not nws:
    assert bool((wv == SENTINEL).all())
  return _np(ov)


def _run_igrad(dev, g, w, geom):
  lib = L.lib()
  gw_, gv = _framed(dev, g, np.nan)
  ww, wv = _framed(dev, w, np.nan)
  st = geom.struct()
  shape = (g.shape[0], geom.H, geom.W, geom.Cin)
  ow, ov = _framed(dev, np.full(shape, SENTINEL, F32), SENTINEL)
  L.check(lib.snnqp_conv_input_grad(ops._ptr(gv), ops._ptr(wv), g.shape[0], ctypes.byref(st),
                                    ops._ptr(ov), ops._stream()))
  torch.cuda.synchronize()
  assert _frame_untouched(ow, ov.numel(), SENTINEL)
  return _np(ov)


def _check_both(dev, rng, NB, H, W, Cin, Cout, ks, st, padding, splits=(1, None), data=mixed):
  pads, (OH, OW) = cr.geometry(H, W, ks, st, padding)
  geom = _geom(H, W, Cin, Cout, ks, st, pads)
  assert geom.out_hw() == (OH, OW)
  x = data(rng, (NB, H, W, Cin))
  g = mixed(rng, (NB, OH, OW, Cout))
  w = mixed(rng, tuple(ks) + (Cin, Cout))
  a, b = cr.wgrad_matrices(x, g, ks, st, pads)
  for s in splits:
    n = ops.conv_grad_splits(geom, NB) if s is None else s
    got = _run_wgrad(dev, x, g, geom, s)
    want = cr.split_sum_ref(a, b, n).reshape(got.shape)
    print("wgrad splits=%s: differing elements %d of %d" % (n, int((got != want).sum()), want.size))
    np.testing.assert_array_equal(got, want)
  a, b = cr.igrad_matrices(g, w, H, W, st, pads)
  got = _run_igrad(dev, g, w, geom)
  want = tr.gemm_chain(a, b).reshape(got.shape)
  print("igrad: differing elements %d of %d" % (int((got != want).sum()), want.size))
  np.testing.assert_array_equal(got, want)
  return geom


# (NB, H, W, Cin, Cout, ks): I = KH KW Cin on 1, 18, 63, 64, 65, 129; Cout on 1, 15, 16, 17, 64, 65;
# Rn = NB OH OW (SAME, stride 1: NB H W) on 1, 15, 16, 17, 33.
EDGES = [
    (1, 1, 1, 1, 1, (1, 1)),          # I 1, Cout 1, Rn 1
    (1, 3, 5, 2, 15, (3, 3)),         # I 18, Cout 15, Rn 15
    (1, 4, 4, 7, 16, (3, 3)),         # I 63, Cout 16, Rn 16
    (1, 1, 17, 16, 17, (2, 2)),       # I 64, Cout 17, Rn 17
    (3, 1, 11, 13, 64, (1, 5)),       # I 65, Cout 64, Rn 33
    (1, 3, 11, 43, 65, (3, 1)),       # I 129, Cout 65, Rn 33
    (2, 6, 7, 18, 65, (1, 1)),        # 1x1 kernel, I 18, Rn 84
    (2, 5, 9, 129, 1, (1, 1)),        # I 129 in one tap, Cout 1
]


@pytest.mark.parametrize("case", EDGES, ids=lambda c: "x".join(map(str, c[:5])) + "k%dx%d" % c[5])
def test_products_bit_equal_chain_tile_edges(dev, case):
  NB, H, W, Cin, Cout, ks = case
  rng = np.random.default_rng(NB * 7919 + H * 131 + W * 17 + Cin + Cout)
  geom = _check_both(dev, rng, NB, H, W, Cin, Cout, ks, (1, 1), "SAME", splits=(1, 2, None))
  assert geom.KH * geom.KW * Cin in (1, 18, 63, 64, 65, 129)


@pytest.mark.parametrize("g", cases.REF_CONV_GEOMS, ids=[g[0] for g in cases.REF_CONV_GEOMS])
def test_products_bit_equal_chain_nine_geometries(dev, g):
  name, H, W, ks, st, pad, OH, OW = g
  rng = np.random.default_rng(len(name) * 31 + H)
  geom = _check_both(dev, rng, 2, H, W, 3, 5, ks, st, pad, splits=(1, 3, None))
  assert geom.out_hw() == (OH, OW)


def test_padding_wider_than_kernel(dev):
  rng = np.random.default_rng(8)
  # whole kernel positions lie in the padding; stride 2 leaves rows of gx with no tap at all
  _check_both(dev, rng, 2, 3, 4, 5, 6, (2, 3), (2, 2), ((4, 3), (5, 4)), splits=(1, 3))
  _check_both(dev, rng, 1, 1, 1, 3, 4, (3, 3), (1, 1), ((3, 3), (3, 3)), splits=(1, 2))


def test_spike_inputs(dev):
  rng = np.random.default_rng(9)
  spikes = lambda r, shape: (r.random(shape) < 0.2).astype(F32)     # noqa: E731
  _check_both(dev, rng, 3, 8, 8, 16, 16, (3, 3), (1, 1), ((1, 1), (1, 1)), splits=(1, 7, None),
              data=spikes)


@pytest.mark.parametrize("splits", [1, 2, 3, 7, None])
def test_weight_grad_splits(dev, splits):
  rng = np.random.default_rng(10)
  NB, H, W, Cin, Cout, ks = 5, 9, 11, 6, 20, (3, 3)
  pads, (OH, OW) = cr.geometry(H, W, ks, (1, 1), "SAME")
  geom = _geom(H, W, Cin, Cout, ks, (1, 1), pads)
  x, g = mixed(rng, (NB, H, W, Cin)), mixed(rng, (NB, OH, OW, Cout))
  a, b = cr.wgrad_matrices(x, g, ks, (1, 1), pads)
  n = ops.conv_grad_splits(geom, NB) if splits is None else splits
  got = _run_wgrad(dev, x, g, geom, splits)
  np.testing.assert_array_equal(got, cr.split_sum_ref(a, b, n).reshape(got.shape))
  again = _run_wgrad(dev, x, g, geom, splits)
  assert got.tobytes() == again.tobytes()
  # the split changes the rounding, not the sum: inside gamma of float64 either way
  slack = tr.gamma(a.shape[0]) * tr.gemm_mag(a, b)
  assert (np.abs(got.reshape(slack.shape).astype(F64) - tr.gemm_f64(a, b)) <= slack).all()


def test_weight_grad_default_split_more_than_one(dev):
  """A shape whose default split is > 1, so that the default path runs the second kernel."""
  rng = np.random.default_rng(11)
  NB, H, W, Cin, Cout, ks = 4, 16, 16, 4, 8, (3, 3)
  pads, (OH, OW) = cr.geometry(H, W, ks, (1, 1), "SAME")
  geom = _geom(H, W, Cin, Cout, ks, (1, 1), pads)
  n = ops.conv_grad_splits(geom, NB)
  assert n > 1
  x, g = mixed(rng, (NB, H, W, Cin)), mixed(rng, (NB, OH, OW, Cout))
  a, b = cr.wgrad_matrices(x, g, ks, (1, 1), pads)
  got = _np(ops.conv_weight_grad(torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev), geom))
  np.testing.assert_array_equal(got, cr.split_sum_ref(a, b, n).reshape(got.shape))


def test_weight_grad_last_range_empty(dev):
  rng = np.random.default_rng(12)
  NB, H, W, Cin, Cout, ks = 1, 3, 11, 5, 7, (3, 3)                    # Rn = 33: 3 chunks of 16
  pads, (OH, OW) = cr.geometry(H, W, ks, (1, 1), "SAME")
  geom = _geom(H, W, Cin, Cout, ks, (1, 1), pads)
  ranges = cr.split_ranges(NB * OH * OW, 7)
  assert ranges[-1][0] == ranges[-1][1] and ranges[2] == (32, 33)
  x, g = mixed(rng, (NB, H, W, Cin)), mixed(rng, (NB, OH, OW, Cout))
  a, b = cr.wgrad_matrices(x, g, ks, (1, 1), pads)
  got = _run_wgrad(dev, x, g, geom, 7)
  np.testing.assert_array_equal(got, cr.split_sum_ref(a, b, 7).reshape(got.shape))


def test_one_by_one_conv_is_dense_weight_grad(dev):
  rng = np.random.default_rng(13)
  NB, H, W, Cin, Cout = 3, 5, 7, 70, 33
  geom = _geom(H, W, Cin, Cout, (1, 1), (1, 1), ((0, 0), (0, 0)))
  x, g = mixed(rng, (NB, H, W, Cin)), mixed(rng, (NB, H, W, Cout))
  xd, gd = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
  conv = ops.conv_weight_grad(xd, gd, geom, splits=1).reshape(Cin, Cout)
  dense = ops.dense_weight_grad(xd.reshape(-1, Cin), gd.reshape(-1, Cout))
  assert torch.equal(conv, dense)
  np.testing.assert_array_equal(_np(dense), tr.gemm_chain(x.reshape(-1, Cin), g.reshape(-1, Cout)))


def test_nan_and_inf_reach_what_the_chain_says(dev):
  rng = np.random.default_rng(14)
  NB, H, W, Cin, Cout, ks, st = 2, 6, 5, 3, 4, (3, 3), (2, 1)
  pads, (OH, OW) = cr.geometry(H, W, ks, st, "SAME")
  geom = _geom(H, W, Cin, Cout, ks, st, pads)
  x, g, w = mixed(rng, (NB, H, W, Cin)), mixed(rng, (NB, OH, OW, Cout)), mixed(rng, ks + (Cin, Cout))
  x[0, 0, 0, 1] = np.nan                       # a corner: some taps never see it
  x[1, 3, 2, 0] = np.inf
  g[1, 1, 3, 2] = -np.inf
  g[0, 2, 0, 0] = np.nan
  w[1, 1, 2, 3] = np.inf
  a, b = cr.wgrad_matrices(x, g, ks, st, pads)
  for splits in (1, 2):
    got = _run_wgrad(dev, x, g, geom, splits)
    want = cr.split_sum_ref(a, b, splits).reshape(got.shape)
    np.testing.assert_array_equal(got, want)
    assert np.isnan(want).any() and np.isfinite(want).any()
  a, b = cr.igrad_matrices(g, w, H, W, st, pads)
  got = _run_igrad(dev, g, w, geom)
  want = tr.gemm_chain(a, b).reshape(got.shape)
  np.testing.assert_array_equal(got, want)
  assert np.isnan(want).any() and np.isfinite(want).any()


def test_no_images(dev):
  geom = _geom(4, 4, 3, 5, (3, 3), (1, 1), ((1, 1), (1, 1)))
  st = geom.struct()
  gw = torch.full((3, 3, 3, 5), SENTINEL, dtype=torch.float32, device=dev)
  for splits in (1, 3):
    gw.fill_(SENTINEL)
    L.check(L.lib().snnqp_conv_weight_grad(None, None, 0, ctypes.byref(st), splits, None,
                                           ops._ptr(gw), ops._stream()))
    assert bool((gw == 0).all())
  L.check(L.lib().snnqp_conv_input_grad(None, None, 0, ctypes.byref(st), None, ops._stream()))


@pytest.mark.parametrize("shape", [(3, 5, 7, 3), (2, 4, 6, 33), (1, 1, 1, 2), (2, 2, 3, 1), (5, 7, 2, 65)],
                         ids=lambda s: "x".join(map(str, s)))
def test_pool_backward(dev, shape):
  rng = np.random.default_rng(sum(shape))
  NB, H, W, C = shape
  s = (rng.random(shape) < 0.4).astype(F32)                 # spikes: ties in most windows
  s[0] = 1.0 if NB > 1 else s[0]                            # windows of all-equal values
  if NB > 1:
    s[1] = 0.0
  gp = mixed(rng, (NB, H // 2, W // 2, C))
  sw, sv = _framed(dev, s, np.nan)
  gw_, gv = _framed(dev, gp, np.nan)
  ow, ov = _framed(dev, np.full(shape, SENTINEL, F32), SENTINEL)
  L.check(L.lib().snnqp_maxpool2x2_backward(ops._ptr(sv), ops._ptr(gv) if gp.size else None, NB, H, W,
                                            C, ops._ptr(ov), ops._stream()))
  torch.cuda.synchronize()
  assert _frame_untouched(ow, ov.numel(), SENTINEL)
  want = cr.pool_vjp_first_max(s, gp)
  np.testing.assert_array_equal(_np(ov), want)
  np.testing.assert_array_equal(_np(ops.maxpool2x2_backward(sv, gv)), want)
  if H % 2:
    assert (want[:, H - 1] == 0).all()
  if W % 2:
    assert (want[:, :, W - 1] == 0).all()


def test_pool_backward_real_values(dev):
  rng = np.random.default_rng(15)
  s = rng.integers(-2, 3, (2, 6, 5, 9)).astype(F32)         # few distinct values: many ties
  gp = mixed(rng, (2, 3, 2, 9))
  got = _np(ops.maxpool2x2_backward(torch.from_numpy(s).to(dev), torch.from_numpy(gp).to(dev)))
  np.testing.assert_array_equal(got, cr.pool_vjp_first_max(s, gp))
  pooled = _np(ops.maxpool2x2(torch.from_numpy(s).to(dev)))
  up = np.repeat(np.repeat(pooled, 2, 1), 2, 2)
  hit = got != 0
  assert (s[:, :6, :4][hit[:, :6, :4]] == up[hit[:, :6, :4]]).all()
