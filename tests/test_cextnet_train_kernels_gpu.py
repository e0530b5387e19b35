"""The two kernels of csrc/train_gate.hip against their references (tests/cextnet_train_reference.py),
bit for bit: NaN-framed inputs, sentinel-framed outputs, at the channel counts around the wave and
block sizes and the rasters with no window, one window and trailing odd rows and columns."""

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import cextnet_train_reference as xr
from tests.train_helpers import _frame_untouched, _framed, _np, mixed

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -12345.5
CHANNELS = (1, 31, 32, 33, 64, 65, 128)
RASTERS = ((1, 1), (2, 2), (2, 3), (3, 2), (5, 7), (8, 8), (16, 16))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _run(dev, x, gate, gp, gm):
  """Both entry points on NaN-framed inputs into sentinel-framed outputs -> (ggate, gx)."""
  NB, H, W, C = x.shape
  lib = L.lib()
  keep = [_framed(dev, a, np.nan) for a in (x, gate, gp, gm)]
  (_, xv), (_, gv), (_, pv), (_, mv) = keep
  gw, go = _framed(dev, np.full((NB, C), SENTINEL, F32), SENTINEL)
  xw, xo = _framed(dev, np.full(x.shape, SENTINEL, F32), SENTINEL)
  ptr = lambda t: ops._ptr(t) if t.numel() else None                # noqa: E731
  L.check(lib.snnqp_gate_pool_grad_gate(ptr(xv), ptr(gv), ptr(pv), NB, H, W, C, ptr(go), ops._stream()))
  L.check(lib.snnqp_gate_pool_grad_input(ptr(xv), ptr(gv), ptr(pv), ptr(mv), NB, H, W, C, ptr(xo),
                                         ops._stream()))
  torch.cuda.synchronize()
  assert _frame_untouched(gw, go.numel(), SENTINEL) and _frame_untouched(xw, xo.numel(), SENTINEL)
  return _np(go), _np(xo)


def _inputs(rng, NB, H, W, C, spikes):
  if spikes:
    x = (rng.random((NB, H, W, C)) < 0.4).astype(F32)
  else:
    x = rng.integers(-3, 4, (NB, H, W, C)).astype(F32) * F32(0.37)   # few distinct values: ties
    x += (rng.random(x.shape) < 0.5) * mixed(rng, x.shape)           # ... among general ones
    x = x.astype(F32)
  if NB and H >= 2 and W >= 2:
    x[0, 0:2, 0:2] = x[0, 0, 0]                                      # a window with all four equal
  gate = (1.0 / (1.0 + np.exp(-2.0 * rng.standard_normal((NB, C))))).astype(F32)
  if NB:
    gate[0, C // 2] = 0.0                                            # a channel with gate == 0
  gp = mixed(rng, (NB, H // 2, W // 2, C))
  gm = mixed(rng, (NB, C))
  return x, gate, gp, gm


@pytest.mark.parametrize("hw", RASTERS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C", CHANNELS)
def test_kernels_bit_equal_reference(dev, C, hw):
  H, W = hw
  rng = np.random.default_rng(1000 * C + 10 * H + W)
  for NB in (0, 1, 3):
    for spikes in (False, True):
      x, gate, gp, gm = _inputs(rng, NB, H, W, C, spikes)
      ggate, gx = _run(dev, x, gate, gp, gm)
      if NB == 0:
        continue                                                     # nothing written, frames intact
      np.testing.assert_array_equal(ggate, xr.gate_grad_gate_ref(x, gate, gp))
      np.testing.assert_array_equal(gx, xr.gate_grad_input_ref(x, gate, gp, gm))
      if H < 2 or W < 2:
        assert not ggate.any()


def test_no_images_write_nothing(dev):
  """NB == 0: SNNQP_OK, no pointer is looked at."""
  lib = L.lib()
  assert lib.snnqp_gate_pool_grad_gate(None, None, None, 0, 8, 8, 32, None, ops._stream()) == L.OK
  assert lib.snnqp_gate_pool_grad_input(None, None, None, None, 0, 8, 8, 32, None, ops._stream()) == L.OK
  e = torch.empty((0, 8, 8, 32), device=dev)
  assert tuple(ops.gate_pool_grad_gate(e, e[:, 0, 0], e[:, :4, :4]).shape) == (0, 32)
  assert tuple(ops.gate_pool_grad_input(e, e[:, 0, 0], e[:, :4, :4], e[:, 0, 0]).shape) == (0, 8, 8, 32)


def test_nan_and_inf_in_gp(dev):
  rng = np.random.default_rng(8)
  x, gate, gp, gm = _inputs(rng, 2, 6, 6, 33, False)
  gp[0, 1, 1, 3] = np.nan
  gp[1, 2, 0, 5] = np.inf
  gp[1, 0, 2, 16] = -np.inf                    # channel 16 of image 1 ...
  gate[1, 16] = 0.0                            # ... with gate == 0: inf * 0 in the route
  ggate, gx = _run(dev, x, gate, gp, gm)
  want_g, want_x = xr.gate_grad_gate_ref(x, gate, gp), xr.gate_grad_input_ref(x, gate, gp, gm)
  np.testing.assert_array_equal(ggate, want_g)
  np.testing.assert_array_equal(gx, want_x)
  assert np.isnan(want_g[0, 3]) and not np.isfinite(want_g[1, 5]) and np.isnan(want_x[1, :, :, 16]).any()
  assert np.isfinite(want_g).sum() >= want_g.size - 3


def test_wrappers_and_reproducibility(dev):
  """ops.gate_pool_grad_* on [T, B, ...] tensors at the model's geometry, twice: the same bits."""
  rng = np.random.default_rng(21)
  T, B, H, W, C = 4, 3, 16, 16, 128
  x, gate, gp, gm = _inputs(rng, T * B, H, W, C, True)
  dv = lambda a, *lead: torch.from_numpy(a).to(dev).reshape(tuple(lead) + a.shape[1:])   # noqa: E731
  xt, gt, pt, mt = (dv(a, T, B) for a in (x, gate, gp, gm))
  runs = [(_np(ops.gate_pool_grad_gate(xt, gt, pt)), _np(ops.gate_pool_grad_input(xt, gt, pt, mt)))
          for _ in range(2)]
  assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
  assert runs[0][0].shape == (T, B, C) and runs[0][1].shape == (T, B, H, W, C)
  np.testing.assert_array_equal(runs[0][0].reshape(T * B, C), xr.gate_grad_gate_ref(x, gate, gp))
  np.testing.assert_array_equal(runs[0][1].reshape(x.shape), xr.gate_grad_input_ref(x, gate, gp, gm))


def test_more_than_one_block_per_kernel(dev):
  """NB C past one 256-lane block of the gate kernel with a short last block, real-valued x."""
  rng = np.random.default_rng(5)
  x, gate, gp, gm = _inputs(rng, 5, 7, 9, 65, False)             # 325 lanes: two blocks, 69 in the last
  ggate, gx = _run(dev, x, gate, gp, gm)
  np.testing.assert_array_equal(ggate, xr.gate_grad_gate_ref(x, gate, gp))
  np.testing.assert_array_equal(gx, xr.gate_grad_input_ref(x, gate, gp, gm))


# ---- the float64-chain conv weight gradient (the model's first block) --------------------------------

WGRAD_CASES = [
    # NB, H, W, Cin, Cout, kernel, strides, pads
    (1, 1, 1, 1, 1, (1, 1), (1, 1), ((0, 0), (0, 0))),
    (2, 8, 8, 2, 16, (3, 3), (1, 1), ((1, 1), (1, 1))),        # the first block's geometry, one range
    (3, 20, 19, 2, 33, (3, 3), (1, 1), ((1, 1), (1, 1))),      # 1140 rows: two ranges of 570
    (5, 21, 21, 3, 5, (3, 3), (1, 1), ((1, 1), (1, 1))),       # 2205 rows: three ranges of 735
    (1, 25, 41, 2, 7, (3, 3), (1, 1), ((1, 1), (1, 1))),       # 1025 rows: ranges of 513 and 512 (a short last one)
    (2, 9, 7, 3, 65, (2, 3), (2, 1), ((0, 1), (2, 0))),        # strides, uneven padding, 65 lanes in a row
    (1, 1, 6, 4, 4, (1, 4), (1, 1), ((0, 0), (1, 2))),         # a 1-D geometry
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c[:5])))
def test_weight_grad_f64_bit_equal_reference(dev, case):
  import ctypes
  from tests import conv_train_reference as cr
  NB, H, W, Cin, Cout, ks, st, pads = case
  rng = np.random.default_rng(NB * 100 + H)
  geom = ops.ConvGeom(H, W, Cin, Cout, ks[0], ks[1], st, pads)
  OH, OW = geom.out_hw()
  x = np.minimum(rng.poisson(0.6, (NB, H, W, Cin)), 255).astype(F32) + (rng.random((NB, H, W, Cin)) < 0.2) * mixed(rng, (NB, H, W, Cin))
  x = x.astype(F32)
  gI = mixed(rng, (NB, OH, OW, Cout))
  (_, xv), (_, gv) = _framed(dev, x, np.nan), _framed(dev, gI, np.nan)
  g = geom.struct()
  nbytes = L.lib().snnqp_conv_weight_grad_f64_workspace_bytes(ctypes.byref(g), NB)
  assert nbytes == len(xr.wgrad_f64_ranges(NB * OH * OW)) * ks[0] * ks[1] * Cin * Cout * 8
  ws = torch.full((nbytes // 8 + 16,), float("nan"), dtype=torch.float64, device=dev)
  shape = (ks[0], ks[1], Cin, Cout)
  ow, ov = _framed(dev, np.full(shape, SENTINEL, F32), SENTINEL)
  L.check(L.lib().snnqp_conv_weight_grad_f64(ops._ptr(xv), ops._ptr(gv), NB, ctypes.byref(g), ops._ptr(ws),
                                             ops._ptr(ov), ops._stream()))
  torch.cuda.synchronize()
  assert _frame_untouched(ow, ov.numel(), SENTINEL)
  assert bool(torch.isnan(ws[nbytes // 8:]).all())                 # nothing past the stated workspace
  want = xr.wgrad_f64_ref(x, gI, ks, st, pads)
  np.testing.assert_array_equal(_np(ov), want)
  again = _np(ops.conv_weight_grad_f64(xv, gv, geom))
  assert again.tobytes() == want.tobytes()
  # and it is the float64 product rounded once, to a few units of float64 roundoff of the magnitudes
  a, b = cr.wgrad_matrices(x, gI, ks, st, pads)
  exact = a.astype(np.float64).T @ b.astype(np.float64)
  mag = np.abs(a.astype(np.float64)).T @ np.abs(b.astype(np.float64))
  assert (np.abs(want.reshape(exact.shape) - exact) <= 2.0 ** -24 * np.abs(exact) + a.shape[0] * 2.0 ** -52 * mag + 2.0 ** -149).all()


def test_weight_grad_f64_no_images_and_nonfinite(dev):
  import ctypes
  geom = ops.ConvGeom(4, 4, 2, 5, 3, 3, (1, 1), ((1, 1), (1, 1)))
  g = geom.struct()
  ws = torch.empty(3 * 3 * 2 * 5, dtype=torch.float64, device=dev)
  gw = torch.full((3, 3, 2, 5), SENTINEL, dtype=torch.float32, device=dev)
  L.check(L.lib().snnqp_conv_weight_grad_f64(None, None, 0, ctypes.byref(g), ops._ptr(ws), ops._ptr(gw),
                                             ops._stream()))
  assert bool((gw == 0).all())
  rng = np.random.default_rng(3)
  x = rng.standard_normal((2, 4, 4, 2)).astype(F32)
  gI = mixed(rng, (2, 4, 4, 5))
  gI[0, 1, 1, 2] = np.nan
  gI[1, 3, 0, 4] = np.inf
  got = _np(ops.conv_weight_grad_f64(torch.from_numpy(x).to(dev), torch.from_numpy(gI).to(dev), geom))
  want = xr.wgrad_f64_ref(x, gI, (3, 3), (1, 1), ((1, 1), (1, 1)))
  np.testing.assert_array_equal(got, want)
  assert np.isnan(want[..., 2]).any() and np.isfinite(want[..., 0]).all()
