"""GPU suite: the float32-MFMA connection (csrc/fseq_gemm.hip) alone, one launch of
snnqp_conv_forward per entry of tests/fseq_cases.py -- all 14 instantiations of the kernel, both
tiles at their ragged edges -- bit for bit against the plain im2col + fmaf-chain reference, into a
framed output, with the dispatch query naming the instantiation on the real tensors."""
import ctypes
import time

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import fseq_cases as fc
from tests.train_helpers import PAD, _frame_untouched, _framed, _np

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  L.lib()
  return torch.device("cuda:0")


def _framed_int(dev, a, dtype, fill, offset=0):
  """A device copy of the integer array `a` inside a frame of `fill`, `offset` elements past an
  aligned address: (whole, view)."""
  whole = torch.full((a.size + 2 * PAD + 16,), fill, dtype=dtype, device=dev)
  assert whole.data_ptr() % 16 == 0
  view = whole[PAD + offset:PAD + offset + a.size].view(a.shape)
  view.copy_(torch.from_numpy(np.array(a)).view(dtype))          # (a copy: the shared data is read-only)
  return whole, view


def _device_input(dev, c):
  """The case's x on the device as the kernel reads it, framed with what an out-of-range read
  would show in the result: NaN / 255 / all-ones words."""
  xk = fc.data(c.name)[0]
  if c.kind == "f32":
    keep, xv = _framed(dev, xk.copy(), np.nan)
    assert xv.data_ptr() % 16 == 0
    return keep, xv, xv
  if c.kind == "u8":
    keep, xv = _framed_int(dev, xk, torch.uint8, 255, c.offset)
    assert xv.data_ptr() % 8 == c.offset % 8
    return keep, xv, xv
  keep, xv = _framed_int(dev, xk.view(np.int32), torch.int32, -1)
  return keep, xv, ops.PackedSpikes(xv, c.Cin)


def _launch(dev, c, xv, wv, geom, NB=None):
  shape = (c.NB, c.H, c.W, c.Cout)
  ow, ov = _framed(dev, np.full(shape, SENTINEL, F32), SENTINEL)
  g, w = geom.struct(), ops.Weight(L.W_F32, wv).struct()
  L.check(L.lib().snnqp_conv_forward(ops._ptr(xv), fc.IN_TYPES[c.kind], c.NB if NB is None else NB,
                                     ctypes.byref(g), ctypes.byref(w), ops._ptr(ov), None, ops._stream()))
  torch.cuda.synchronize()
  assert _frame_untouched(ow, ov.numel(), SENTINEL), c.name + ": wrote outside y"
  return ov


@pytest.mark.parametrize("c", fc.CASES, ids=[c.name for c in fc.CASES])
def test_connection_bit_equal_reference(dev, c):
  t0 = time.perf_counter()
  want = fc.reference(c.name)
  t1 = time.perf_counter()
  _, _, w = fc.data(c.name)
  M, K, N = fc.dims(c)
  geom = ops.ConvGeom(c.H, c.W, c.Cin, N, c.ks[0], c.ks[1], (1, 1), c.pads)
  assert geom.out_hw() == (c.H, c.W)
  keep_x, xv, xq = _device_input(dev, c)
  keep_w, wv = _framed(dev, w.reshape(K, N).copy(), np.nan)
  assert wv.data_ptr() % 16 == 0
  assert ops.conv_float_form(xq, geom, ops.Weight(L.W_F32, wv)) == (c.kind,) + c.form
  got = _np(_launch(dev, c, xv, wv, geom))
  diff = int((got.view(np.uint32) != want.view(np.uint32)).sum()) if not c.nonfinite else -1
  print("%s: M %d K %d N %d form %s: differing elements %d of %d (reference %.3f s, GPU part %.3f s)"
        % (c.name, M, K, N, c.form, diff, want.size, t1 - t0, time.perf_counter() - t1))
  assert not (got == SENTINEL).any(), "an output was not written"
  np.testing.assert_array_equal(got, want)                  # (NaN equals NaN here)
  if c.nonfinite:
    assert np.isnan(want).any() and np.isinf(fc.data(c.name)[1]).any()
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))
  else:
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  again = _np(_launch(dev, c, xv, wv, geom))
  np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))
  assert ops.device_status() == 0


@pytest.mark.parametrize("name", ["f32_m0_cin16_1x1", "u8_m3_dense_k24", "bits_m3_cin32_3x3"])
def test_no_images_write_nothing(dev, name):
  c = fc.BY_NAME[name]
  _, _, w = fc.data(name)
  M, K, N = fc.dims(c)
  geom = ops.ConvGeom(c.H, c.W, c.Cin, N, c.ks[0], c.ks[1], (1, 1), c.pads)
  keep_x, xv, _ = _device_input(dev, c)
  keep_w, wv = _framed(dev, w.reshape(K, N).copy(), np.nan)
  ov = _launch(dev, c, xv, wv, geom, NB=0)                  # rc OK (L.check), frame untouched
  assert bool((ov == SENTINEL).all())
  assert ops.device_status() == 0
