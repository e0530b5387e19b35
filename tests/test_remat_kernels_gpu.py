"""The two kernels of csrc/train_remat.hip one at a time on the cases of
tests/remat_cases.py, bit for bit: snnqp_bn_lif_forward_state against the numpy reference of the
fused step and against conv_train.bn_normalise followed by the existing state scan on the device;
snnqp_maxpool2x2_backward_h against the numpy routing and against snnqp_maxpool2x2_backward on the
compare's raster."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import conv_train as ct
from snnquantprune_amd import ops
from tests import remat_cases as rc
from tests import remat_reference as rr
from tests.train_helpers import _frame_untouched, _framed as _framed_at, _np

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -12345.5
NAN = float("nan")
CASES = rc.scan_cases()
_ids = [c[0] for c in CASES]
POOLS = rc.pool_cases()
_framed = partial(_framed_at, pad=37)
_frame_intact = partial(_frame_untouched, pad=37)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _t(a, dev):
  return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the cases are read-only)


def _ptr(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _neuron(c):
  return ops.Neuron(L.NEURON_MULTI_STEP_LIF, c["tau"], c["vth"], c["vr"])


# ---- snnqp_bn_lif_forward_state ----------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fused_scan_is_the_reference_and_the_unfused_sequence(dev, case):
  """T in {6, 1, 0} from zeros and from a given membrane, and every chunking of rc.SPLITS from the
  carried one: h, s and u_T are the numpy reference's and those of bn_normalise followed by
  ops.lif_forward_save(u0=, return_state=True) on the device; what is not wanted is None."""
  c = rc.scan_case(*case[1:])
  nrn = _neuron(c)
  cur, mean, mul, bias = (_t(c[k], dev) for k in ("cur", "mean", "mul", "bias"))
  R, C = c["cur"].shape[1:]

  def unfused(t0, t1, u0):
    y = ct.bn_normalise(cur[t0:t1].clone(), mean[t0:t1], mul[t0:t1], bias)
    return ops.lif_forward_save(y, nrn, u0=u0, return_state=True)

  for T in (rc.T, 1, 0):
    h, s, u = ops.bn_lif_forward(cur[:T], mean[:T], mul[:T], bias, nrn, return_state=True)
    assert tuple(h.shape) == (T, R, C) and tuple(s.shape) == (T, R, C) and tuple(u.shape) == (R, C)
    np.testing.assert_array_equal(_np(h), c["h"][:T])
    np.testing.assert_array_equal(_np(s), c["s"][:T])
    np.testing.assert_array_equal(_np(u), c["starts"][T])
    for a, b in zip((h, s, u), unfused(0, T, None)):
      assert torch.equal(a, b), T
    z = ops.bn_lif_forward(cur[:T], mean[:T], mul[:T], bias, nrn, u0=torch.zeros_like(cur[0]), return_state=True)
    assert all(torch.equal(a, b) for a, b in zip(z, (h, s, u)))
    # from a given membrane: the steps 2..2+T of the whole run
    u2 = _t(c["starts"][2], dev)
    h2, s2, u_T = ops.bn_lif_forward(cur[2:2 + T], mean[2:2 + T], mul[2:2 + T], bias, nrn, u0=u2, return_state=True)
    np.testing.assert_array_equal(_np(h2), c["h"][2:2 + T])
    np.testing.assert_array_equal(_np(s2), c["s"][2:2 + T])
    np.testing.assert_array_equal(_np(u_T), c["starts"][min(2 + T, rc.T)] if T else c["starts"][2])
    assert torch.equal(u2, _t(c["starts"][2], dev))                      # the input is an input
    for a, b in zip((h2, s2, u_T), unfused(2, 2 + T, u2)):
      assert torch.equal(a, b), T
  for W in rc.SPLITS:
    u, hs, ss = None, [], []
    for t0, t1 in rr.chunks(rc.T, W):
      h, s, u = ops.bn_lif_forward(cur[t0:t1], mean[t0:t1], mul[t0:t1], bias, nrn, u0=u, return_state=True)
      np.testing.assert_array_equal(_np(u), c["starts"][t1], err_msg="u_T W=%d chunk %d" % (W, t0))
      hs.append(h)
      ss.append(s)
    np.testing.assert_array_equal(_np(torch.cat(hs)), c["h"])
    np.testing.assert_array_equal(_np(torch.cat(ss)), c["s"])
  # what is not wanted is not returned; without return_state two results
  h, s = ops.bn_lif_forward(cur, mean, mul, bias, nrn, want_h=False)
  assert h is None
  np.testing.assert_array_equal(_np(s), c["s"])
  h, s = ops.bn_lif_forward(cur, mean, mul, bias, nrn, want_s=False)
  assert s is None
  np.testing.assert_array_equal(_np(h), c["h"])


@pytest.mark.parametrize("case", [c for c in CASES if c[2:4] in ((17, 15), (257, 1), (5, 65), (1, 1))],
                         ids=lambda c: c[0])
def test_fused_scan_abi_in_place_state_frames_and_nulls(dev, case):
  """The raw entry with u0 and u_out one buffer, every input framed by NaN and every output by a
  sentinel: the state walks the reference's boundary membranes in place and nothing outside is
  touched; a null h_out or s_out is not written; T == 0 writes u_out = u0 and nothing else."""
  c = rc.scan_case(*case[1:])
  entry = L.lib().snnqp_bn_lif_forward_state
  R, C = c["cur"].shape[1:]
  st = ctypes.byref(_neuron(c).struct())
  bb, vb = _framed(dev, np.array(c["bias"]), NAN)
  bu, vu = _framed(dev, np.zeros((R, C), F32), SENTINEL)
  for t0, t1 in [(0, 2), (2, 2), (2, 5), (5, 6)]:
    n = t1 - t0
    bx, vx = _framed(dev, np.array(c["cur"][t0:t1]), NAN)
    bm, vm = _framed(dev, np.array(c["mean"][t0:t1]), NAN)
    bk, vk = _framed(dev, np.array(c["mul"][t0:t1]), NAN)
    bh, vh = _framed(dev, np.full((n, R, C), SENTINEL, F32), SENTINEL)
    bs, vs = _framed(dev, np.full((n, R, C), SENTINEL, F32), SENTINEL)
    if n == 0:
      L.check(entry(None, None, None, None, 0, R, C, st, _ptr(vu), _ptr(vu), None, None, _stream()))
    else:
      L.check(entry(_ptr(vx), _ptr(vm), _ptr(vk), _ptr(vb), n, R, C, st, _ptr(vu), _ptr(vu), _ptr(vh), _ptr(vs),
                    _stream()))
      np.testing.assert_array_equal(_np(vh), c["h"][t0:t1])
      np.testing.assert_array_equal(_np(vs), c["s"][t0:t1])
    np.testing.assert_array_equal(_np(vu), c["starts"][t1])
    assert _frame_intact(bu, R * C, SENTINEL) and _frame_intact(bh, vh.numel(), SENTINEL)
    assert _frame_intact(bs, vs.numel(), SENTINEL)
    for whole, view in ((bx, vx), (bm, vm), (bk, vk), (bb, vb)):
      assert _frame_intact(whole, view.numel(), NAN)
  # u0 null is zeros; h_out null: s and u_out alone; s_out null: h alone
  x, m, k = (_t(c[key][:2], dev) for key in ("cur", "mean", "mul"))
  bh, vh = _framed(dev, np.full((2, R, C), SENTINEL, F32), SENTINEL)
  bs, vs = _framed(dev, np.full((2, R, C), SENTINEL, F32), SENTINEL)
  vu.fill_(7.0)
  L.check(entry(_ptr(x), _ptr(m), _ptr(k), _ptr(vb), 2, R, C, st, None, _ptr(vu), None, _ptr(vs), _stream()))
  np.testing.assert_array_equal(_np(vs), c["s"][:2])
  np.testing.assert_array_equal(_np(vu), c["starts"][2])
  assert bool((vh == SENTINEL).all()) and _frame_intact(bs, vs.numel(), SENTINEL)
  vs.fill_(SENTINEL)
  L.check(entry(_ptr(x), _ptr(m), _ptr(k), _ptr(vb), 2, R, C, st, None, None, _ptr(vh), None, _stream()))
  np.testing.assert_array_equal(_np(vh), c["h"][:2])
  assert bool((vs == SENTINEL).all()) and _frame_intact(bh, vh.numel(), SENTINEL)
  # T == 0 from a null u0 writes zeros; R == 0 launches nothing
  vu.fill_(7.0)
  L.check(entry(None, None, None, None, 0, R, C, st, None, _ptr(vu), None, None, _stream()))
  assert not _np(vu).any() and _frame_intact(bu, R * C, SENTINEL)
  assert entry(None, None, None, None, 3, 0, C, st, None, None, None, None, _stream()) == L.OK


def test_fused_scan_wrapper_refuses_wrong_shapes(dev):
  msl = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  plif = ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, 0.5, 1.0, 0.0)
  cur = torch.zeros((3, 4, 30), device=dev)
  tc, c = torch.zeros((3, 30), device=dev), torch.zeros(30, device=dev)
  with pytest.raises(ValueError, match="mean and mul"):
    ops.bn_lif_forward(cur, tc[:2], tc, c, msl)
  with pytest.raises(ValueError, match="mean and mul"):
    ops.bn_lif_forward(cur, tc, tc, tc, msl)
  with pytest.raises(ValueError, match="u0"):
    ops.bn_lif_forward(cur, tc, tc, c, msl, u0=torch.zeros((4, 29), device=dev))
  with pytest.raises(L.SnnqpError, match="snnqp_neuron_forward_save_state"):
    ops.bn_lif_forward(cur, tc, tc, c, plif)


# ---- snnqp_maxpool2x2_backward_h ---------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", POOLS, ids=[p[0] for p in POOLS])
def test_pool_routing_from_h(dev, name, shape):
  """Odd sizes, a 1 x 1 image, all-equal windows, planted ties: the numpy routing, and
  ops.maxpool2x2_backward on the raster of the forward's compare; the output inside a sentinel
  frame, the inputs inside NaN ones, and 5-D shapes as the block passes them."""
  c = rc.pool_case(shape)
  NB, H, W, C = shape
  want = rr.pool_route_h(c["h"], c["vth"], c["gp"])
  h, gp = _t(c["h"], dev), _t(c["gp"], dev)
  got = ops.maxpool2x2_backward_h(h, c["vth"], gp)
  np.testing.assert_array_equal(_np(got), want)
  s = ((h - c["vth"]) >= 0).to(torch.float32)
  assert torch.equal(got, ops.maxpool2x2_backward(s, gp))
  got5 = ops.maxpool2x2_backward_h(h[None], c["vth"], gp[None])
  assert tuple(got5.shape) == (1,) + shape and torch.equal(got5[0], got)
  bh, vh = _framed(dev, np.array(c["h"]), NAN)
  bg, vg = _framed(dev, np.array(c["gp"]), NAN)
  bo, vo = _framed(dev, np.full(shape, SENTINEL, F32), SENTINEL)
  L.check(L.lib().snnqp_maxpool2x2_backward_h(_ptr(vh), c["vth"], _ptr(vg) if c["gp"].size else None, NB, H, W, C,
                                              _ptr(vo), _stream()))
  np.testing.assert_array_equal(_np(vo), want)
  assert _frame_intact(bo, vo.numel(), SENTINEL) and _frame_intact(bh, vh.numel(), NAN)
  assert _frame_intact(bg, vg.numel(), NAN)


def test_pool_routing_another_threshold(dev):
  """vth is the kernel's argument, not a constant: the same h at 0.75."""
  c = rc.pool_case((3, 4, 6, 17))
  h, gp = _t(c["h"], dev), _t(c["gp"], dev)
  got = ops.maxpool2x2_backward_h(h, 0.75, gp)
  np.testing.assert_array_equal(_np(got), rr.pool_route_h(c["h"], 0.75, c["gp"]))
  assert not torch.equal(got, ops.maxpool2x2_backward_h(h, c["vth"], gp))
