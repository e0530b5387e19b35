"""The training kernels of csrc/train_dense.hip one at a time, bit for bit against the plain
references of tests/train_reference.py, at the edges of the 16 / 32 / 64 tiles and of the
surrogates.  Where bits cannot be promised (slayer's expf) the bound is derived, not tuned."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import train_reference as tr
from tests.train_helpers import _frame_untouched, _framed as _framed_at, _np, mixed

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _a_operand(rng, kind, shape):
  if kind == "mixed":
    return mixed(rng, shape)
  if kind == "spikes":
    return (rng.random(shape) < 0.3).astype(F32)
  return np.minimum(rng.poisson(1.5, shape), 255).astype(np.uint8)       # counts


def _check_product(got, a_ri, b_rj, mask=None):
  """Bit-equal to the k-ordered chain, and inside gamma_R sum |a||b| of float64."""
  chain = tr.gemm_chain(a_ri, b_rj)
  want = chain if mask is None else chain * mask
  print("differing elements: %d of %d" % (int((got != want).sum()), want.size))
  np.testing.assert_array_equal(got, want)
  R = a_ri.shape[0]
  exact, slack = tr.gemm_f64(a_ri, b_rj), tr.gamma(R) * tr.gemm_mag(a_ri, b_rj)
  assert (np.abs(chain.astype(F64) - exact) <= slack).all()
  if mask is None:
    assert (np.abs(got.astype(F64) - exact) <= slack).all()


# (M, K, N): x [M, K], gI [M, N], w [K, N].  M walks the r chunks of the weight gradient (16 with a
# register prefetch) and the i tiles of the input gradient; K and N sit on the 16 / 32 / 64 edges.
TRIPLES = [
    (0, 17, 33), (0, 1, 1), (1, 1, 1), (1, 65, 17), (1, 16, 129), (3, 15, 15), (3, 129, 1),
    (3, 1, 129), (4, 16, 16), (4, 63, 65), (15, 17, 63), (15, 64, 64), (15, 1, 17), (16, 16, 16),
    (16, 65, 129), (16, 110, 1), (17, 17, 17), (17, 33, 65), (17, 129, 63), (17, 1, 64),
    (31, 31, 31), (31, 64, 110), (31, 15, 1), (33, 65, 17), (33, 17, 65), (33, 63, 33),
    (33, 1, 1), (33, 129, 129), (33, 512, 15), (100, 110, 110), (100, 16, 512), (100, 65, 1),
    (100, 1, 33), (100, 129, 31), (5120, 129, 110), (5120, 1, 1), (5120, 17, 1), (5120, 1, 65),
    (5120, 512, 110), (5120, 2048, 512),
]
_ids = lambda t: "x".join(map(str, t))      # noqa: E731


def _weight_cases():
  for t in TRIPLES:
    for kind in ("mixed", "spikes", "counts"):
      if kind == "mixed" or t != (5120, 2048, 512):
        yield pytest.param(t, kind, id="%s-%s" % (_ids(t), kind))


@pytest.mark.parametrize("shape,kind", list(_weight_cases()))
def test_weight_grad_bit_equal_chain(dev, shape, kind):
  M, K, N = shape
  rng = np.random.default_rng(M * 7919 + K * 131 + N)
  x, gI = _a_operand(rng, kind, (M, K)), mixed(rng, (M, N))
  got = _np(ops.dense_weight_grad(torch.from_numpy(x).to(dev), torch.from_numpy(gI).to(dev)))
  assert got.shape == (K, N) and got.dtype == F32
  _check_product(got, x.astype(F32), gI)
  if M == 0:
    assert not got.any()


@pytest.mark.parametrize("shape", TRIPLES, ids=_ids)
def test_input_grad_bit_equal_chain(dev, shape):
  M, K, N = shape
  rng = np.random.default_rng(M * 7919 + K * 131 + N + 1)
  gI, w = mixed(rng, (M, N)), mixed(rng, (K, N))
  mask = (rng.random((M, K)) < 0.6).astype(F32)
  g, wt = torch.from_numpy(gI).to(dev), torch.from_numpy(w).to(dev)
  plain = _np(ops.dense_input_grad(g, wt))
  masked = _np(ops.dense_input_grad(g, wt, torch.from_numpy(mask).to(dev)))
  ones = _np(ops.dense_input_grad(g, wt, torch.ones((M, K), device=dev)))
  assert plain.shape == (M, K) and plain.dtype == F32
  if M == 0:
    return                                            # an empty tensor, nothing launched
  a_ri, b_rj = np.ascontiguousarray(gI.T), np.ascontiguousarray(w.T)    # r = n
  _check_product(plain, a_ri, b_rj)
  _check_product(masked, a_ri, b_rj, mask)
  np.testing.assert_array_equal(ones, plain)


# ---- raw ABI: strays, empties, error codes -----------------------------------------------------

# the frame of this file is 37 elements: odd, so that the slices are only 4-byte aligned
_framed = partial(_framed_at, pad=37)
_frame_intact = partial(_frame_untouched, pad=37)


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("shape", [(17, 65, 33), (33, 15, 17), (3, 129, 1), (100, 63, 65),
                                   (1, 1, 1), (16, 64, 64), (35, 1, 129)], ids=_ids)
def test_no_stray_read_or_write(dev, shape):
  """Inputs surrounded by NaN, outputs by a sentinel: a read outside a tile that is used puts a
  NaN in the result, a write outside the output moves the sentinel.  Nothing here faults."""
  M, K, N = shape
  rng = np.random.default_rng(M + K + N)
  x, gI, w = mixed(rng, (M, K)), mixed(rng, (M, N)), mixed(rng, (K, N))
  mask = (rng.random((M, K)) < 0.6).astype(F32)
  nan = float("nan")
  (bx, vx), (bg, vg), (bw, vw), (bm, vm) = (_framed(dev, v, nan) for v in (x, gI, w, mask))
  bgw, vgw = _framed(dev, np.zeros((K, N), F32), SENTINEL)
  vgw.fill_(SENTINEL)
  L.check(L.lib().snnqp_dense_weight_grad(_ptr(vx), _ptr(vg), M, K, N, _ptr(vgw), _stream()))
  assert _frame_intact(bgw, K * N, SENTINEL)
  np.testing.assert_array_equal(_np(vgw), tr.gemm_chain(x, gI))
  bgx, vgx = _framed(dev, np.zeros((M, K), F32), SENTINEL)
  vgx.fill_(SENTINEL)
  L.check(L.lib().snnqp_dense_input_grad(_ptr(vg), _ptr(vw), _ptr(vm), M, K, N, _ptr(vgx),
                                         _stream()))
  assert _frame_intact(bgx, M * K, SENTINEL)
  np.testing.assert_array_equal(_np(vgx), tr.gemm_chain(gI.T, w.T) * mask)
  for b, v in ((bx, x), (bg, gI), (bw, w), (bm, mask)):                 # the inputs are inputs
    host = _np(b)
    assert np.isnan(host[:37]).all() and np.isnan(host[37 + v.size:]).all()
    np.testing.assert_array_equal(host[37:37 + v.size].reshape(v.shape), v)


def test_zero_rows(dev):
  """M == 0: the weight gradient is all zeros (written over whatever was there), the input
  gradient is empty."""
  K, N = 65, 17
  gw = torch.full((K, N), SENTINEL, dtype=torch.float32, device=dev)
  L.check(L.lib().snnqp_dense_weight_grad(None, None, 0, K, N, _ptr(gw), _stream()))
  assert not _np(gw).any()
  x, gI = torch.empty((0, K), device=dev), torch.empty((0, N), device=dev)
  got = ops.dense_weight_grad(x, gI)
  assert tuple(got.shape) == (K, N) and not _np(got).any()
  gx = ops.dense_input_grad(gI, torch.ones((K, N), device=dev))
  assert tuple(gx.shape) == (0, K)
  L.check(L.lib().snnqp_dense_input_grad(None, None, None, 0, K, N, None, _stream()))


def test_nan_and_inf_reach_what_the_reference_says(dev):
  M, K, N = 33, 65, 17
  rng = np.random.default_rng(5)
  x = (rng.random((M, K)) < 0.4).astype(F32)                # 0 * inf is a NaN too
  gI, w = mixed(rng, (M, N)), mixed(rng, (K, N))
  gI[20, 3], gI[20, 9] = np.nan, np.inf
  mask = (rng.random((M, K)) < 0.6).astype(F32)
  g = torch.from_numpy(gI).to(dev)
  gw = _np(ops.dense_weight_grad(torch.from_numpy(x).to(dev), g))
  want = tr.gemm_chain(x, gI)
  assert np.isnan(want[:, 3]).all() and np.isfinite(np.delete(want, (3, 9), axis=1)).all()
  assert (np.isnan(want[:, 9]) == (x[20] == 0)).all() and (want[x[20] == 1, 9] == np.inf).all()
  np.testing.assert_array_equal(gw, want)
  gx = _np(ops.dense_input_grad(g, torch.from_numpy(w).to(dev), torch.from_numpy(mask).to(dev)))
  want = tr.gemm_chain(gI.T, w.T) * mask
  assert np.isnan(want[20]).all() and np.isfinite(np.delete(want, 20, axis=0)).all()
  np.testing.assert_array_equal(gx, want)


def test_views_give_the_bits_of_copies(dev):
  M, K, N = 33, 65, 17
  rng = np.random.default_rng(6)
  xb = torch.from_numpy(mixed(rng, (M, 2 * K))).to(dev)
  gb = torch.from_numpy(mixed(rng, (N, M))).to(dev)
  wb = torch.from_numpy(mixed(rng, (K + 3, N + 5))).to(dev)
  mb = torch.from_numpy((rng.random((K, M)) < 0.6).astype(F32)).to(dev)
  x, gI, w, mask = xb[:, ::2], gb.t(), wb[2:K + 2, 1:N + 1], mb.t()
  assert not (x.is_contiguous() or gI.is_contiguous() or w.is_contiguous() or mask.is_contiguous())
  a = ops.dense_weight_grad(x, gI)
  b = ops.dense_weight_grad(x.contiguous(), gI.contiguous())
  assert torch.equal(a, b)
  np.testing.assert_array_equal(_np(a), tr.gemm_chain(_np(x), _np(gI)))
  a = ops.dense_input_grad(gI, w, mask)
  b = ops.dense_input_grad(gI.contiguous(), w.contiguous(), mask.contiguous())
  assert torch.equal(a, b)
  np.testing.assert_array_equal(_np(a), tr.gemm_chain(_np(gI).T, _np(w).T) * _np(mask))
  cnt = torch.from_numpy(_a_operand(rng, "counts", (M, K))).to(dev)        # uint8 rows
  assert torch.equal(ops.dense_weight_grad(cnt, gI), ops.dense_weight_grad(cnt.float(), gI))


def test_grid_limit_is_an_error_not_a_truncation(dev):
  """64-row tiles on grid.y: 65535 tile rows run, 65536 come back as SNNQP_EINVAL untouched."""
  rows_ok, rows_bad = 65535 * 64, 65535 * 64 + 1
  rng = np.random.default_rng(8)
  gI = mixed(rng, (rows_bad, 1))
  g = torch.from_numpy(gI).to(dev)
  w = torch.tensor([[1.5]], dtype=torch.float32, device=dev)
  gx = torch.full((rows_bad, 1), SENTINEL, dtype=torch.float32, device=dev)
  rc = L.lib().snnqp_dense_input_grad(_ptr(g), _ptr(w), None, rows_bad, 1, 1, _ptr(gx), _stream())
  assert rc == L.EINVAL and b"grid too large" in L.lib().snnqp_last_error()
  torch.cuda.synchronize()
  assert bool((gx == SENTINEL).all())
  with pytest.raises(L.SnnqpError):
    ops.dense_input_grad(g, w)
  rc = L.lib().snnqp_dense_input_grad(_ptr(g), _ptr(w), None, rows_ok, 1, 1, _ptr(gx), _stream())
  assert rc == L.OK
  got = _np(gx)
  np.testing.assert_array_equal(got[:rows_ok], gI[:rows_ok] * F32(1.5))
  assert got[rows_ok, 0] == SENTINEL


# ---- snnqp_lif_forward_save --------------------------------------------------------------------

def _neuron(tau, vth, vr):
  return ops.Neuron(L.NEURON_MULTI_STEP_LIF, float(F32(tau)), vth, vr)


def _threshold_currents(tau, vth, vr):
  """Currents x for which the first step's h = fl(fl(x + vr) / tau) equals vth exactly."""
  c = [F32(F32(vth) * F32(tau)) - F32(vr)]
  for _ in range(64):
    c = [np.nextafter(c[0], F32(-np.inf))] + c + [np.nextafter(c[-1], F32(np.inf))]
  c = np.array(c, F32)
  h = ((c - (F32(0) - F32(vr))) / F32(tau)).astype(F32)
  return c[h - F32(vth) == 0]


@pytest.mark.parametrize("vr", [0.0, 0.1])
@pytest.mark.parametrize("vth", [1.0, 0.7])
@pytest.mark.parametrize("tau", [2.0, 3.0, 4.0, 1.5])
def test_lif_forward_save_bit_equal_oracle(dev, tau, vth, vr):
  """h - vth cannot be subnormal at these thresholds (float32 neighbours of 0.7 or 1 differ from
  it by 2^-25 or more, or not at all), so the subnormal values planted are currents: with
  v_reset = 0 their h = x / tau is subnormal too and must not be flushed."""
  nrn = _neuron(tau, vth, vr)
  hit = _threshold_currents(tau, vth, vr)
  assert hit.size > 0
  for T in (0, 1, 2, 33):
    for R, C in ((1, 1), (3, 85), (16, 16), (1, 257), (70, 110)):
      rng = np.random.default_rng(T * 1000 + R * C)
      cur = (0.6 * F32(vth) * F32(tau) + 1.2 * rng.standard_normal((T, R, C))).astype(F32)
      flat = cur.reshape(T, R * C)
      if T:
        flat[0, 0] = hit[0]
        sub = np.array([2.0 ** -140, -(2.0 ** -149), 3 * 2.0 ** -130], F32)
        k = min(3, R * C - 1)
        flat[:, 1:1 + k] = sub[:k]
      h, s = ops.lif_forward_save(torch.from_numpy(cur).to(dev), nrn)
      assert tuple(h.shape) == (T, R, C) and tuple(s.shape) == (T, R, C)
      if T == 0:
        continue
      want_h, want_s = tr.lif_save_ref(cur, tau, vth, vr)
      assert want_h.reshape(T, -1)[0, 0] - F32(vth) == 0 and want_s.reshape(T, -1)[0, 0] == 1
      if vr == 0.0 and R * C > 1:
        tiny = np.abs(want_h.reshape(T, -1)[:, 1:1 + k])
        assert ((tiny > 0) & (tiny < 2.0 ** -126)).any()
      if R * C > 16:
        assert 0.02 < want_s.mean() < 0.98
      np.testing.assert_array_equal(_np(h), want_h, err_msg="h T=%d R=%d C=%d" % (T, R, C))
      np.testing.assert_array_equal(_np(s), want_s, err_msg="s T=%d R=%d C=%d" % (T, R, C))
      u_eval, s_eval = ops.lif_forward(torch.from_numpy(cur).to(dev), nrn)
      assert torch.equal(s_eval, s)
      u_last = torch.where(s[-1] != 0, torch.full_like(h[-1], float(F32(vr))), h[-1])
      assert torch.equal(u_eval, u_last)
  h, s = ops.lif_forward_save(torch.empty((5, 0, 7), device=dev), nrn)
  assert tuple(h.shape) == (5, 0, 7) and tuple(s.shape) == (5, 0, 7)


# ---- snnqp_lif_backward ------------------------------------------------------------------------

SURR = {"fast_sigmoid": L.SURR_FAST_SIGMOID, "atan": L.SURR_ATAN, "slayer": L.SURR_SLAYER,
        "smooth_step": L.SURR_SMOOTH_STEP, "piecewise_linear": L.SURR_PIECEWISE_LINEAR}
EDGES = {1.0: {-0.5, 0.0, 0.5, 0.25, -0.25}, 0.7: {-0.5, 0.0, 0.25, -0.25}}   # tr.planted_h


def _backward_case(vth, shape=(9, 7, 37), seed=12):
  rng = np.random.default_rng(seed)
  h, reached = tr.planted_h(rng, shape, vth, shift=-0.5)
  assert reached >= EDGES[vth]
  rate = ((h - F32(vth)) >= 0).mean()
  assert 0.05 <= rate <= 0.5, rate
  return h, mixed(rng, shape)


@pytest.mark.parametrize("vth", [1.0, 0.7])
@pytest.mark.parametrize("tau", [2.0, 3.0])
@pytest.mark.parametrize("name", ["fast_sigmoid", "atan", "smooth_step", "piecewise_linear"])
def test_lif_backward_bit_equal_recurrence(dev, name, tau, vth):
  h, gs = _backward_case(vth)
  got = _np(ops.lif_backward(torch.from_numpy(h).to(dev), _neuron(tau, vth, 0.0), SURR[name],
                             gs=torch.from_numpy(gs).to(dev)))
  want = tr.lif_backward_ref32(h, gs, tau, vth, name)
  print("differing elements: %d of %d" % (int((got != want).sum()), want.size))
  np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("vth", [1.0, 0.7])
@pytest.mark.parametrize("tau", [2.0, 3.0])
def test_lif_backward_slayer_inside_bound(dev, tau, vth):
  """expf is not bit-exact against numpy; the bound is the magnitude recurrence of
  tr.lif_backward_ref64 with sigma' charged 2 ulp.  Largest error / bound measured on MI355X:
  0.44 / 0.43 (tau 2, threshold 1 / 0.7) and 0.49 / 0.50 (tau 3); DESIGN.md section 10."""
  h, gs = _backward_case(vth)
  got = _np(ops.lif_backward(torch.from_numpy(h).to(dev), _neuron(tau, vth, 0.0),
                             SURR["slayer"], gs=torch.from_numpy(gs).to(dev)))
  ref, bound = tr.lif_backward_ref64(h, gs, tau, vth, "slayer")
  ratio = np.abs(got.astype(F64) - ref) / bound
  print("slayer tau=%g vth=%g: largest error / bound %.4f" % (tau, vth, ratio.max()))
  assert (ratio <= 1.0).all(), ratio.max()


@pytest.mark.parametrize("C,group", [(C, g) for C in (10, 110, 30) for g in sorted({1, 10, C})])
@pytest.mark.parametrize("name", ["atan", "slayer"])
def test_lif_backward_vote_equals_expanded_upstream(dev, name, C, group):
  T, R = 7, 5
  rng = np.random.default_rng(C + group)
  h, _ = tr.planted_h(rng, (T, R, C), 1.0, shift=-0.5)
  gl = mixed(rng, (R, C // group))
  gs = np.broadcast_to((np.repeat(gl, group, axis=1) / F32(group * T)).astype(F32)[None],
                       (T, R, C)).copy()
  nrn = _neuron(3.0, 1.0, 0.0)
  ht = torch.from_numpy(h).to(dev)
  fused = ops.lif_backward(ht, nrn, SURR[name], glogits=torch.from_numpy(gl).to(dev), group=group)
  plain = ops.lif_backward(ht, nrn, SURR[name], gs=torch.from_numpy(gs).to(dev))
  assert torch.equal(fused, plain)
  if name != "slayer":
    np.testing.assert_array_equal(_np(fused), tr.lif_backward_ref32(h, gs, 3.0, 1.0, name))


def test_lif_backward_refusals_and_empties(dev):
  nrn = _neuron(2.0, 1.0, 0.0)
  h = torch.zeros((3, 4, 30), device=dev)
  gs, gl = torch.zeros((3, 4, 30), device=dev), torch.zeros((4, 3), device=dev)
  for kw in (dict(glogits=torch.zeros((4, 4), device=dev), group=7), dict(gs=gs, glogits=gl),
             dict()):
    with pytest.raises(L.SnnqpError) as e:
      ops.lif_backward(h, nrn, L.SURR_ATAN, **kw)
    assert e.value.code == L.EINVAL
  with pytest.raises(L.SnnqpError):
    ops.lif_backward(h, nrn, 99, gs=gs)
  for shape in ((0, 4, 30), (3, 0, 30)):
    e = torch.empty(shape, device=dev)
    assert tuple(ops.lif_backward(e, nrn, L.SURR_ATAN, gs=e).shape) == shape
    gle = torch.zeros((shape[1], 3), device=dev)
    assert tuple(ops.lif_backward(e, nrn, L.SURR_ATAN, glogits=gle, group=10).shape) == shape
