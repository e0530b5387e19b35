"""The direct-form block (csrc/generic_block.hip) against the oracle off the 3x3 / stride 1 / pad 1
path: the geometries of tests/generic_cases.py -- strides, VALID and explicit padding, kernels
other than 3x3, input and kernel dilation, feature groups on bit-packed input, 1-D and 3-D --
as fused blocks (BatchNorm + neuron over T + u0 carry + spike raster) and as connections alone.
Potentials and rasters bit for bit; tests/test_generic_block_cpu.py pins the oracle at the same
geometries against torch.  The stress property tests (tests/stress.py) call an MFMA kernel right
when it equals this kernel, so this file is what their verdict rests on.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import generic_cases as gc
from tests.helpers import packbits_lastaxis

pytestmark = pytest.mark.gpu
F32 = np.float32
BITS = [b for b, _ in gc.CODES]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()                      # fails loudly if the HIP extension is missing
  return torch.device("cuda:0")


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(x):
  from snnquantprune_amd import ops
  if isinstance(x, ops.PackedSpikes):
    return x.bits.cpu().numpy().view(np.uint32)
  return x.cpu().numpy()


def _packed_kernel(leaf, bits, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  desc = QuantDesc(L.Q_DUQ, bits, a, c, float(2 ** (bits - 1) - 1), c)
  return packing.PackedKernel(_t(leaf["kernel"], dev), desc, _t(leaf["prune_0"]["mask"], dev))


def _last_error():
  from snnquantprune_amd import _lib as L
  return L.lib().snnqp_last_error().decode("utf-8", "replace")


def _mslif():
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  return ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)


def _bn(o, bn, dev, flags=0):
  from snnquantprune_amd import ops
  mean, mul, bias = o.bn_coeffs(bn["mean"], bn["var"], bn["scale"], bn["bias"])
  return ops.BnCoeffs(_t(mean, dev), _t(mul, dev), _t(bias, dev), flags)


def _geom(o, g):
  """The geometry as the library takes it, padding resolved by the oracle (1-D: H = 1)."""
  from snnquantprune_amd import ops
  nsp = len(g.spatial)
  pads = o.resolve_padding(g.spatial, g.kernel, g.strides, g.padding)
  in_dil = tuple(g.in_dil or (1,) * nsp)
  k_dil = tuple(g.k_dil or (1,) * nsp)
  if nsp == 3:
    return ops.Conv3dGeom(*g.spatial, g.cin, g.cout, *g.kernel, tuple(g.strides), tuple(pads), in_dil, k_dil,
                          g.groups)
  if nsp == 1:
    return ops.ConvGeom(1, g.spatial[0], g.cin, g.cout, 1, g.kernel[0], (1, g.strides[0]), ((0, 0), pads[0]),
                        (1, in_dil[0]), (1, k_dil[0]), g.groups)
  return ops.ConvGeom(g.spatial[0], g.spatial[1], g.cin, g.cout, g.kernel[0], g.kernel[1], tuple(g.strides),
                      tuple(pads), in_dil, k_dil, g.groups)


def _as_h1(g, a, lead):
  """A 1-D case as the kernel sees it: a height axis of 1 behind the `lead` leading axes."""
  return a if len(g.spatial) != 1 else np.expand_dims(a, lead)


_CASES = {}


def _case(o, name, bits):
  """The case with the oracle's block in both arithmetic modes, computed once and left unchanged."""
  key = (name, bits)
  if key not in _CASES:
    c = gc.build(o, name, bits)
    okw = gc.oracle_kwargs(c["g"])
    c["int"] = o.conv_block(c["x"], c["qw"], c["bn"], None, "int", u0=c["u0"], **okw)
    for a in c["int"]:
      a.setflags(write=False)
    _CASES[key] = c
  return _CASES[key]


def _block(o, c, dev, x, w, nrn=None, bn=None, u0="case", want_u=True, packed_out=True, fmt="u8",
           time_major=True):
  """One launch of the direct-form block on x [T, B, *spatial, Cin] (numpy) in the input format
  `fmt` ("u8", "bits", "f32") -> (u_T | None, raster) as numpy in the oracle's shapes (raster: the
  packed words, or float32)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  g = c["g"]
  geom = _geom(o, g)
  nrn = nrn or _mslif()
  bn = _bn(o, c["bn"], dev) if bn is None else bn
  u0 = c["u0"] if isinstance(u0, str) else u0
  xk = _as_h1(g, x, 2)
  if not time_major:
    xk = np.swapaxes(xk, 0, 1)
  xin = _t(xk.astype(F32) if fmt == "f32" else xk, dev)
  if fmt == "bits":
    xin = ops.pack_bits(xin)
  u0k = None if u0 is None else _t(_as_h1(g, u0, 1), dev)
  if len(g.spatial) == 3:
    assert time_major
    u, s = ops.conv3d_lif_forward(xin, geom, w, nrn, bn=bn, u0=u0k, want_u=want_u, packed_out=packed_out)
  else:
    u, s = ops.conv_lif_forward(xin, geom, w, nrn, bn=bn, u0=u0k, want_u=want_u, packed_out=packed_out,
                                impl=L.IMPL_GENERIC, time_major=time_major)
  u, s = (None if u is None else _np(u)), _np(s)
  if len(g.spatial) == 1:
    u, s = (None if u is None else u[:, 0]), s[:, :, 0]
  return u, s


def _check(u, s, eu, es, packed_out, tag):
  np.testing.assert_array_equal(s, packbits_lastaxis(es) if packed_out else es, err_msg=tag)
  if u is not None:
    np.testing.assert_array_equal(u, eu, err_msg=tag)


# ---------------------------------------------------------------------------
# integer blocks, every row
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", gc.NAMES)
def test_generic_int_block_every_geometry(dev, oracle, name, bits):
  """ops.conv_lif_forward(impl=IMPL_GENERIC) / ops.conv3d_lif_forward with a carried-in u0: uint8 and
  bit-packed input, time-major and batch-major, bit-packed and float32 spikes, with and without u_T;
  then the scan split 2 + 2 with u_T carried over."""
  from snnquantprune_amd import ops
  c = _case(oracle, name, bits)
  eu, es = c["int"]
  w = _packed_kernel(c["leaf"], bits, dev).int_weight()
  three_d = len(c["g"].spatial) == 3
  for fmt in ("u8", "bits"):
    for tm in ((True,) if three_d else (True, False)):
      for packed_out in (True, False):
        for want_u in (True, False):
          u, s = _block(oracle, c, dev, c["x"], w, fmt=fmt, time_major=tm, packed_out=packed_out, want_u=want_u)
          assert (u is None) == (not want_u)
          _check(u, s, eu, es, packed_out, "%s tm %s packed %s u %s" % (fmt, tm, packed_out, want_u))
  for fmt in ("u8", "bits"):
    u1, s1 = _block(oracle, c, dev, c["x"][:2], w, fmt=fmt)
    u2, s2 = _block(oracle, c, dev, c["x"][2:], w, fmt=fmt, u0=u1)
    _check(u2, np.concatenate([s1, s2]), eu, es, True, "split scan " + fmt)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# the fused 2x2 pool
# ---------------------------------------------------------------------------


def _conv_lif_if(pred, xin, in_type, T, B, geom, w, bn, nrn, u0, u_out, s, s_type, pool):
  """snnqp_conv_lif_forward_if on time-major input, return code unchecked: the one entry that hands
  a pool to the direct-form kernel (snnqp_conv_lif_forward refuses pool = 2 with it and the caller
  pools the raster afterwards)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  g, ws, n = geom.struct(), w.struct(), nrn.struct()
  b = bn.struct() if bn is not None else None
  unit = geom.H * geom.W * xin.shape[-1]
  return L.lib().snnqp_conv_lif_forward_if(
      ops._ptr(pred), ops._ptr(xin), in_type, B * unit, unit, T, B, ctypes.byref(g), ctypes.byref(ws),
      ctypes.byref(b) if b is not None else None, ctypes.byref(n), ops._ptr(u0), ops._ptr(u_out), ops._ptr(s),
      s_type, pool, ops._stream())


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", ["depthwise", "k5_stride2_valid"])
def test_generic_block_fused_pool(dev, oracle, name, bits):
  """pool = 2 in the direct-form kernel (a thread owns a 2x2 window) on an even output (8x6) and an
  odd one (5x7 -> 2x3): the pooled raster equals oracle.max_pool_2x2 of the oracle's raster, and with
  u_T wanted the walk covers ceil(FH / 2) x ceil(FW / 2) windows, so the potentials of the last row
  and column the pool drops equal the oracle's too.  Integer codes on uint8 and bit-packed input, and
  the float32 kernel (the `fseq` contract) on uint8 input."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  c = _case(oracle, name, bits)
  g = c["g"]
  geom = _geom(oracle, g)
  OH, OW = g.out
  pk = _packed_kernel(c["leaf"], bits, dev)
  okw = gc.oracle_kwargs(g)
  fseq = oracle.conv_block(c["x"], c["qw"], c["bn"], None, "fseq", u0=c["u0"], **okw)
  bn, nrn = _bn(oracle, c["bn"], dev), _mslif()
  one = torch.ones(1, dtype=torch.int32, device=dev)
  x8 = _t(c["x"], dev)
  CW = (g.cout + 31) // 32
  for w, fmt, (eu, es) in ((pk.int_weight(), "u8", c["int"]), (pk.int_weight(), "bits", c["int"]),
                           (pk.float_weight(), "u8", fseq)):
    ep = oracle.max_pool_2x2(es)
    assert ep.shape[2:4] == (OH // 2, OW // 2)
    xin, in_type = (x8, L.U8) if fmt == "u8" else (ops.pack_bits(x8).bits, L.BITS)
    for packed_out in (True, False):
      for want_u in (True, False):
        tag = "%s wtype %d packed %s u %s" % (fmt, w.wtype, packed_out, want_u)
        u = torch.full((g.B, OH, OW, g.cout), float("nan"), device=dev) if want_u else None
        if packed_out:
          s = torch.full((gc.T, g.B, OH // 2, OW // 2, CW), -1, dtype=torch.int32, device=dev)
        else:
          s = torch.full((gc.T, g.B, OH // 2, OW // 2, g.cout), float("nan"), device=dev)
        L.check(_conv_lif_if(one, xin, in_type, gc.T, g.B, geom, w, bn, nrn, _t(c["u0"], dev), u, s,
                             L.BITS if packed_out else L.F32, 2))
        got = _np(s).view(np.uint32) if packed_out else _np(s)
        np.testing.assert_array_equal(got, packbits_lastaxis(ep) if packed_out else ep, err_msg=tag)
        if want_u:
          np.testing.assert_array_equal(_np(u), eu, err_msg=tag)
          np.testing.assert_array_equal(_np(u)[:, OH - 1], eu[:, OH - 1], err_msg=tag + " last row")
          np.testing.assert_array_equal(_np(u)[:, :, OW - 1], eu[:, :, OW - 1], err_msg=tag + " last column")
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# float32 kernels (FSEQ)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", ["dilated_grouped", "input_dilation", "1d_dilated_stride",
                                  "explicit_dilated_grouped"])
def test_generic_float_kernels(dev, oracle, name, bits):
  """The float32 fake-quantised kernel on real-valued float32 (mixed magnitudes: another chain order
  gives other bits, tests/test_generic_block_cpu.py), uint8 and bit-packed input against the
  oracle's `fseq` mode, as blocks and as the connection alone.  None of these geometries is one the
  f32-MFMA connection kernel serves (asserted), so the connection runs on the direct-form kernel."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  c = _case(oracle, name, bits)
  g = c["g"]
  geom = _geom(oracle, g)
  okw = gc.oracle_kwargs(g)
  fw = _packed_kernel(c["leaf"], bits, dev).float_weight()
  assert fw.wtype == L.W_F32
  np.testing.assert_array_equal(_np(fw.w), c["qw"].w_fq)
  three_d = len(g.spatial) == 3
  if not three_d:
    assert not ops.fseq_gemm_supported(geom)      # snnqp_conv_forward keeps these off fseq_gemm.hip
  for fmt, x in (("f32", c["xr"]), ("u8", c["x"]), ("bits", c["x"])):
    xf = x.astype(F32)
    eu, es = oracle.conv_block(xf, c["qw"], c["bn"], None, "fseq", u0=c["u0"], **okw)
    for packed_out in (True, False):
      u, s = _block(oracle, c, dev, x, fw, fmt=fmt, packed_out=packed_out)
      _check(u, s, eu, es, packed_out, "block %s packed %s" % (fmt, packed_out))
    # the connection alone, the T * B images as the batch
    nb = x.shape[0] * x.shape[1]
    ey = oracle.quant_conv(xf.reshape((nb,) + x.shape[2:]), c["qw"], mode="fseq", **okw)
    xk = _as_h1(g, x, 2)
    xin = _t((xk.astype(F32) if fmt == "f32" else xk).reshape((nb,) + xk.shape[2:]), dev)
    if fmt == "bits":
      xin = ops.pack_bits(xin)
    y = _np(ops.conv3d_lif_forward(xin, geom, fw) if three_d else ops.conv_forward(xin, geom, fw))
    np.testing.assert_array_equal(y.reshape(ey.shape), ey, err_msg="connection " + fmt)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# neuron and BatchNorm forms
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("kind", ["plif", "lif", "mslif_tau3", "mslif_vreset", "bn_mul_only"])
def test_generic_block_neuron_forms(dev, oracle, kind, bits):
  """dilated_grouped with the other neurons -- PLIF, per-channel LIF (the decay vector indexed by the
  output channel across the groups), multi_step_LIF with tau 3 and with v_reset 0.1 -- and BatchNorm
  declared multiply-only (BN_MEAN_ZERO | BN_BIAS_ZERO)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  c = _case(oracle, "dilated_grouped", bits)
  g = c["g"]
  rng = np.random.Generator(np.random.PCG64(gc.seed_of(kind, bits)))
  bn_d, bn = c["bn"], None
  if kind == "plif":
    tp = F32(-0.35)
    nrn = ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, float(oracle.sigmoid_f32(tp)), 1.0, 0.0)
    ncfg = {"kind": "parametric_leaky_IF", "tau_param": tp}
  elif kind == "lif":
    tv = rng.uniform(-1, 2, g.cout).astype(F32)
    nrn = ops.Neuron(L.NEURON_LIF, 1.0, 1.0, 0.0, decay=_t(oracle.sigmoid_f32(tv), dev))
    ncfg = {"kind": "LIF", "tau_vec": tv}
  elif kind == "mslif_tau3":
    nrn, ncfg = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 3.0, 1.0, 0.0), {"kind": "multi_step_LIF", "tau": 3.0}
  elif kind == "mslif_vreset":
    nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.1)
    ncfg = {"kind": "multi_step_LIF", "tau": 2.0, "v_reset": 0.1}
  else:
    nrn, ncfg = _mslif(), None
    bn_d = dict(c["bn"], mean=np.zeros(g.cout, F32), bias=np.zeros(g.cout, F32))
    bn = _bn(oracle, bn_d, dev, L.BN_MEAN_ZERO | L.BN_BIAS_ZERO)
  eu, es = oracle.conv_block(c["x"], c["qw"], bn_d, ncfg, "int", u0=c["u0"], **gc.oracle_kwargs(g))
  assert 0 < es.mean() < 1
  w = _packed_kernel(c["leaf"], bits, dev).int_weight()
  for fmt in ("u8", "bits"):
    for packed_out in (True, False):
      u, s = _block(oracle, c, dev, c["x"], w, nrn=nrn, bn=bn, fmt=fmt, packed_out=packed_out)
      _check(u, s, eu, es, packed_out, "%s %s packed %s" % (kind, fmt, packed_out))
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# as the model reaches it
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", ["dilated_grouped", "same_kernel_dilation", "1d_same_k4",
                                  "explicit_dilated_grouped"])
def test_generic_block_through_the_spiking_block(dev, oracle, name, bits):
  """SpikingBlock(QuantConv(...), BatchNorm, neuron) with impl left at AUTO: the module resolves the
  geometry itself (SAME with a kernel dilation as the reference does), the library hands the block
  to the direct-form kernel and counts it (the 3-D entry has no other kernel and counts nothing),
  and the result is the oracle's, for uint8 and bit-packed input."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops, synthetic as syn
  from snnquantprune_amd.flax_qconv import QuantConv
  from snnquantprune_amd.spiking_learning import SpikingBlock
  c = _case(oracle, name, bits)
  g = c["g"]
  eu, es = c["int"]
  cfg = syn.make_config(bits=bits, prune_percentage=dict(gc.CODES)[bits])
  conv = QuantConv(g.cout, tuple(g.kernel), use_bias=False, config=cfg.quant, bits=bits, g_scale=cfg.quant.g_scale,
                   **gc.conv_kwargs(g))
  assert conv.out_shape(c["x"].shape[1:]) == es.shape[1:]
  blk = SpikingBlock(connection_fn=conv, neural_dynamics=cfg.neuron_dynamics(dtype=torch.float32),
                     norm_fn=nn.BatchNorm(use_running_average=True, momentum=0.9, epsilon=1e-5), return_state=True)
  bn = c["bn"]
  variables = nn.tree_from_numpy({"params": {"connection_fn": c["leaf"],
                                             "norm_fn": {"scale": bn["scale"], "bias": bn["bias"]}},
                                  "batch_stats": {"norm_fn": {"mean": bn["mean"], "var": bn["var"]}}}, dev)
  for fmt in ("u8", "bits"):
    xin = _t(c["x"], dev)
    if fmt == "bits":
      xin = ops.pack_bits(xin)
    ops.fallback_counts(reset=True)
    u, sp = blk.apply(variables, _t(c["u0"], dev), xin)
    counts = ops.fallback_counts()
    if len(g.spatial) != 3:
      assert counts["conv_blocks"] >= 1 and counts["last_reason"].startswith("conv: "), counts
    assert isinstance(sp, ops.PackedSpikes)
    np.testing.assert_array_equal(_np(sp), packbits_lastaxis(es), err_msg=fmt)
    np.testing.assert_array_equal(_np(u), eu, err_msg=fmt)
  ops.fallback_counts(reset=True)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# the grid-stride walk
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cout", [288, 257])
def test_generic_block_walks_beyond_one_grid(dev, oracle, cout):
  """B = 4, 64x64, a 1x1 kernel on 3 channels: 4 * 64 * 64 * Cout threads -- 4 718 592 (Cout 288,
  ballot words) and 4 210 688 (Cout 257, atomicOr) -- against the 16384 workgroups x 256 threads =
  4 194 304 of one grid, so the second trip of the grid-stride loop runs.  Whole raster and u_T."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops, synthetic as syn
  from tests.helpers import qweight_of
  T, B, HW, cin = 2, 4, 64, 3
  assert B * HW * HW * cout > 16384 * 256
  seed = gc.seed_of("grid_stride", cout)
  leaf = syn.quant_leaf((1, 1, cin, cout), gc.GAIN, seed, True, 0.3)
  bp, bs = syn.bn_leaf(cout, True, seed + 1)
  bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
  rng = np.random.Generator(np.random.PCG64(seed + 2))
  x = (rng.random((T, B, HW, HW, cin)) < 0.5).astype(np.uint8)
  u0 = (0.3 * rng.standard_normal((B, HW, HW, cout))).astype(F32)
  qw = qweight_of(oracle, leaf, 8)
  eu, es = oracle.conv_block(x, qw, bn, None, "int", padding="VALID", u0=u0)
  assert 0.03 < es.mean() < 0.5 and es[-1, -1, -1].max() == 1       # the tail of the walk spikes too
  w = _packed_kernel(leaf, 8, dev).int_weight()
  geom = ops.ConvGeom(HW, HW, cin, cout, 1, 1)
  u, s = ops.conv_lif_forward(_t(x, dev), geom, w, _mslif(), bn=_bn(oracle, bn, dev), u0=_t(u0, dev),
                              packed_out=True, impl=L.IMPL_GENERIC)
  np.testing.assert_array_equal(_np(s), packbits_lastaxis(es))
  np.testing.assert_array_equal(_np(u), eu)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# the predicated float32 launch behind an integer one
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("bits", BITS)
def test_generic_block_predicated_launch(dev, oracle, bits):
  """k5_stride2_valid (ragged Cout: the raster is assembled with atomicOr into zeroed words) on
  integer-valued float32 input: narrowed to uint8 by the checked pass, whose word stays 0, so the
  float32 launch behind the integer one -- and the zeroing in front of it -- must do nothing: raster
  and u_T are the integer launch's, bit for bit, although the kernel standing by holds other
  weights.  With the word set the same call leaves the float32 kernel's result (`fseq`)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  c = _case(oracle, "k5_stride2_valid", bits)
  g = c["g"]
  geom = _geom(oracle, g)
  eu, es = c["int"]
  pk = _packed_kernel(c["leaf"], bits, dev)
  w, fw = pk.int_weight(), pk.float_weight()
  other = ops.Weight(L.W_F32, (-fw.w).contiguous())
  xf = _t(c["x"].astype(F32), dev)
  x8, pred = ops.narrow_f32_async(xf)
  assert int(pred.item()) == 0
  np.testing.assert_array_equal(_np(x8), c["x"])
  bn = _bn(oracle, c["bn"], dev)
  for packed_out in (True, False):
    u, s = ops.conv_lif_forward(x8, geom, w, _mslif(), bn=bn, u0=_t(c["u0"], dev), packed_out=packed_out,
                                impl=L.IMPL_GENERIC, fallback=ops.FloatFallback(other, x=xf, pred=pred))
    _check(_np(u), _np(s), eu, es, packed_out, "not taken, packed %s" % packed_out)
  # taken: one value is not an integer
  xr = c["x"].astype(F32)
  xr[1, 1, 6, 8, 2] = 0.375
  xf = _t(xr, dev)
  x8, pred = ops.narrow_f32_async(xf)
  assert int(pred.item()) != 0
  fu, fs = oracle.conv_block(xr, c["qw"], c["bn"], None, "fseq", u0=c["u0"], **gc.oracle_kwargs(g))
  for packed_out in (True, False):
    u, s = ops.conv_lif_forward(x8, geom, w, _mslif(), bn=bn, u0=_t(c["u0"], dev), packed_out=packed_out,
                                impl=L.IMPL_GENERIC, fallback=ops.FloatFallback(fw, x=xf, pred=pred))
    _check(_np(u), _np(s), fu, fs, packed_out, "taken, packed %s" % packed_out)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------


def test_generic_block_refusals_write_nothing(dev, oracle):
  """What the direct-form block refuses comes back as the library's error with the outputs as they
  were (sentinel words, ragged Cout and bit-packed spikes: the case whose raster is zeroed by a
  launch of its own in front of the kernel):
    * pool = 2 handed to the direct-form kernel by snnqp_conv_lif_forward (EUNSUPPORTED: the caller
      pools the raster afterwards), and on a 3-D block (the 3-D entry takes no pool; SpikingBlock
      refuses it);
    * pool = 2 without a neuron;
    * feature groups that do not divide Cin, or Cout;
    * int8 codes with float32 input: without x_flags at snnqp_conv_lif_forward, and at the
      predicated entry, which has no integer kernel for float32 input."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops, synthetic as syn
  from snnquantprune_amd.flax_qconv import QuantConv
  from snnquantprune_amd.spiking_learning import SpikingBlock
  import dataclasses
  c = _case(oracle, "k5_stride2_valid", 4)
  g = c["g"]
  geom = _geom(oracle, g)
  OH, OW = g.out
  pk = _packed_kernel(c["leaf"], 4, dev)
  w, fw = pk.int_weight(), pk.float_weight()
  bn, nrn = _bn(oracle, c["bn"], dev), _mslif()
  x8 = _t(c["x"], dev)
  xf = _t(c["x"].astype(F32), dev)
  u0 = _t(c["u0"], dev)
  one = torch.ones(1, dtype=torch.int32, device=dev)
  SENT = 0x5A5A5A5A

  def outputs(g=g):
    return (torch.full((g.B,) + tuple(g.out) + (g.cout,), SENT, dtype=torch.int32, device=dev),
            torch.full((gc.T, g.B) + tuple(g.out) + ((g.cout + 31) // 32,), SENT, dtype=torch.int32, device=dev))

  def untouched(u, s, tag):
    assert bool((u == SENT).all()) and bool((s == SENT).all()), tag

  def conv_lif(x, in_type, gm, wt, pool, u, s, x_flags=None, g=g, bn=bn, u0=u0):
    gs, ws, ns, bs = gm.struct(), wt.struct(), nrn.struct(), bn.struct()
    unit = gm.H * gm.W * g.cin
    return L.lib().snnqp_conv_lif_forward(
        ops._ptr(x), in_type, g.B * unit, unit, gc.T, g.B, ctypes.byref(gs), ctypes.byref(ws), None,
        ctypes.byref(bs), ctypes.byref(ns), ops._ptr(u0), ops._ptr(u), ops._ptr(s), L.BITS, pool, L.IMPL_GENERIC,
        1, None, ops._ptr(x_flags), ops._stream())

  # pool = 2 with the direct-form kernel at the unpredicated entry
  u, s = outputs()
  assert conv_lif(x8, L.U8, geom, w, 2, u, s) == L.EUNSUPPORTED
  untouched(u, s, "pool = 2, impl = GENERIC")
  with pytest.raises(L.SnnqpError) as e:
    ops.conv_lif_forward(x8, geom, w, nrn, bn=bn, packed_out=True, pool=2, impl=L.IMPL_GENERIC)
  assert e.value.code == L.EUNSUPPORTED and "max-pool" in str(e.value)
  # ... and on a 3-D block
  c3 = _case(oracle, "explicit_dilated_grouped", 4)
  g3 = c3["g"]
  cfg = syn.make_config(bits=4, prune_percentage=0.5)
  blk = SpikingBlock(connection_fn=QuantConv(g3.cout, tuple(g3.kernel), use_bias=False, config=cfg.quant, bits=4,
                                             g_scale=cfg.quant.g_scale, **gc.conv_kwargs(g3)),
                     neural_dynamics=cfg.neuron_dynamics(dtype=torch.float32), pool=2)
  with pytest.raises(ValueError, match="2-D"):
    blk.apply(nn.tree_from_numpy({"params": {"connection_fn": c3["leaf"]}}, dev), None, _t(c3["x"], dev))
  # pool = 2 without a neuron
  none = ops.Neuron(L.NEURON_NONE)
  for wt, x, in_type in ((w, x8, L.U8), (fw, xf, L.F32)):
    u, s = outputs()
    assert _conv_lif_if(one, x, in_type, gc.T, g.B, geom, wt, bn, none, u0, u, s, L.BITS, 2) == L.EINVAL
    untouched(u, s, "pool = 2, no neuron")
  # groups that divide neither Cin = 48 nor Cout = 66 (5), Cin alone (4), Cout alone (11)
  c2 = _case(oracle, "dilated_grouped", 4)
  g2 = c2["g"]
  geom2 = _geom(oracle, g2)
  w2 = _packed_kernel(c2["leaf"], 4, dev).int_weight()
  bn2 = _bn(oracle, c2["bn"], dev)
  x2, u02 = _t(c2["x"], dev), _t(c2["u0"], dev)
  for groups in (5, 4, 11):
    assert (g2.cin % groups, g2.cout % groups) != (0, 0)
    bad = dataclasses.replace(geom2, groups=groups)
    u, s = outputs(g2)
    assert conv_lif(x2, L.U8, bad, w2, 1, u, s, g=g2, bn=bn2, u0=u02) == L.EINVAL
    assert "feature_group_count" in _last_error()
    untouched(u, s, "groups %d" % groups)
    u, s = outputs(g2)
    assert _conv_lif_if(one, x2, L.U8, gc.T, g2.B, bad, w2, bn2, nrn, u02, u, s, L.BITS, 1) == L.EINVAL
    untouched(u, s, "groups %d, predicated" % groups)
    y = torch.full((gc.T * g2.B,) + tuple(g2.out) + (g2.cout,), SENT, dtype=torch.int32, device=dev)
    bs, ws = bad.struct(), w2.struct()
    assert L.lib().snnqp_conv_forward(ops._ptr(x2), L.U8, gc.T * g2.B, ctypes.byref(bs), ctypes.byref(ws),
                                      ops._ptr(y), None, ops._stream()) == L.EINVAL
    assert bool((y == SENT).all())
  # int8 codes with float32 input
  with pytest.raises(ValueError, match="FloatFallback"):
    ops.conv_lif_forward(xf, geom, w, nrn, bn=bn, packed_out=True, impl=L.IMPL_GENERIC)
  u, s = outputs()
  assert conv_lif(xf, L.F32, geom, w, 1, u, s) == L.EINVAL
  untouched(u, s, "float32 into codes, no x_flags")
  u, s = outputs()
  flags = torch.zeros(1, dtype=torch.int32, device=dev)
  assert conv_lif(xf, L.F32, geom, w, 1, u, s, x_flags=flags) == L.EUNSUPPORTED
  untouched(u, s, "float32 into codes, impl = GENERIC")
  u, s = outputs()
  assert _conv_lif_if(one, xf, L.F32, gc.T, g.B, geom, w, bn, nrn, u0, u, s, L.BITS, 1) == L.EUNSUPPORTED
  assert "integer-typed input" in _last_error()
  untouched(u, s, "float32 into codes, predicated")
  y = torch.full((gc.T * g.B, OH, OW, g.cout), SENT, dtype=torch.int32, device=dev)
  gs, ws = geom.struct(), w.struct()
  assert L.lib().snnqp_conv_forward(ops._ptr(xf), L.F32, gc.T * g.B, ctypes.byref(gs), ctypes.byref(ws),
                                    ops._ptr(y), None, ops._stream()) == L.EUNSUPPORTED
  assert bool((y == SENT).all())
  # the same outputs take the block once the call is one the kernel serves
  u, s = outputs()
  L.check(conv_lif(x8, L.U8, geom, w, 1, u, s))
  np.testing.assert_array_equal(_np(s).view(np.uint32), packbits_lastaxis(c["int"][1]))
  np.testing.assert_array_equal(_np(u).view(F32), c["int"][0])
  assert ops.device_status() == 0
