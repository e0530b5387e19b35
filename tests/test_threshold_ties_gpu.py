"""Every fused forward epilogue at exact threshold ties.

The cases of tests/tie_cases.py put membrane potentials EXACTLY on v_threshold (dyadic DuQ scale,
dyadic BatchNorm, power-of-two decays; tests/test_threshold_ties_cpu.py asserts that each case
holds such ties, and that a strict compare would change its raster).  Here each kernel path runs
them: packed raster and u_T equal the oracle's census bit for bit, so a compare site that used
`>`, reset another lane set, pooled a tie away or contracted the update into an FMA one ulp off
the threshold fails.  Each launch is bracketed by ops.fallback_counts() -- a silent drop to the
direct-form kernel fails the case -- and ends on a clear device status word."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import tie_cases as tc
from tests.helpers import packbits_lastaxis

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()                      # fails loudly if the HIP extension is missing
  return torch.device("cuda:0")


@pytest.fixture
def no_new_fallbacks():
  from snnquantprune_amd import ops
  before = ops.fallback_counts()
  yield
  after = ops.fallback_counts()
  assert (after["conv_blocks"], after["dense_blocks"]) == (before["conv_blocks"], before["dense_blocks"]), after
  assert ops.device_status() == 0


@pytest.fixture
def conv_knobs_restored():
  from snnquantprune_amd import linen as nn
  yield
  nn.set_conv_kpack(True)
  nn.set_conv_k16(True)
  nn.set_channel_compaction(True)


def _ids(*paths):
  return [c["id"] for c in tc.CASES if c["path"] in paths]


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
  desc = None if a == -1.0 else QuantDesc(L.Q_DUQ, bits, a, c, float(2 ** (bits - 1) - 1), c)
  mask = leaf.get("prune_0", {}).get("mask")
  return packing.PackedKernel(_t(leaf["kernel"], dev), desc, None if mask is None else _t(mask, dev))


def _mfma_weight(leaf, bits, dev):
  n = leaf["kernel"].shape[-1]
  return _packed_kernel(leaf, bits, dev).int_weight_mfma((n + 31) // 32 * 32)


def _neuron(oracle, cfg, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  vth, vr = cfg["v_threshold"], cfg["v_reset"]
  if cfg["kind"] == "multi_step_LIF":
    return ops.Neuron(L.NEURON_MULTI_STEP_LIF, cfg["tau"], vth, vr)
  if cfg["kind"] == "parametric_leaky_IF":
    return ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, float(oracle.sigmoid_f32(cfg["tau_param"])), vth, vr)
  return ops.Neuron(L.NEURON_LIF, 1.0, vth, vr, decay=_t(oracle.sigmoid_f32(cfg["tau_vec"]), dev))


def _bn(oracle, b, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  bn = b["bn"]
  if bn is None:
    return None
  mean, mul, bias = oracle.bn_coeffs(bn["mean"], bn["var"], bn["scale"], bn["bias"], 1e-5)
  flags = 0
  for name in tc.bn_flags(b["case"]["bn"]):
    flags |= getattr(L, name)
  return ops.BnCoeffs(_t(mean, dev), _t(mul, dev), _t(bias, dev), flags)


def _check(got_u, got_s, r, what, pooled=False):
  np.testing.assert_array_equal(_np(got_s), packbits_lastaxis(r["pooled"] if pooled else r["s"]), err_msg=what)
  if got_u is not None:
    np.testing.assert_array_equal(_np(got_u), r["u"], err_msg=what)


# ---------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("id", _ids("dense"))
def test_dense_kernels_at_ties(dev, oracle, no_new_fallbacks, id):
  """dense_mfma.hip (bit and uint8 rows, and fp6-sized codes with the fp6 tiles withheld),
  dense_fp6.hip (4-bit, 2-bit with L = 1, the true division, K split over workgroups),
  dense_wide.hip (uint8, bit and float32 rows; the general walk: every case with u_T returned,
  a carried-in state ON the threshold, tau 4 / v_th 0.75 / v_reset 0.25, decay 0.5 and 1, tau 3;
  the fast walk: the walk="fast" cases launched without u_T, with and without BatchNorm) and
  the direct-form kernel."""
  import ctypes
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  T, B, K, N = c["T"], c["B"], c["K"], c["N"]
  pk = _packed_kernel(b["leaf"], c["bits"], dev)
  w = pk.int_weight_mfma((N + 31) // 32 * 32)
  kernel, rows = c["kernel"], c["rows"]
  if c.get("drop_fp6"):
    assert w.wt6 is not None and 0 < w.code_max <= 7       # it WOULD take the fp6 kernel
    w = dataclasses.replace(w, wt6=None)
  x = _t(b["x"], dev)
  xin = {"bits": lambda: ops.pack_bits(x), "u8": lambda: x, "f32": lambda: x.to(torch.float32)}[rows]()
  fb = ops.FloatFallback(pk.float_weight()) if rows == "f32" else None
  fp6_takes_it = rows == "bits" and w.wt6 is not None and 0 < w.code_max <= 7
  if kernel == "mfma":
    assert w.wt is not None and not fp6_takes_it and N <= 128
    impl = L.IMPL_MFMA
  elif kernel in ("fp6", "fp6_split"):
    assert fp6_takes_it
    ws = int(L.lib().snnqp_dense_workspace_bytes(L.BITS, T, B, K, N, ctypes.byref(w.struct())))
    assert (ws > 0) == (kernel == "fp6_split"), ws
    impl = L.IMPL_AUTO
  elif kernel == "wide":
    assert w.wt is not None and not fp6_takes_it and N > 128
    impl = L.IMPL_AUTO if rows == "f32" else L.IMPL_MFMA
  else:
    impl = L.IMPL_GENERIC
  u0 = None if b["u0"] is None else _t(b["u0"], dev)
  nrn, bn = _neuron(oracle, b["cfg"], dev), _bn(oracle, b, dev)
  # dense_wide.hip takes neuron_walk_fast only in a launch that neither carries a state in nor
  # returns u_T (its `straight`): the wide cases run both ways -- with u_T on the general walk
  # (`(u - v_th) >= 0`), without it on the fast one where the case allows it (`u >= v_th`)
  if c.get("walk") == "fast":
    assert u0 is None and nrn.v_reset == 0.0 and nrn.decay is None and ops.is_pow2(nrn.k)
  for want_u in (True, False) if kernel == "wide" else (True,):
    u, s = ops.dense_lif_forward(xin, w, K, N, nrn, bn=bn, u0=u0, want_u=want_u, packed_out=True,
                                 impl=impl, fallback=fb)
    assert (u is not None) == want_u
    _check(u, s, r, "%s want_u %s" % (id, want_u))


@pytest.mark.parametrize("id", _ids("head"))
def test_dense_head_at_ties(dev, oracle, no_new_fallbacks, id):
  """The one-launch head: both blocks tie (8-bit codes into 4-bit codes), both rasters and the
  logits equal the oracle's."""
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  w1 = _mfma_weight(b["leaf"], c["bits"], dev)
  w2 = _mfma_weight(b["leaf2"], c["bits2"], dev)
  x = _t(b["x"], dev)
  xin = ops.pack_bits(x) if c["rows"] == "bits" else x
  logits, s1, s2 = ops.dense_head_forward(xin, w1, c["K"], c["N"], _neuron(oracle, b["cfg"], dev), w2, c["N2"],
                                          _neuron(oracle, b["cfg2"], dev), group=10, want_s1=True, want_s2=True)
  _check(None, s1, r, id + " hidden")
  _check(None, s2, r["second"], id + " output")
  np.testing.assert_array_equal(_np(logits), r["logits"])


@pytest.mark.parametrize("id", _ids("gated_dense"))
def test_gated_dense_at_ties(dev, oracle, no_new_fallbacks, id):
  """dense_gated.hip (gates in {0.25, 0.5, 0.75, 1}: the fmaf chain over the channels is exact)
  and the neuron scan behind it, e2m3 codes (4-bit) and two e3m2 digits (6-bit)."""
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  pk = _packed_kernel(b["leaf"], c["bits"], dev)
  w = pk.int_weight()
  assert (w.code_max > 7) == (c["bits"] > 4)
  x = ops.GatedSpikes(ops.pack_bits(_t(b["x"], dev)), _t(b["gate"], dev)).flattened()
  y = ops.dense_gated_forward(x, w, pk.gated_dense_codes(c["C"], c["H"] * c["W"]))
  u, s = ops.lif_forward(y, _neuron(oracle, b["cfg"], dev), packed_out=True)
  _check(u, s, r, id)


@pytest.mark.parametrize("id", _ids("fseq_dense"))
def test_float_weights_at_ties(dev, oracle, no_new_fallbacks, id):
  """Unquantised float32 weights n / 16 on 0/1 rows through fseq_gemm.hip (the connection of a
  float block, spiking_learning.py _float_block) and the neuron scan: the sum is exact in any
  order, an integrate-and-fire neuron keeps the grid, and ties are frequent."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  T, B, K, N = c["T"], c["B"], c["K"], c["N"]
  w = _packed_kernel(b["leaf"], 8, dev).float_weight()
  assert w.wtype == L.W_F32
  geom = ops.ConvGeom(1, 1, K, N, 1, 1)
  assert ops.fseq_gemm_supported(geom)
  x = _t(b["x"].astype(F32), dev)
  y = ops.conv_forward(x.reshape(T * B, 1, 1, K), geom, w).reshape(T, B, N)
  u, s = ops.lif_forward(y, _neuron(oracle, b["cfg"], dev), packed_out=True)
  _check(u, s, r, id)
  # ... and as SpikingBlock selects that path itself: real-valued inputs by declaration
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import packing, synthetic as syn
  from snnquantprune_amd.flax_qdense import QuantDense
  from snnquantprune_amd.spiking_learning import LIF, SpikingBlock, atan
  cfg = syn.make_config(bits=8, prune_percentage=-1.0)
  blk = SpikingBlock(connection_fn=QuantDense(N, use_bias=False, config=cfg.quant, bits=8, g_scale=cfg.quant.g_scale),
                     neural_dynamics=LIF(init_tau=2.0, spike_fn=atan), return_state=True, packed=True)
  variables = nn.tree_from_numpy({"params": {"connection_fn": b["leaf"],
                                             "neural_dynamics": {"tau": b["cfg"]["tau_vec"]}}}, dev)
  with packing.integer_inputs(False):
    u, s = blk.apply(variables, None, x)
  _check(u, s, r, id + " through SpikingBlock")


# ---------------------------------------------------------------------------
# conv
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("id", _ids("conv_bits"))
def test_conv_bits_kernel_at_ties(dev, oracle, no_new_fallbacks, id):
  """conv3x3_bits.hip: Cin 32 / 64 / 128 into 40 / 128 channels on 8x8 and a clipped 5x11, with
  and without the 2x2 pool; the table, arithmetic and L = 1 dequantisation forms; no BatchNorm,
  the uniform fold, per-channel coefficients, negative multipliers; every neuron form; a
  carried-in state ON the threshold.  Each launch runs twice: as packed, and with the
  min_current_bits hint that lets the kernel fuse the membrane update where that is exact (a
  carried-in state must keep the fused form out whatever the hint says)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  w = _mfma_weight(b["leaf"], c["bits"], dev)
  nrn, bn = _neuron(oracle, b["cfg"], dev), _bn(oracle, b, dev)
  if "dq" in c:
    assert ops.conv_dequant_form(w, nrn) == c["dq"]
  geom = ops.ConvGeom(c["H"], c["W"], c["cin"], c["cout"], 3, 3, (1, 1), ((1, 1), (1, 1)))
  xin = ops.pack_bits(_t(b["x"], dev))
  u0 = None if b["u0"] is None else _t(b["u0"], dev)
  hinted = dataclasses.replace(w, min_current_bits=ops.current_min_bits(w, bn, int(w.abs_sum_max), c["cout"]))
  for ww, name in ((w, "plain"), (hinted, "hinted")):
    for pool in c["pools"]:
      u, s = ops.conv_lif_forward(xin, geom, ww, nrn, bn=bn, u0=u0, packed_out=True, pool=pool,
                                  impl=L.IMPL_MFMA, x_max=1)
      _check(u, s, r, "%s %s pool %d" % (id, name, pool), pooled=pool == 2)


@pytest.mark.parametrize("id", _ids("conv_knobs"))
def test_conv_bits_kernel_knobs_at_ties(dev, oracle, no_new_fallbacks, conv_knobs_restored, id):
  """One block (Cin 80: 96 or 128 padded channels, a 16-channel last group; 64 of its 128 output
  channels pruned dead) with K packing, the 16-channel half walk and channel compaction at their defaults, and with all
  three off: the same tie-laden rasters and potentials."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops, packing, synthetic as syn
  from snnquantprune_amd.flax_qconv import QuantConv
  from snnquantprune_amd.spiking_learning import SpikingBlock
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  H, W, cin, cout = c["H"], c["W"], c["cin"], c["cout"]
  nrn, bn = _neuron(oracle, b["cfg"], dev), _bn(oracle, b, dev)
  geom = ops.ConvGeom(H, W, cin, cout, 3, 3, (1, 1), ((1, 1), (1, 1)))
  x = _t(b["x"], dev)
  xin = ops.pack_bits(x)
  cfg = syn.make_config(bits=c["bits"], prune_percentage=c["prune"])
  variables = nn.tree_from_numpy(
      {"params": {"connection_fn": b["leaf"], "norm_fn": {"scale": b["bn"]["scale"], "bias": b["bn"]["bias"]}},
       "batch_stats": {"norm_fn": {"mean": b["bn"]["mean"], "var": b["bn"]["var"]}}}, dev)
  for on in (True, False):
    nn.set_conv_kpack(on)
    nn.set_conv_k16(on)
    nn.set_channel_compaction(on)
    w = _mfma_weight(b["leaf"], c["bits"], dev)
    assert w.wt.shape[1] == 9 * packing.conv_cin_pad(cin, on) // 32
    for pool in (1, 2):
      u, s = ops.conv_lif_forward(xin, geom, w, nrn, bn=bn, packed_out=True, pool=pool, impl=L.IMPL_MFMA, x_max=1)
      _check(u, s, r, "%s knobs %s pool %d" % (id, on, pool), pooled=pool == 2)
    blk = SpikingBlock(connection_fn=QuantConv(features=cout, kernel_size=(3, 3), padding=((1, 1), (1, 1)),
                                               use_bias=False, config=cfg.quant, bits=c["bits"],
                                               g_scale=cfg.quant.g_scale),
                       neural_dynamics=cfg.neuron_dynamics(dtype=torch.float32),
                       norm_fn=nn.BatchNorm(use_running_average=True, momentum=0.9, epsilon=1e-5),
                       pool=2, return_state=False, compact=True)
    _, sp = blk.apply(variables, None, xin)
    cm = getattr(sp, "chan_map", None)
    assert (cm is not None) == on, "compaction %s: channel map %r" % (on, cm)
    if on:
      assert cm.index.size < cout
    _check(None, ops.expand_channels(sp), r, "%s block, knobs %s" % (id, on), pooled=True)


@pytest.mark.parametrize("id", _ids("conv_u8c2"))
def test_event_layer_at_ties(dev, oracle, no_new_fallbacks, id):
  """conv3x3_u8c2.hip on 16x16 two-channel frames with per-channel BatchNorm: binary frames as
  uint8, bit-packed (EV1) and float32; count frames (values up to 3) as uint8, nibble-packed
  (EV4) and float32; pooled and not; with u_T returned and without (two instances of the
  kernel); multi_step_LIF with tau 2 and the true division."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  pk = _packed_kernel(b["leaf"], c["bits"], dev)
  w = pk.int_weight_mfma(c["cout"])
  assert w.ch_stack_max > 0 and w.ch_slots is not None and w.code_max <= 7
  nrn, bn = _neuron(oracle, b["cfg"], dev), _bn(oracle, b, dev)
  geom = ops.ConvGeom(c["H"], c["W"], 2, c["cout"], 3, 3, (1, 1), ((1, 1), (1, 1)))
  x = _t(b["x"], dev)
  x_max = int(b["x"].max())
  assert x_max == (1 if c["frames"] == "binary" else 3)
  frames = [("uint8", x, L.IMPL_MFMA, None),
            ("EV1" if x_max == 1 else "EV4", ops.pack_frames(x, L.EV1 if x_max == 1 else L.EV4), L.IMPL_MFMA, None),
            ("float32", x.to(torch.float32), L.IMPL_AUTO, ops.FloatFallback(pk.float_weight()))]
  # without u_T (how a model launches it: nothing carried in or out, T in one chunk) the launcher
  # takes the instance whose potentials live behind the staging code (template parameter ONE)
  for name, xin, impl, fb in frames:
    for pool in c["pools"]:
      for want_u in (True, False):
        u, s = ops.conv_lif_forward(xin, geom, w, nrn, bn=bn, want_u=want_u, packed_out=True, pool=pool,
                                    impl=impl, x_max=x_max, fallback=fb)
        assert (u is not None) == want_u
        _check(u, s, r, "%s %s pool %d want_u %s" % (id, name, pool, want_u), pooled=pool == 2)


@pytest.mark.parametrize("id", _ids("gated_conv"))
def test_gated_conv_at_ties(dev, oracle, no_new_fallbacks, id):
  """conv_gated.hip on a clipped 5x11 image with dyadic gates, then BatchNorm and the neuron
  scan: e2m3 codes (4-bit) and two e3m2 digits (6-bit)."""
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  pk = _packed_kernel(b["leaf"], c["bits"], dev)
  w = pk.int_weight()
  assert (w.code_max > 7) == (c["bits"] > 4)
  geom = ops.ConvGeom(c["H"], c["W"], c["cin"], c["cout"], 3, 3, (1, 1), ((1, 1), (1, 1)))
  x = ops.GatedSpikes(ops.pack_bits(_t(b["x"], dev)), _t(b["gate"], dev))
  y = ops.conv_gated_forward(x, geom, w, pk.gated_codes())
  u, s = ops.lif_forward(y, _neuron(oracle, b["cfg"], dev), bn=_bn(oracle, b, dev), packed_out=True)
  _check(u, s, r, id)


@pytest.mark.parametrize("id", _ids("conv_generic", "conv3d"))
def test_direct_form_kernel_at_ties(dev, oracle, no_new_fallbacks, id):
  """generic_block.hip: a strided 2-D geometry with asymmetric padding, and a 3-D one (SAME,
  strides 2 / 1 / 2) with LIF decays 0.5 and 1, on uint8 and bit-packed input."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  b, r = tc.build(id), tc.tie_census(oracle, id)
  c = b["case"]
  w = _packed_kernel(b["leaf"], c["bits"], dev).int_weight()
  nrn, bn = _neuron(oracle, b["cfg"], dev), _bn(oracle, b, dev)
  x = _t(b["x"], dev)
  ks, st = c["ksize"], c["strides"]
  for xin in (x, ops.pack_bits(x)):
    if c["path"] == "conv3d":
      sp = (c["D"], c["H"], c["W"])
      pads = oracle.resolve_padding(sp, ks, st, c["padding"])
      geom = ops.Conv3dGeom(*sp, c["cin"], c["cout"], *ks, stride=st, pad=pads)
      u, s = ops.conv3d_lif_forward(xin, geom, w, nrn, bn=bn, packed_out=True)
    else:
      geom = ops.ConvGeom(c["H"], c["W"], c["cin"], c["cout"], ks[0], ks[1], st, c["padding"])
      u, s = ops.conv_lif_forward(xin, geom, w, nrn, bn=bn, packed_out=True, impl=L.IMPL_GENERIC)
    assert tuple(u.shape) == r["u"].shape
    _check(u, s, r, id)
