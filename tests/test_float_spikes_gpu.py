"""GPU suite: float32 spike output (SpikingBlock(packed=False), the reference's own output format)
through every dispatch branch of the fused block, against the oracle.

Every case runs the block twice on the same variables and inputs, with packed=False and with
packed=True, and asserts: the float32 raster has exactly the reference's shape and is bit-equal to
the oracle's (so holds +0.0 / 1.0 only); u_T is bit-equal to the oracle's carry, the edge neurons of
odd pooled images included; the bit-packed result unpacks to the float32 one; nothing was reported
into the device status word.  Integer-valued input is checked against the `int` contract, input
with a non-integer against `fseq`.  With packed=False the quantised conv and dense blocks run on the
direct-form kernel, so the shapes stay small.

Section I lowers the byte budget of the blocks that walk the batch in slices, so that the code
behind more than one slice runs: sliced and whole must agree bit for bit, and with the oracle.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import cases
from tests.helpers import qweight_of

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()                      # fails loudly if the HIP extension is missing
  return torch.device("cuda:0")


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(x):
  return x.cpu().numpy()


def _conv_block(bits, N, pool, packed, ks=(3, 3), padding=((1, 1), (1, 1)), bn=True, batch_major=False, **kw):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import synthetic as syn
  from snnquantprune_amd.flax_qconv import QuantConv
  from snnquantprune_amd.spiking_learning import SpikingBlock
  cfg = syn.make_config(bits=bits, prune_percentage=0.9)
  return SpikingBlock(connection_fn=QuantConv(features=N, kernel_size=ks, padding=padding, use_bias=False,
                                              config=cfg.quant, bits=bits, g_scale=cfg.quant.g_scale, **kw),
                      neural_dynamics=cfg.neuron_dynamics(dtype=torch.float32),
                      norm_fn=nn.BatchNorm(use_running_average=True, momentum=0.9, epsilon=1e-5) if bn else None,
                      pool=pool, return_state=True, packed=packed, batch_major_input=batch_major)


def _dense_block(bits, N, packed, use_bias=False, batch_major=False):
  from snnquantprune_amd import synthetic as syn
  from snnquantprune_amd.flax_qdense import QuantDense
  from snnquantprune_amd.spiking_learning import SpikingBlock
  cfg = syn.make_config(bits=bits, prune_percentage=0.5)
  return SpikingBlock(connection_fn=QuantDense(N, use_bias=use_bias, config=cfg.quant, bits=bits,
                                               g_scale=cfg.quant.g_scale),
                      neural_dynamics=cfg.neuron_dynamics(dtype=torch.float32), return_state=True, packed=packed,
                      batch_major_input=batch_major)


def _conv_vars(leaf, bn, dev):
  from snnquantprune_amd import linen as nn
  if bn is None:
    return nn.tree_from_numpy({"params": {"connection_fn": leaf}}, dev)
  return nn.tree_from_numpy({"params": {"connection_fn": leaf, "norm_fn": {"scale": bn["scale"], "bias": bn["bias"]}},
                             "batch_stats": {"norm_fn": {"mean": bn["mean"], "var": bn["var"]}}}, dev)


def _check(got_f32, got_packed, eu, es, tag):
  """got_*: (u_T, spikes) of the packed=False / packed=True runs; eu, es: the oracle's carry and
  raster (pooled already where the block pools)."""
  from snnquantprune_amd import ops
  uf, sf = got_f32
  up, sp = got_packed
  es = np.asarray(es, F32)
  assert isinstance(sf, torch.Tensor) and sf.dtype == torch.float32, (tag, type(sf))
  assert tuple(sf.shape) == es.shape, (tag, tuple(sf.shape), es.shape)
  # bit patterns: +0.0 / 1.0 exactly as the oracle's Heaviside writes them (no -0.0, no NaN)
  np.testing.assert_array_equal(_np(sf).view(np.uint32), es.view(np.uint32), err_msg=tag + " float32 spikes")
  np.testing.assert_array_equal(_np(uf), eu, err_msg=tag + " u_T (packed=False)")
  assert isinstance(sp, ops.PackedSpikes), (tag, type(sp))
  assert tuple(sp.shape) == es.shape, (tag, sp.shape, es.shape)
  np.testing.assert_array_equal(_np(sp.to_dense()).view(np.uint32), _np(sf).view(np.uint32),
                                err_msg=tag + " packed vs float32 spikes")
  np.testing.assert_array_equal(_np(up), eu, err_msg=tag + " u_T (packed=True)")


def _pooled(oracle, es, pool):
  return oracle.max_pool_2x2(es) if pool == 2 else es


# ---------------------------------------------------------------------------
# A. the 2-channel event layer
# ---------------------------------------------------------------------------

EV_T, EV_B = 5, 3
FRAME_KINDS = ["u8_binary", "u8_counts", "f32_binary", "f32_half", "ev1", "ev4"]


@lru_cache(maxsize=None)
def _event_frames(hw):
  rng = np.random.Generator(np.random.PCG64(300 + hw))
  shape = (EV_T, EV_B, hw, hw, 2)
  binary = (rng.random(shape) < 0.1).astype(np.uint8)
  binary[:, :, hw - 1, hw - 1, :] = 1                        # the last pixel (an edge patch) fires
  counts = np.minimum(rng.poisson(0.4, shape), 9).astype(np.uint8)
  counts15 = counts.copy()
  counts15[1, 2, hw // 2, 3, 0] = 15                         # the largest count EV4 holds
  counts[EV_T - 1, EV_B - 1, hw - 1, hw - 2, 1] = 255        # a hot pixel
  return binary, counts, counts15


def _event_host(kind, hw):
  """(float32 frames as the oracle sees them, oracle mode) of a frame kind."""
  binary, counts, counts15 = _event_frames(hw)
  if kind in ("u8_binary", "ev1"):
    return binary.astype(F32), "int"
  if kind == "u8_counts":
    return counts.astype(F32), "int"
  if kind == "ev4":
    return counts15.astype(F32), "int"
  x = binary.astype(F32)
  if kind == "f32_half":
    x[2, 1, hw // 2, hw - 1, 1] = 0.5
    return x, "fseq"
  assert kind == "f32_binary"
  x[(binary == 0) & (np.arange(binary.size).reshape(binary.shape) % 7 == 0)] = -0.0
  assert np.signbit(x).any()
  return x, "int"


def _event_input(kind, hw, dev):
  """The frames of a kind on the device, in the kind's own format."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  binary, counts, counts15 = _event_frames(hw)
  if kind == "ev1":
    return ops.pack_frames(_t(binary, dev), L.EV1)
  if kind == "ev4":
    return ops.pack_frames(_t(counts15, dev), L.EV4)
  if kind.startswith("u8"):
    return _t(binary if kind == "u8_binary" else counts, dev)
  return _t(_event_host(kind, hw)[0], dev)


@lru_cache(maxsize=None)
def _event_case():
  return cases.conv_block_case(T=EV_T, B=EV_B, hw=8, cin=2, seed=961, gain=4.0)


@lru_cache(maxsize=None)
def _event_expected(kind, hw):
  from oracle import snn_oracle as oracle
  c = _event_case()
  xf, mode = _event_host(kind, hw)
  return oracle.conv_block(xf, qweight_of(oracle, c["leaf"], c["bits"]), c["bn"], None, mode)


def _hint_after_counts(dev, hw):
  """Make the device's count hint report counts (a packed=True event layer on count frames)."""
  from snnquantprune_amd import ops
  c = _event_case()
  _, counts, _ = _event_frames(hw)
  blk = _conv_block(c["bits"], 128, 1, True)
  blk.apply(_conv_vars(c["leaf"], c["bn"], dev), None, _t(counts, dev))
  torch.cuda.synchronize()
  hint = ops.count_hint(dev)
  hint.current()
  assert not hint.binary_so_far()


@pytest.mark.parametrize("hw", [16, 13], ids=["hw16", "hw13_odd"])
@pytest.mark.parametrize("pool", [1, 2], ids=["pool1", "pool2"])
@pytest.mark.parametrize("kind", FRAME_KINDS)
def test_event_layer_float32_spikes(dev, oracle, kind, pool, hw):
  """The first layer of every model (Cin 2, 3x3 SAME, Cout 128) with packed=False, on every frame
  format, with the count hint fresh ("binary so far": the state in which the layer speculates on
  bit-packed frames) and again after a batch of count frames."""
  from snnquantprune_amd import ops
  c = _event_case()
  variables = _conv_vars(c["leaf"], c["bn"], dev)
  eu, es = _event_expected(kind, hw)
  assert es.shape == (EV_T, EV_B, hw, hw, 128) and 0.005 < es.mean() < 0.5
  assert np.abs(eu[:, hw - 1]).max() > 0                     # the edge row is alive
  x = _event_input(kind, hw, dev)
  try:
    for hint in ("fresh", "after_counts"):
      ops._count_hints.clear()
      if hint == "after_counts":
        _hint_after_counts(dev, hw)
      else:
        assert ops.count_hint(dev).binary_so_far()
      got_f = _conv_block(c["bits"], 128, pool, False).apply(variables, None, x)
      got_p = _conv_block(c["bits"], 128, pool, True).apply(variables, None, x)
      _check(got_f, got_p, eu, _pooled(oracle, es, pool), "%s pool %d hw %d hint %s" % (kind, pool, hw, hint))
  finally:
    ops._count_hints.clear()
  assert ops.device_status() == 0


@pytest.mark.parametrize("kind", ["u8_binary", "u8_counts", "f32_binary", "f32_half"])
def test_event_layer_float32_spikes_batch_major_and_carried_state(dev, oracle, kind):
  """The event layer with packed=False on [B, T, ...] frames (batch_major_input, the model's input
  layout) and with a carried-in state, pool 2 on an odd image, count hint fresh."""
  from snnquantprune_amd import ops
  hw = 13
  c = _event_case()
  qw = qweight_of(oracle, c["leaf"], c["bits"])
  variables = _conv_vars(c["leaf"], c["bn"], dev)
  x = _event_input(kind, hw, dev)
  xf, mode = _event_host(kind, hw)
  rng = np.random.Generator(np.random.PCG64(17))
  u0 = (rng.random((EV_B, hw, hw, 128)) * 0.8).astype(F32)
  try:
    eu, es = _event_expected(kind, hw)
    xb = x.transpose(0, 1).contiguous()
    ops._count_hints.clear()
    got_f = _conv_block(c["bits"], 128, 2, False, batch_major=True).apply(variables, None, xb)
    got_p = _conv_block(c["bits"], 128, 2, True, batch_major=True).apply(variables, None, xb)
    _check(got_f, got_p, eu, oracle.max_pool_2x2(es), kind + " batch-major")
    eu, es = oracle.conv_block(xf, qw, c["bn"], None, mode, u0=u0)
    ops._count_hints.clear()
    got_f = _conv_block(c["bits"], 128, 2, False).apply(variables, _t(u0, dev), x)
    got_p = _conv_block(c["bits"], 128, 2, True).apply(variables, _t(u0, dev), x)
    _check(got_f, got_p, eu, oracle.max_pool_2x2(es), kind + " carried u0")
  finally:
    ops._count_hints.clear()
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# B. bit-input conv blocks
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cin,cout,hw,pool", [(128, 128, 8, 2), (128, 100, 8, 1), (64, 128, 8, 1),
                                              (64, 100, 7, 2), (48, 128, 8, 2), (48, 100, 8, 1)],
                         ids=["c128_o128_pool", "c128_o100", "c64_o128", "c64_o100_odd_pool", "c48_o128_pool",
                              "c48_o100"])
def test_bit_input_conv_float32_spikes(dev, oracle, cin, cout, hw, pool):
  """A 3x3 conv block on spikes with packed=False: the input as PackedSpikes, and as float32 {0, 1}
  (narrowed to bits by the checked pass); one float32 input with a 0.5 (the float32 kernel behind)."""
  from snnquantprune_amd import ops
  c = cases.conv_block_case(T=3, B=2, hw=hw, cin=cin, cout=cout, seed=1000 + cin + cout)
  qw = qweight_of(oracle, c["leaf"], c["bits"])
  variables = _conv_vars(c["leaf"], c["bn"], dev)
  xf = c["x"].astype(F32)
  half = xf.copy()
  half[1, 1, hw // 2, hw - 1, cin - 1] = 0.5
  for name, x, xo, mode in (("packed", ops.pack_bits(_t(c["x"], dev)), xf, "int"),
                            ("f32", _t(xf, dev), xf, "int"), ("f32_half", _t(half, dev), half, "fseq")):
    eu, es = oracle.conv_block(xo, qw, c["bn"], None, mode)
    assert 0.005 < es.mean() < 0.5
    got_f = _conv_block(c["bits"], cout, pool, False).apply(variables, None, x)
    got_p = _conv_block(c["bits"], cout, pool, True).apply(variables, None, x)
    _check(got_f, got_p, eu, _pooled(oracle, es, pool), "%s cin %d cout %d" % (name, cin, cout))
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# C. dense blocks
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("K,N", [(2048, 512), (208, 70)], ids=["wide_2048_512", "narrow_208_70"])
def test_dense_float32_spikes(dev, oracle, K, N):
  """A quantised dense block with packed=False on bit-packed spikes, uint8 counts, float32 rows
  (integer-valued and with a 7.5), and with a carried-in state."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  d = cases.dense_block_case(T=5, B=4, K=K, N=N, bits=8, p=0.5, counts=True)
  sp = cases.dense_block_case(T=5, B=4, K=K, N=N, bits=8, p=0.5, counts=False)
  qd = qweight_of(oracle, d["leaf"], 8)
  variables = nn.tree_from_numpy({"params": {"connection_fn": d["leaf"]}}, dev)
  counts = d["x"]
  assert counts.max() > 1
  cf = counts.astype(F32)
  frac = cf.copy()
  frac[3, 2, K // 3] = 7.5
  runs = (("packed", ops.pack_bits(_t(sp["x"], dev)), sp["x"].astype(F32), "int", None),
          ("u8_counts", _t(counts, dev), cf, "int", None),
          ("f32_counts", _t(cf, dev), cf, "int", None),
          ("f32_7.5", _t(frac, dev), frac, "fseq", None),
          ("u8_counts_u0", _t(counts, dev), cf, "int", d["u0"]))
  for name, x, xo, mode, u0 in runs:
    eu, es = oracle.dense_block(xo, qd, None, mode, u0=u0)
    assert 0.005 < es.mean() < 0.5
    carry = None if u0 is None else _t(u0, dev)
    got_f = _dense_block(8, N, False).apply(variables, carry, x)
    got_p = _dense_block(8, N, True).apply(variables, carry, x)
    _check(got_f, got_p, eu, es, "%s K %d N %d" % (name, K, N))
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# D. gated (TCJA) blocks
# ---------------------------------------------------------------------------


def test_gated_blocks_float32_spikes(dev, oracle):
  """GatedSpikes into a Cin-128 3x3 conv block (pool 1 and 2) and into a gated dense block, with
  packed=False, against gated_conv_block / gated_dense_block."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops, synthetic as syn
  T, B, H, W, C, N = 3, 2, 8, 8, 128, 128
  leaf = syn.quant_leaf((3, 3, C, N), 5.0, 971, True, 0.9)
  bp, bs = syn.bn_leaf(N, True, 972)
  bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
  qw = qweight_of(oracle, leaf, 4)
  rng = np.random.Generator(np.random.PCG64(3))
  s = (rng.random((T, B, H, W, C)) < 0.2).astype(np.uint8)
  gate = (1.0 / (1.0 + np.exp(-rng.standard_normal((T, B, C)) * 1.5))).astype(F32)
  x = ops.GatedSpikes(ops.pack_bits(_t(s, dev)), _t(gate, dev))
  eu, es = oracle.gated_conv_block(s.astype(F32), gate, qw, bn)
  assert 0.005 < es.mean() < 0.5
  variables = _conv_vars(leaf, bn, dev)
  for pool in (1, 2):
    got_f = _conv_block(4, N, pool, False).apply(variables, None, x)
    got_p = _conv_block(4, N, pool, True).apply(variables, None, x)
    _check(got_f, got_p, eu, _pooled(oracle, es, pool), "gated conv pool %d" % pool)
  # the dense block behind the second gate: channel-major flattening of gate x raster
  T, B, H, W, C, N = 3, 5, 4, 4, 128, 512
  leaf = syn.quant_leaf((C * H * W, N), 5.0, 981, True, 0.9)
  qw = qweight_of(oracle, leaf, 4)
  s = (rng.random((T, B, H, W, C)) < 0.3).astype(np.uint8)
  gate = (1.0 / (1.0 + np.exp(-rng.standard_normal((T, B, C)) * 1.5))).astype(F32)
  x = ops.GatedSpikes(ops.pack_bits(_t(s, dev)), _t(gate, dev)).flattened()
  eu, es = oracle.gated_dense_block(s.astype(F32), gate, qw)
  assert 0.005 < es.mean() < 0.5
  variables = nn.tree_from_numpy({"params": {"connection_fn": leaf}}, dev)
  got_f = _dense_block(4, N, False).apply(variables, None, x)
  got_p = _dense_block(4, N, True).apply(variables, None, x)
  _check(got_f, got_p, eu, es, "gated dense")
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# E. 3-D conv blocks
# ---------------------------------------------------------------------------


def test_conv3d_block_float32_spikes(dev, oracle):
  """A 3-D QuantConv block (3x3x3, stride (2, 1, 2), SAME; BatchNorm; u0 carried) with
  packed=False on float32 input, integer-valued and with a 1.5."""
  from snnquantprune_amd import ops, synthetic as syn
  T, B, D, H, W, C, N, ks = 4, 3, 5, 6, 7, 4, 40, (3, 3, 3)
  leaf = syn.quant_leaf(ks + (C, N), 5.0, 77, True, 0.9)
  qw = qweight_of(oracle, leaf, 4)
  bp, bs = syn.bn_leaf(N, True, 78)
  bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
  variables = _conv_vars(leaf, bn, dev)
  rng = np.random.Generator(np.random.PCG64(79))
  xs = rng.integers(0, 2, size=(T, B, D, H, W, C)).astype(F32)
  half = xs.copy()
  half[2, 1, 0, 1, 1, 0] = 1.5
  ckw = dict(padding="SAME", strides=(2, 1, 2))
  u0 = None
  for name, xin, mode in (("int", xs, "int"), ("fseq", half, "fseq")):
    if u0 is None:
      eu0, _ = oracle.conv_block(xs[:1], qw, bn, None, "int", **ckw)
      u0 = (rng.standard_normal(eu0.shape) * 0.3).astype(F32)
    eu, es = oracle.conv_block(xin, qw, bn, None, mode, u0=u0, **ckw)
    assert 0.005 < es.mean() < 0.7
    got_f = _conv_block(4, N, 1, False, ks=ks, padding="SAME", strides=(2, 1, 2)).apply(
        variables, _t(u0, dev), _t(xin, dev))
    got_p = _conv_block(4, N, 1, True, ks=ks, padding="SAME", strides=(2, 1, 2)).apply(
        variables, _t(u0, dev), _t(xin, dev))
    _check(got_f, got_p, eu, es, "conv3d " + name)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# F. unquantised weights: the float32 kernel (f32 MFMA + neuron scan)
# ---------------------------------------------------------------------------


def test_float_block_float32_spikes(dev, oracle, monkeypatch):
  """An unquantised conv block (DuQ a = -1: float32 kernels) with packed=False and pool 2 on an
  odd image: the f32-MFMA connection and the neuron scan (SpikingBlock._float_block), on uint8
  spikes and on real-valued float32 input."""
  from snnquantprune_amd import ops, synthetic as syn
  from snnquantprune_amd import spiking_learning as sl
  T, B, hw, C, N = 3, 2, 9, 32, 64
  leaf = syn.quant_leaf((3, 3, C, N), 5.0, 991, False, 0.5)
  qw = qweight_of(oracle, leaf, 4, quantized=False)
  bp, bs = syn.bn_leaf(N, True, 992)
  bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
  variables = _conv_vars(leaf, bn, dev)
  rng = np.random.Generator(np.random.PCG64(993))
  spikes = (rng.random((T, B, hw, hw, C)) < 0.2).astype(np.uint8)
  real = ((rng.random((T, B, hw, hw, C)) < 0.3) * rng.random((T, B, hw, hw, C)) * 2).astype(F32)
  taken = []
  old = sl.SpikingBlock._float_block

  def spy(self, *a, **k):
    taken.append(self.packed)
    return old(self, *a, **k)
  monkeypatch.setattr(sl.SpikingBlock, "_float_block", spy)
  for name, x, xo in (("u8 spikes", _t(spikes, dev), spikes.astype(F32)), ("f32 real", _t(real, dev), real)):
    eu, es = oracle.conv_block(xo, qw, bn, None, "fseq")
    assert 0.005 < es.mean() < 0.5 and np.abs(eu[:, hw - 1]).max() > 0
    got_f = _conv_block(4, N, 2, False).apply(variables, None, x)
    got_p = _conv_block(4, N, 2, True).apply(variables, None, x)
    _check(got_f, got_p, eu, oracle.max_pool_2x2(es), "float block " + name)
  assert taken == [False, True, False, True]
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# G. composed blocks (a connection with a bias)
# ---------------------------------------------------------------------------


def test_composed_block_float32_spikes(dev, oracle):
  """SpikingBlock(QuantDense(use_bias=True)) composes the stand-alone ops (SpikingBlock._composed);
  packed=None gives float32 spikes there, as in the reference.  Against the oracle's scan of
  quant_dense + bias -> multi_step_LIF."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  K, N = 208, 70
  d = cases.dense_block_case(T=5, B=4, K=K, N=N, bits=8, p=0.5, counts=False)
  qd = qweight_of(oracle, d["leaf"], 8)
  bias = (np.random.Generator(np.random.PCG64(5)).standard_normal(N) * 0.3).astype(F32)
  variables = nn.tree_from_numpy({"params": {"connection_fn": dict(d["leaf"], bias=bias)}}, dev)
  neuron = lambda u, v: oracle.multi_step_lif(u, v, 2.0)
  for name, x in (("u8", _t(d["x"], dev)), ("f32", _t(d["x"].astype(F32), dev))):
    eu, es = oracle.spiking_block(None, d["x"].astype(F32), lambda v: oracle.quant_dense(v, qd, "int") + bias, neuron)
    assert 0.005 < es.mean() < 0.5
    got_f = _dense_block(8, N, None, use_bias=True).apply(variables, None, x)
    got_p = _dense_block(8, N, True, use_bias=True).apply(variables, None, x)
    _check(got_f, got_p, eu, es, "composed " + name)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# H. empty batch, zero steps
# ---------------------------------------------------------------------------


def test_empty_batch_and_zero_steps_float32_spikes(dev, oracle):
  """B = 0 and T = 0 with packed=False: empty float32 rasters of the reference's shape, and over zero
  steps u_T is the carry (spiking_learning.py:446-462: a scan over no steps returns its carry -- u0,
  or the zeros of initialize_carry)."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  c = _event_case()
  ev_vars = _conv_vars(c["leaf"], c["bn"], dev)
  b = cases.conv_block_case(T=3, B=2, hw=8)
  b_vars = _conv_vars(b["leaf"], b["bn"], dev)
  d = cases.dense_block_case(T=5, B=4, K=208, N=70, bits=8, p=0.5)
  d_vars = nn.tree_from_numpy({"params": {"connection_fn": d["leaf"]}}, dev)
  rng = np.random.Generator(np.random.PCG64(6))
  try:
    for T, B in ((0, 2), (3, 0), (0, 0)):
      for pool in (1, 2):
        ops._count_hints.clear()
        shapes = ((T, B, 8, 8, 2), (T, B, 8, 8, 128))
        for (blk_vars, bits), shape in zip(((ev_vars, c["bits"]), (b_vars, b["bits"])), shapes):
          for x in (torch.zeros(shape, dtype=torch.uint8, device=dev), torch.zeros(shape, device=dev)):
            for u0 in (None, (rng.random((B, 8, 8, 128)) * 0.5).astype(F32)):
              # (a freed block of the state's size holds NaN: a state nothing writes is caught)
              del_me = torch.full((B, 8, 8, 128), float("nan"), device=dev)
              del del_me
              u, s = _conv_block(bits, 128, pool, False).apply(blk_vars, None if u0 is None else _t(u0, dev), x)
              assert s.dtype == torch.float32 and tuple(s.shape) == (T, B, 8 // pool, 8 // pool, 128)
              assert tuple(u.shape) == (B, 8, 8, 128)
              if T == 0:
                np.testing.assert_array_equal(_np(u), np.zeros((B, 8, 8, 128), F32) if u0 is None else u0)
      for x in (torch.zeros((T, B, 208), dtype=torch.uint8, device=dev), torch.zeros((T, B, 208), device=dev)):
        for u0 in (None, (rng.random((B, 70)) * 0.5).astype(F32)):
          del_me = torch.full((B, 70), float("nan"), device=dev)
          del del_me
          u, s = _dense_block(8, 70, False).apply(d_vars, None if u0 is None else _t(u0, dev), x)
          assert s.dtype == torch.float32 and tuple(s.shape) == (T, B, 70) and tuple(u.shape) == (B, 70)
          if T == 0:
            np.testing.assert_array_equal(_np(u), np.zeros((B, 70), F32) if u0 is None else u0)
  finally:
    ops._count_hints.clear()
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# the ABI underneath
# ---------------------------------------------------------------------------


def test_conv_lif_forward_float32_spikes_at_the_abi(dev, oracle):
  """ops.conv_lif_forward on event frames with packed_out=False: uint8 frames with binary_first=True
  (the speculation does not apply to float32 spikes) equal the oracle, one direct-form launch; packed
  event frames are refused with EUNSUPPORTED before they count as a fallback."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops, packing
  from snnquantprune_amd.quant import QuantDesc
  hw = 13
  c = _event_case()
  qw = qweight_of(oracle, c["leaf"], c["bits"])
  leaf, bits = c["leaf"], c["bits"]
  a, cc = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  pk = packing.PackedKernel(_t(leaf["kernel"], dev), QuantDesc(L.Q_DUQ, bits, a, cc, float(2 ** (bits - 1) - 1), cc),
                            _t(leaf["prune_0"]["mask"], dev))
  w = pk.int_weight_mfma(128)
  mul = (F32(1) / np.sqrt(c["bn"]["var"] + F32(1e-5))) * c["bn"]["scale"]
  bn = ops.BnCoeffs(_t(c["bn"]["mean"], dev), _t(mul.astype(F32), dev), _t(c["bn"]["bias"], dev))
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  g = ops.ConvGeom(hw, hw, 2, 128, 3, 3, (1, 1), ((1, 1), (1, 1)))
  binary, _, counts15 = _event_frames(hw)
  for name, x in (("binary", binary), ("counts", counts15)):
    eu, es = oracle.conv_block(x.astype(F32), qw, c["bn"], None, "int")
    before = ops.fallback_counts()["conv_blocks"]
    u, s = ops.conv_lif_forward(_t(x, dev), g, w, nrn, bn=bn, want_u=True, packed_out=False, pool=1,
                                x_max=1, binary_first=True)
    assert s.dtype == torch.float32 and tuple(s.shape) == es.shape
    np.testing.assert_array_equal(_np(s).view(np.uint32), es.view(np.uint32), err_msg=name)
    np.testing.assert_array_equal(_np(u), eu, err_msg=name)
    assert ops.fallback_counts()["conv_blocks"] == before + 1, name
  for fmt, x in ((L.EV1, binary), (L.EV4, counts15)):
    pf = ops.pack_frames(_t(x, dev), fmt)
    for packed_out, impl in ((False, L.IMPL_AUTO), (True, L.IMPL_GENERIC)):
      before = ops.fallback_counts()
      with pytest.raises(L.SnnqpError) as e:
        ops.conv_lif_forward(pf, g, w, nrn, bn=bn, want_u=True, packed_out=packed_out, pool=1, impl=impl, x_max=1)
      assert e.value.code == L.EUNSUPPORTED and "unpack" in str(e.value), str(e.value)
      after = ops.fallback_counts()
      assert after["conv_blocks"] == before["conv_blocks"], (fmt, packed_out)
  assert ops.device_status() == 0


# ---------------------------------------------------------------------------
# I. the batch walked in slices (spiking_learning.CURRENTS_SLICE_BYTES)
# ---------------------------------------------------------------------------
# Blocks that keep a slice's float32 currents between the connection and the neuron scan walk the
# batch under a byte budget; at the product value more than one slice needs over 1 GiB of currents.
# Lowered here so that B = 5 walks as 2 + 2 + 1: the carried state sliced on axis 0, the batch-major
# input sliced and transposed, potentials joined on axis 0 and rasters on axis 1.

SL_T, SL_B, SL_C, SL_N = 3, 5, 32, 64
SLICE_KINDS = ["f32_real", "u8_counts", "packed"]


@lru_cache(maxsize=None)
def _slice_conv_case(hw):
  """An unquantised 3x3 conv block: (leaf, bn, u0, {kind: host input [T, B, hw, hw, C]})."""
  from snnquantprune_amd import synthetic as syn
  leaf = syn.quant_leaf((3, 3, SL_C, SL_N), 5.0, 1991 + hw, False, 0.5)
  bp, bs = syn.bn_leaf(SL_N, True, 1992 + hw)
  bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
  rng = np.random.Generator(np.random.PCG64(1993 + hw))
  shape = (SL_T, SL_B, hw, hw, SL_C)
  xs = {"f32_real": ((rng.random(shape) < 0.3) * rng.random(shape) * 2).astype(F32),
        "u8_counts": np.minimum(rng.poisson(0.15, shape), 255).astype(np.uint8),
        "packed": (rng.random(shape) < 0.2).astype(np.uint8)}
  assert xs["u8_counts"].max() > 1
  u0 = (rng.standard_normal((SL_B, hw, hw, SL_N)) * 0.4).astype(F32)
  return leaf, bn, u0, xs


@lru_cache(maxsize=None)
def _slice_conv_expected(hw, kind):
  from oracle import snn_oracle as oracle
  leaf, bn, u0, xs = _slice_conv_case(hw)
  qw = qweight_of(oracle, leaf, 4, quantized=False)
  return oracle.conv_block(xs[kind].astype(F32), qw, bn, None, "fseq", u0=u0)


@lru_cache(maxsize=None)
def _slice_dense_case():
  """An unquantised dense block, K = 200 -> N = 70: (leaf, u0, {kind: host input [T, B, K]})."""
  from snnquantprune_amd import synthetic as syn
  K, N = 200, 70
  leaf = syn.quant_leaf((K, N), 4.0, 2991, False, 0.5)
  rng = np.random.Generator(np.random.PCG64(2993))
  shape = (SL_T, SL_B, K)
  xs = {"f32_real": ((rng.random(shape) < 0.3) * rng.random(shape) * 2).astype(F32),
        "u8_counts": np.minimum(rng.poisson(0.15, shape), 255).astype(np.uint8),
        "packed": (rng.random(shape) < 0.2).astype(np.uint8)}
  u0 = (rng.standard_normal((SL_B, N)) * 0.4).astype(F32)
  return leaf, u0, xs


@lru_cache(maxsize=None)
def _slice_dense_expected(kind):
  from oracle import snn_oracle as oracle
  leaf, u0, xs = _slice_dense_case()
  return oracle.dense_block(xs[kind].astype(F32), qweight_of(oracle, leaf, 4, quantized=False), None, "fseq", u0=u0)


@lru_cache(maxsize=None)
def _slice_gated_case():
  """A quantised Cin-32 3x3 conv block behind a gate: (leaf, bn, u0, spikes, gate, (u_T, raster))."""
  from oracle import snn_oracle as oracle
  from snnquantprune_amd import synthetic as syn
  H = W = 8
  leaf = syn.quant_leaf((3, 3, SL_C, 128), 12.0, 3971, True, 0.9)      # (32 gated inputs: rate 0.12)
  bp, bs = syn.bn_leaf(128, True, 3972)
  bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
  rng = np.random.Generator(np.random.PCG64(3973))
  s = (rng.random((SL_T, SL_B, H, W, SL_C)) < 0.2).astype(np.uint8)
  gate = (1.0 / (1.0 + np.exp(-rng.standard_normal((SL_T, SL_B, SL_C)) * 1.5))).astype(F32)
  u0 = (rng.standard_normal((SL_B, H, W, 128)) * 0.4).astype(F32)
  exp = oracle.gated_conv_block(s.astype(F32), gate, qweight_of(oracle, leaf, 4), bn, u0=u0)
  return leaf, bn, u0, s, gate, exp


def _slice_input(kind, x, batch_major, dev):
  from snnquantprune_amd import ops
  if batch_major:
    x = np.swapaxes(x, 0, 1)
  t = _t(x, dev)
  return ops.pack_bits(t) if kind == "packed" else t


def _walk(monkeypatch, name, blocks, variables, u0, x, per_sample, T, eu, es, tag, dev):
  """Runs each block of `blocks` (packed=False, packed=True) in one slice and with the budget at
  2.5 samples, counts the launches of ops.<name>, and checks both runs against each other bit for
  bit and against the oracle."""
  from snnquantprune_amd import ops
  from snnquantprune_amd import spiking_learning as sl
  assert sl.CURRENTS_SLICE_BYTES == 1 << 30
  launches = []
  real = getattr(ops, name)

  def spy(xi, *a, **k):
    # (images of the launch: [T, nb, ...] behind a gate, T * nb rows else)
    launches.append(int(xi.spikes.shape[1]) if isinstance(xi, ops.GatedSpikes) else int(xi.shape[0]) // T)
    return real(xi, *a, **k)
  monkeypatch.setattr(ops, name, spy)
  got = {}
  for budget, want in ((1 << 30, [SL_B]), (2 * per_sample + per_sample // 2, [2, 2, 1])):
    monkeypatch.setattr(sl, "CURRENTS_SLICE_BYTES", budget)
    for blk in blocks:
      del launches[:]
      got[budget, blk.packed] = blk.apply(variables, _t(u0, dev), x)
      assert launches == want, (tag, budget, launches)
  monkeypatch.setattr(sl, "CURRENTS_SLICE_BYTES", 1 << 30)
  monkeypatch.setattr(ops, name, real)
  for packed in (False, True):
    (u1, s1), (u3, s3) = got[1 << 30, packed], got[2 * per_sample + per_sample // 2, packed]
    assert tuple(u3.shape) == tuple(u1.shape) and u3.is_contiguous()
    np.testing.assert_array_equal(_np(u3).view(np.uint32), _np(u1).view(np.uint32), err_msg=tag + " u_T sliced vs whole")
    b1, b3 = (s1.bits, s3.bits) if packed else (s1, s3)
    assert tuple(s3.shape) == tuple(s1.shape) and b3.is_contiguous()
    np.testing.assert_array_equal(_np(b3), _np(b1), err_msg=tag + " raster sliced vs whole")
  sliced = 2 * per_sample + per_sample // 2
  _check(got[sliced, False], got[sliced, True], eu, es, tag + " sliced")
  _check(got[1 << 30, False], got[1 << 30, True], eu, es, tag + " whole")


@pytest.mark.parametrize("batch_major", [False, True], ids=["time_major", "batch_major"])
@pytest.mark.parametrize("kind", SLICE_KINDS)
@pytest.mark.parametrize("hw,pool", [(9, 1), (8, 2)], ids=["hw9_pool1", "hw8_pool2"])
def test_float_conv_block_walks_the_batch_in_slices(dev, oracle, monkeypatch, hw, pool, kind, batch_major):
  from snnquantprune_amd import ops
  leaf, bn, u0, xs = _slice_conv_case(hw)
  eu, es = _slice_conv_expected(hw, kind)
  assert 0.01 < es.mean() < 0.6 and np.abs(eu).max() > 0
  x = _slice_input(kind, xs[kind], batch_major, dev)
  blocks = [_conv_block(4, SL_N, pool, p, batch_major=batch_major) for p in (False, True)]
  _walk(monkeypatch, "conv_forward", blocks, _conv_vars(leaf, bn, dev), u0, x, 4 * SL_T * hw * hw * SL_N, SL_T,
        eu, _pooled(oracle, es, pool), "conv %s hw %d pool %d %s" % (kind, hw, pool, "BM" if batch_major else "TM"), dev)
  assert ops.device_status() == 0


@pytest.mark.parametrize("batch_major", [False, True], ids=["time_major", "batch_major"])
@pytest.mark.parametrize("kind", SLICE_KINDS)
def test_float_dense_block_walks_the_batch_in_slices(dev, oracle, monkeypatch, kind, batch_major):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  leaf, u0, xs = _slice_dense_case()
  eu, es = _slice_dense_expected(kind)
  assert 0.01 < es.mean() < 0.6
  x = _slice_input(kind, xs[kind], batch_major, dev)
  blocks = [_dense_block(4, 70, p, batch_major=batch_major) for p in (False, True)]
  variables = nn.tree_from_numpy({"params": {"connection_fn": leaf}}, dev)
  _walk(monkeypatch, "conv_forward", blocks, variables, u0, x, 4 * SL_T * 70, SL_T, eu, es,
        "dense %s %s" % (kind, "BM" if batch_major else "TM"), dev)
  assert ops.device_status() == 0


@pytest.mark.parametrize("pool", [1, 2], ids=["pool1", "pool2"])
def test_gated_conv_block_walks_the_batch_in_slices(dev, oracle, monkeypatch, pool):
  from snnquantprune_amd import ops
  leaf, bn, u0, s, gate, (eu, es) = _slice_gated_case()
  assert 0.01 < es.mean() < 0.6
  x = ops.GatedSpikes(ops.pack_bits(_t(s, dev)), _t(gate, dev))
  blocks = [_conv_block(4, 128, pool, p) for p in (False, True)]
  _walk(monkeypatch, "conv_gated_forward", blocks, _conv_vars(leaf, bn, dev), u0, x, 4 * SL_T * 8 * 8 * 128, SL_T,
        eu, _pooled(oracle, es, pool), "gated conv pool %d" % pool, dev)
  assert ops.device_status() == 0
