"""The 16-channel K walk of the bit-input 3x3 conv kernel: a last 32-channel
group whose upper half holds no input channel is walked in (tap, 16-channel) units.  Conv blocks on
bit-packed spikes against the oracle, rasters bit-exact, around every boundary of the walk, fp6 and
int8 codes, pooled and not, table and arithmetic dequantisation, random BatchNorm, and the same
bits as the walk over whole groups on the same build (nn.set_conv_k16(False)); the C3 model with
channel compaction; and a launch whose dropped half-word and tile rows hold garbage."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import cases
from tests.helpers import packbits_lastaxis, qweight_of

pytestmark = pytest.mark.gpu
F32 = np.float32
T, B, COUT = 5, 2, 64
H, W = 9, 14


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()
  return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _k16_default():
  from snnquantprune_amd import linen as nn
  assert nn.conv_k16()              # the default
  yield
  nn.set_conv_k16(True)
  nn.set_channel_compaction(True)


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(x):
  from snnquantprune_amd import ops
  if isinstance(x, ops.PackedSpikes):
    return x.bits.cpu().numpy().view(np.uint32)
  return x.cpu().numpy()


def _weight(leaf, bits, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  desc = QuantDesc(L.Q_DUQ, bits, a, c, float(2 ** (bits - 1) - 1), c)
  pk = packing.PackedKernel(_t(leaf["kernel"], dev), desc, _t(leaf["prune_0"]["mask"], dev))
  return pk.int_weight_mfma(COUT)


def _random_bn(cout, seed, dev):
  from snnquantprune_amd import ops
  rng = np.random.Generator(np.random.PCG64(seed))
  bn = dict(mean=rng.normal(0, 0.3, cout).astype(F32), var=rng.uniform(0.3, 2.0, cout).astype(F32),
            scale=rng.uniform(0.5, 1.5, cout).astype(F32), bias=rng.normal(0, 0.3, cout).astype(F32))
  mul = (F32(1) / np.sqrt(bn["var"] + F32(1e-5))) * bn["scale"]
  return bn, ops.BnCoeffs(_t(bn["mean"], dev), _t(mul.astype(F32), dev), _t(bn["bias"], dev), 0)


def _forms(w, bits):
  """(name, weight) per dequantisation form: the table (fp6 codes only) and the arithmetic one."""
  forms = [("table", w)] if bits == 4 else []
  forms.append(("arith", dataclasses.replace(w, abs_sum_max=0)))
  return forms


@pytest.mark.parametrize("bits", [4, 8], ids=["fp6", "int8"])
@pytest.mark.parametrize("cin", [1, 16, 17, 48, 65, 79, 80, 81, 112])
def test_conv_k16_bit_exact(dev, oracle, cin, bits):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  leaf = cases.conv_block_case(T=T, B=B, hw=8, cin=cin, cout=COUT, bits=bits, p=0.5,
                               seed=5301 + cin, gain=3.0)["leaf"]
  qw = qweight_of(oracle, leaf, bits)
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  w = _weight(leaf, bits, dev)
  assert (w.code_max <= 7) == (bits == 4)
  rng = np.random.Generator(np.random.PCG64(cin * 11 + bits))
  x = (rng.random((T, B, H, W, cin)) < 0.35).astype(np.uint8)
  xin = ops.pack_bits(_t(x, dev))
  geom = ops.ConvGeom(H, W, cin, COUT, 3, 3, (1, 1), ((1, 1), (1, 1)))
  bn, bnc = _random_bn(COUT, cin + 19 * bits, dev)
  eu, es = oracle.conv_block(x, qw, bn, None, "int")
  assert es.sum() > 0
  ops.fallback_counts(reset=True)
  for dq, wf in _forms(w, bits):
    assert ops.conv_dequant_form(wf, nrn) == dq
    outs = []
    for k16 in (True, False):
      nn.set_conv_k16(k16)
      what = "cin %d bits %d dq %s k16 %s" % (cin, bits, dq, k16)
      u, s = ops.conv_lif_forward(xin, geom, wf, nrn, bn=bnc, packed_out=True, impl=L.IMPL_MFMA)
      _, sp = ops.conv_lif_forward(xin, geom, wf, nrn, bn=bnc, packed_out=True, pool=2,
                                   impl=L.IMPL_MFMA, want_u=False)
      print(what, "raster bits differing from the oracle:",
            int((np.unpackbits((_np(s) ^ packbits_lastaxis(es)).view(np.uint8))).sum()))
      np.testing.assert_array_equal(_np(s), packbits_lastaxis(es), err_msg=what)
      np.testing.assert_array_equal(_np(u), eu, err_msg=what)
      np.testing.assert_array_equal(_np(sp), packbits_lastaxis(oracle.max_pool_2x2(es)), err_msg=what)
      outs.append((_np(s), _np(u), _np(sp)))
    for a, b in zip(outs[0], outs[1]):
      assert a.tobytes() == b.tobytes(), "cin %d bits %d dq %s: 16-walk != 32-walk" % (cin, bits, dq)
  fc = ops.fallback_counts()
  assert fc["conv_blocks"] == 0 and fc["dense_blocks"] == 0


@pytest.mark.parametrize("bits", [4, 8], ids=["fp6", "int8"])
def test_dropped_half_is_not_read(dev, oracle, bits):
  """Cin = 80 on tiles padded to 96: spikes in bits 16..31 of a pixel's third word and non-zero
  codes in the tile rows behind them must not reach the sums."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf96 = cases.conv_block_case(T=T, B=B, hw=8, cin=96, cout=COUT, bits=bits, p=0.5, seed=6107,
                                 gain=3.0)["leaf"]
  leaf80 = dict(leaf96, kernel=np.ascontiguousarray(leaf96["kernel"][:, :, :80]),
                prune_0=dict(leaf96["prune_0"], mask=np.ascontiguousarray(leaf96["prune_0"]["mask"][:, :, :80])))
  qw96, qw80 = qweight_of(oracle, leaf96, bits), qweight_of(oracle, leaf80, bits)
  w96 = _weight(leaf96, bits, dev)
  codes = w96.w.cpu().numpy().reshape(3, 3, 96, -1)
  assert np.abs(codes[:, :, 80:]).sum() > 0       # the rows behind the dropped half are not zero
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  rng = np.random.Generator(np.random.PCG64(99 + bits))
  x = (rng.random((T, B, H, W, 96)) < 0.35).astype(np.uint8)
  assert x[..., 80:].sum() > 0
  x96 = ops.pack_bits(_t(x, dev))
  x80 = ops.PackedSpikes(x96.bits, 80)            # the same words: three per pixel
  geom = ops.ConvGeom(H, W, 80, COUT, 3, 3, (1, 1), ((1, 1), (1, 1)))
  bn, bnc = _random_bn(COUT, 7 + bits, dev)
  eu, es = oracle.conv_block(x[..., :80], qw80, bn, None, "int")
  eu96, es96 = oracle.conv_block(x, qw96, bn, None, "int")
  assert (es != es96).any()                       # the dropped channels would have mattered
  for dq, wf in _forms(w96, bits):
    for pool in (1, 2):
      u, s = ops.conv_lif_forward(x80, geom, wf, nrn, bn=bnc, packed_out=True, pool=pool,
                                  impl=L.IMPL_MFMA, want_u=pool == 1)
      exp = es if pool == 1 else oracle.max_pool_2x2(es)
      np.testing.assert_array_equal(_np(s), packbits_lastaxis(exp), err_msg="%s pool %d" % (dq, pool))
      if pool == 1:
        np.testing.assert_array_equal(_np(u), eu, err_msg=dq)


def _apply(model, variables, x):
  from snnquantprune_amd import ops
  ops.profile_start()
  (logits, _), mut = model.apply(variables, x, trgt=None, train=False, rng=None,
                                 mutable=["intermediates"])
  ops.profile_stop()
  notes = dict(ops.PROFILE_NOTES)
  pools = [_np(mut["intermediates"]["pool%d" % i][0]) for i in range(3)]
  dense = mut["intermediates"]["dense_out"][0].to_dense().cpu().numpy().astype(np.uint8)
  return logits.cpu().numpy(), pools + [dense], notes


def test_c3_compacted_model(dev, oracle):
  """C3 at full geometry, compaction on: conv1 reads 80 of conv0's 96 computed channels.  Pooled
  rasters at 128 channels, read-out and logits equal to the oracle and to the 32-channel walk."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, synthetic as syn
  c = cases.conv_net_case(T=6, B=1, hw=128, p=0.9, layer_bits=[4, 4, 4, 4], out=100, random_bn=False,
                          gains=(4.0, 5.0, 4.0, 4.0))
  e = cases.conv_net_expected(oracle, c)
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  cfg.quant.layer_bits = [4, 4, 4, 4]
  model = models.ConvDenseSNN(num_classes=10, config=cfg)
  variables = nn.tree_from_numpy(c["vars"], dev)
  xin = ops.pack_frames(_t(c["x"], dev), L.EV1)
  ops.fallback_counts(reset=True)
  res = {}
  for k16 in (True, False):
    nn.set_conv_k16(k16)
    logits, pools, notes = _apply(model, variables, xin)
    cins = sorted(v["channels"]["cin"] for v in notes.values()
                  if isinstance(v, dict) and "channels" in v)
    assert 80 in cins, (cins, notes)              # conv1 is handed 80 input channels
    np.testing.assert_array_equal(logits, e["logits"], err_msg="k16 %s" % k16)
    for i in range(3):
      np.testing.assert_array_equal(pools[i], e["pool%d_bits" % i], err_msg="k16 %s pool%d" % (k16, i))
    np.testing.assert_array_equal(pools[3], e["dense_s"], err_msg="k16 %s read-out" % k16)
    res[k16] = (logits, pools)
  assert res[True][0].tobytes() == res[False][0].tobytes()
  for a, b in zip(res[True][1], res[False][1]):
    assert a.tobytes() == b.tobytes()
  fc = ops.fallback_counts()
  assert fc["conv_blocks"] == 0 and fc["dense_blocks"] == 0
  status = ops.device_status() if hasattr(ops, "device_status") else 0
  assert not status, status
