"""K packing of the bit-input 3x3 conv kernel: the codes padded along Cin to the
next multiple of 32 and the kernel walking (tap, 32-channel group) pairs.  One to four groups,
fp6 and int8 instructions, both dequantisation forms of the fp6 kernel, per-channel and uniform
BatchNorm, a carried-in state, odd image sizes: rasters, pooled rasters and u_T bit-exact against
the oracle, and the same bits as the 64 / 128-channel layout (nn.set_conv_kpack(False))."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import cases
from tests.helpers import packbits_lastaxis, qweight_of

pytestmark = pytest.mark.gpu
F32 = np.float32
T, B, COUT = 5, 2, 64
GEOMS = [(9, 14, True), (7, 11, False)]      # H, W, pooled too


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()
  return torch.device("cuda:0")


@pytest.fixture
def kpack_restored():
  from snnquantprune_amd import linen as nn
  yield
  nn.set_conv_kpack(True)


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(x):
  from snnquantprune_amd import ops
  if isinstance(x, ops.PackedSpikes):
    return x.bits.cpu().numpy().view(np.uint32)
  return x.cpu().numpy()


def _weight(leaf, bits, dev, kpack):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  desc = QuantDesc(L.Q_DUQ, bits, a, c, float(2 ** (bits - 1) - 1), c)
  nn.set_conv_kpack(kpack)
  pk = packing.PackedKernel(_t(leaf["kernel"], dev), desc, _t(leaf["prune_0"]["mask"], dev))
  return pk.int_weight_mfma(COUT)


def _bn_forms(cout, seed):
  """(name, oracle bn dict, library flags): per-channel random statistics, and the fold the
  shipped models get (mean = bias = 0, one multiplier for every channel)."""
  from snnquantprune_amd import _lib as L
  rng = np.random.Generator(np.random.PCG64(seed))
  rnd = dict(mean=rng.normal(0, 0.3, cout).astype(F32), var=rng.uniform(0.3, 2.0, cout).astype(F32),
             scale=rng.uniform(0.5, 1.5, cout).astype(F32), bias=rng.normal(0, 0.3, cout).astype(F32))
  uni = dict(mean=np.zeros(cout, F32), var=np.full(cout, 0.7, F32), scale=np.full(cout, 1.3, F32),
             bias=np.zeros(cout, F32))
  return [("random", rnd, 0), ("uniform", uni, L.BN_MEAN_ZERO | L.BN_BIAS_ZERO | L.BN_MUL_UNIFORM)]


def _bn(bn, flags, dev):
  from snnquantprune_amd import ops
  mul = (F32(1) / np.sqrt(bn["var"] + F32(1e-5))) * bn["scale"]
  return ops.BnCoeffs(_t(bn["mean"], dev), _t(mul.astype(F32), dev), _t(bn["bias"], dev), flags)


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("cin", [1, 31, 32, 33, 64, 79, 96, 97, 127, 128])
def test_conv_kpack_bit_exact(dev, oracle, kpack_restored, cin, bits):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops, packing
  leaf = cases.conv_block_case(T=T, B=B, hw=8, cin=cin, cout=COUT, bits=bits, p=0.5,
                               seed=4201 + cin, gain=3.0)["leaf"]
  qw = qweight_of(oracle, leaf, bits)
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  w_on = _weight(leaf, bits, dev, True)
  w_off = _weight(leaf, bits, dev, False)
  assert w_on.wt.shape[1] == 9 * packing.conv_cin_pad(cin) // 32
  if cin <= 2:
    assert w_off.wt is None          # the 64 / 128 layout never tiled 1 or 2 input channels
  else:
    assert w_off.wt.shape[1] == 9 * packing.conv_cin_pad(cin, False) // 32
  assert (w_on.code_max <= 7) == (bits == 4)
  ws = [w_on] if cin <= 2 else [w_on, w_off]
  forms = [("table", ws)] if bits == 4 else []
  forms.append(("arith", [dataclasses.replace(w, abs_sum_max=0) for w in ws]))
  rng = np.random.Generator(np.random.PCG64(cin * 7 + bits))
  fired = 0
  for H, W, pooled in GEOMS:
    x = (rng.random((T, B, H, W, cin)) < 0.35).astype(np.uint8)
    xin = ops.pack_bits(_t(x, dev))
    geom = ops.ConvGeom(H, W, cin, COUT, 3, 3, (1, 1), ((1, 1), (1, 1)))
    u0 = rng.uniform(-0.5, 0.9, (B, H, W, COUT)).astype(F32)
    for bn_name, bn, flags in _bn_forms(COUT, cin + 17 * bits):
      bnc = _bn(bn, flags, dev)
      for carry in (None, u0):
        eu, es = oracle.conv_block(x, qw, bn, None, "int", u0=carry)
        fired += int(es.sum())
        u0t = None if carry is None else _t(carry, dev)
        for dq, wlist in forms:
          assert ops.conv_dequant_form(wlist[0], nrn) == dq
          what = "cin %d bits %d %dx%d bn %s u0 %s dq %s" % (cin, bits, H, W, bn_name, carry is not None, dq)
          outs = []
          for w in wlist:
            u, s = ops.conv_lif_forward(xin, geom, w, nrn, bn=bnc, u0=u0t, packed_out=True,
                                        impl=L.IMPL_MFMA)
            np.testing.assert_array_equal(_np(s), packbits_lastaxis(es), err_msg=what)
            np.testing.assert_array_equal(_np(u), eu, err_msg=what)
            outs.append((_np(s), _np(u)))
            if pooled:
              _, sp = ops.conv_lif_forward(xin, geom, w, nrn, bn=bnc, u0=u0t, packed_out=True, pool=2,
                                           impl=L.IMPL_MFMA, want_u=False)
              np.testing.assert_array_equal(_np(sp), packbits_lastaxis(oracle.max_pool_2x2(es)), err_msg=what)
          # the 64 / 128 layout gives the same bits, -0.0 and +0.0 in u_T included
          for s, u in outs[1:]:
            np.testing.assert_array_equal(outs[0][0], s, err_msg=what)
            assert outs[0][1].tobytes() == u.tobytes(), what
  assert fired > 0
