"""The currents form of the bit-input MFMA conv (csrc/conv3x3_currents.hip) on the
GPU: currents and accumulators bit for bit against the direct-form kernel and the oracle on the
cases of tests/currents_cases.py, inside framed and misaligned buffers; then the two callers that
route through it, QuantConv on a spike raster and the training forward of ConvDenseSNN, with the
switch nn.set_train_conv_mfma on and off.  Bit-equal: assert_array_equal on the int32 view."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from tests import conv_train_reference as cr
from tests import currents_cases as cc
from tests.helpers import packbits_lastaxis

pytestmark = pytest.mark.gpu
F32 = np.float32
FRAME = 64                       # sentinel words on each side of a buffer
Y_SENTINEL = 0x7FC0BEEF          # a NaN pattern no current equals; as int32 no accumulator either


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()
  return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _switch_default():
  from snnquantprune_amd import linen as nn
  assert nn.train_conv_mfma()      # the default
  yield
  nn.set_train_conv_mfma(True)


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
  a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
  return np.ascontiguousarray(a).view(np.int32)


def _packed_kernel(leaf, bits, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  desc = QuantDesc(L.Q_DUQ, bits, a, c, float(2 ** (bits - 1) - 1), c)
  mask = leaf.get("prune_0", {}).get("mask")
  return packing.PackedKernel(_t(leaf["kernel"], dev), desc, None if mask is None else _t(mask, dev))


def _weight(c, dev):
  """ops.Weight with the MFMA tiles, from the project's DuQ quantiser; wt_cin: the codes padded
  wider than the packing rule, tiled with ops.pack_codes_mfma directly."""
  from snnquantprune_amd import ops
  e = cc.expected(c)
  n_pad = (c["cout"] + 31) // 32 * 32
  w = _packed_kernel(e["leaf"], cc.bits_of(c), dev).int_weight_mfma(n_pad)
  codes = w.w.reshape(3, 3, c["cin"], c["cout"])
  np.testing.assert_array_equal(codes.cpu().numpy(), e["qw"].q.astype(np.int8))   # the oracle's codes
  assert (0 < w.code_max <= 7) == cc.fp6(c)
  if c["wt_cin"]:
    padded = codes.new_zeros((3, 3, c["wt_cin"], c["cout"]))
    padded[:, :, :c["cin"]] = codes
    w = dataclasses.replace(w, wt=ops.pack_codes_mfma(padded.reshape(-1, c["cout"]), n_pad), wt_cin=c["wt_cin"])
  elif c["cin"] <= 128:
    assert w.wt is not None and w.wt_cin in (0, (c["cin"] + 31) // 32 * 32)
  return w


def _geom(c):
  from snnquantprune_amd import ops
  return ops.ConvGeom(c["H"], c["W"], c["cin"], c["cout"], 3, 3, (1, 1), cc.PADS)


def _framed(n, fill, dev):
  """(allocation, view of n int32 words one word off the allocation's alignment)."""
  buf = torch.full((n + 2 * FRAME + 1,), fill, dtype=torch.int32, device=dev)
  view = buf[FRAME + 1:FRAME + 1 + n]
  assert view.data_ptr() % 16 == 4 and view.is_contiguous()
  return buf, view


def _frame_intact(buf, n, fill):
  b = buf.cpu().numpy()
  return (b[:FRAME + 1] == fill).all() and (b[FRAME + 1 + n:] == fill).all()


def _run_ex(c, w, xwords, dev, impl, want_acc=True):
  """snnqp_conv_forward_ex on buffers framed by sentinels and one word off their allocations.
  -> (y bits int32, acc int32 | None), after checking the frames."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  g = _geom(c).struct()
  ws = w.struct()
  ones = np.int32(-1)
  xbuf, xv = _framed(xwords.size, int(ones), dev)
  xv.copy_(_t(xwords.reshape(-1).view(np.int32), dev))
  n = c["NB"] * c["H"] * c["W"] * c["cout"]
  sent = int(np.uint32(Y_SENTINEL).astype(np.int32))
  ybuf, yv = _framed(n, sent, dev)
  abuf, av = _framed(n, sent, dev) if want_acc else (None, None)
  L.check(L.lib().snnqp_conv_forward_ex(ops._ptr(xv), L.BITS, c["NB"], ctypes.byref(g), ctypes.byref(ws),
                                        ops._ptr(w.wt), ops._ptr(yv), ops._ptr(av), impl, ops._stream()))
  torch.cuda.synchronize()
  assert _frame_intact(ybuf, n, sent), "stray write around y"
  assert _frame_intact(xbuf, xwords.size, int(ones)), "the input's frame changed"
  shape = (c["NB"], c["H"], c["W"], c["cout"])
  acc = None
  if want_acc:
    assert _frame_intact(abuf, n, sent), "stray write around acc"
    acc = av.cpu().numpy().reshape(shape)
  return yv.cpu().numpy().reshape(shape), acc


@pytest.mark.parametrize("c", cc.CASES, ids=cc.IDS)
def test_currents_bit_equal(dev, c):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  e = cc.expected(c)
  w = _weight(c, dev)
  xw = packbits_lastaxis(e["x"])
  # the direct-form kernel, as every caller ran it before
  x = ops.PackedSpikes(_t(xw.view(np.int32), dev), c["cin"])
  yg, ag = ops.conv_forward(x, _geom(c), w, want_acc=True, impl="generic")
  np.testing.assert_array_equal(ag.cpu().numpy(), e["acc"])
  np.testing.assert_array_equal(_bits(yg), _bits(e["y"]))
  # the MFMA kernel, framed and misaligned, twice
  y1, a1 = _run_ex(c, w, xw, dev, L.IMPL_MFMA)
  print(cc.case_id(c), "acc differing from the oracle:", int((a1 != e["acc"]).sum()), "of", a1.size,
        "; current bits differing:", int((y1 != _bits(e["y"])).sum()))
  np.testing.assert_array_equal(a1, e["acc"])
  np.testing.assert_array_equal(y1, _bits(e["y"]))
  np.testing.assert_array_equal(y1, _bits(yg))
  y2, a2 = _run_ex(c, w, xw, dev, L.IMPL_AUTO)
  assert y1.tobytes() == y2.tobytes() and a1.tobytes() == a2.tobytes()
  # without the accumulators
  y3, _ = _run_ex(c, w, xw, dev, L.IMPL_MFMA, want_acc=False)
  assert y3.tobytes() == y1.tobytes()
  # and through ops.conv_forward
  ym = ops.conv_forward(x, _geom(c), w, impl="mfma")
  ya, aa = ops.conv_forward(x, _geom(c), w, want_acc=True)
  assert _bits(ym).tobytes() == y1.tobytes() and _bits(ya).tobytes() == y1.tobytes()
  np.testing.assert_array_equal(aa.cpu().numpy(), e["acc"])
  assert ops.device_status() == 0


def test_empty_batch(dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  c = cc.CASES[3]
  w = _weight(c, dev)
  g, ws = _geom(c).struct(), w.struct()
  sent = int(np.uint32(Y_SENTINEL).astype(np.int32))
  ybuf, yv = _framed(256, sent, dev)
  for impl in (L.IMPL_MFMA, L.IMPL_AUTO, L.IMPL_GENERIC):
    L.check(L.lib().snnqp_conv_forward_ex(None, L.BITS, 0, ctypes.byref(g), ctypes.byref(ws), ops._ptr(w.wt),
                                          ops._ptr(yv), None, impl, ops._stream()))
  torch.cuda.synchronize()
  assert (ybuf.cpu().numpy() == sent).all()
  x0 = ops.PackedSpikes(torch.zeros((0, c["H"], c["W"], (c["cin"] + 31) // 32), dtype=torch.int32, device=dev), c["cin"])
  y, acc = ops.conv_forward(x0, _geom(c), w, want_acc=True, impl="mfma")
  assert tuple(y.shape) == (0, c["H"], c["W"], c["cout"]) and tuple(acc.shape) == tuple(y.shape)


def test_cin_129_falls_back_under_auto_and_raises_under_mfma(dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  c = cc._case("q4", 129, 33, 5, 9, 1)
  e = cc.expected(c)
  w = _packed_kernel(e["leaf"], 4, dev).int_weight_mfma(64)
  x = ops.pack_bits(_t(e["x"], dev))
  yg = ops.conv_forward(x, _geom(c), w, impl="generic")
  ya = ops.conv_forward(x, _geom(c), w, impl="auto")
  np.testing.assert_array_equal(_bits(yg), _bits(e["y"]))
  assert _bits(ya).tobytes() == _bits(yg).tobytes()
  with pytest.raises(L.SnnqpError) as ei:
    ops.conv_forward(x, _geom(c), w, impl="mfma")
  assert ei.value.code == L.EUNSUPPORTED
  # with tiles that exist (Cin padded to 160 by hand) the library itself refuses, before any launch
  padded = w.w.new_zeros((3, 3, 160, 33))
  padded[:, :, :129] = w.w.reshape(3, 3, 129, 33)
  wt = dataclasses.replace(w, wt=ops.pack_codes_mfma(padded.reshape(-1, 33), 64), wt_cin=160)
  with pytest.raises(L.SnnqpError, match="Cin <= 128") as ei:
    ops.conv_forward(x, _geom(c), wt, impl="mfma")
  assert ei.value.code == L.EUNSUPPORTED
  ya2 = ops.conv_forward(x, _geom(c), wt, impl="auto")
  assert _bits(ya2).tobytes() == _bits(yg).tobytes()


@pytest.mark.parametrize("quant", ["q4p90", "q8p30"])
def test_quantconv_on_a_raster_switch_on_and_off(dev, quant):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops, synthetic as syn
  from snnquantprune_amd.flax_qconv import QuantConv
  c = cc._case(quant, 96, 48, 5, 9, 2)
  e = cc.expected(c)
  bits = cc.bits_of(c)
  cfg = syn.make_config(bits=bits, prune_percentage=cc.QUANTS[quant][1])
  conv = QuantConv(features=c["cout"], kernel_size=(3, 3), padding=cc.PADS, use_bias=False, config=cfg.quant,
                   bits=bits, g_scale=cfg.quant.g_scale)
  variables = nn.tree_from_numpy({"params": e["leaf"]}, dev)
  x = ops.pack_bits(_t(e["x"], dev))
  out = {}
  for on in (True, False):
    nn.set_train_conv_mfma(on)
    with torch.no_grad():
      out[on] = _bits(conv.apply(variables, x))
    np.testing.assert_array_equal(out[on], _bits(e["y"]), err_msg="switch %s" % on)
  assert out[True].tobytes() == out[False].tobytes()


# ---- training: the sown state, the logits and every gradient with the switch on and off ---------

def _train(dev, monkeypatch, channels, bits, on):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, packing, synthetic as syn, train_utils as tu
  v = syn.conv_net_variables(channels, cr.CIN, cr.NBLOCKS, cr.HW, cr.CLASSES * 10, True, 0.9,
                             gains=(4.0, 5.0, 8.0), random_bn=True)
  rng = np.random.default_rng(77)
  for i in range(cr.NBLOCKS):
    p = v["params"]["BatchNorm_%d" % i]
    p["scale"] = (1.5 + 0.2 * rng.standard_normal(channels)).astype(F32)
    p["bias"] = (0.5 + 0.1 * rng.standard_normal(channels)).astype(F32)
  x = np.minimum(rng.poisson(0.6, (cr.BATCH, cr.T_STEPS, cr.HW, cr.HW, cr.CIN)), 255).astype(np.uint8)
  cfg = syn.make_config(bits=bits, prune_percentage=0.9, channels=channels, tau=cr.TAU, quantized=True,
                        num_conv_blocks=cr.NBLOCKS, dropout=cr.KEEP)
  model = models.ConvDenseSNN(num_classes=cr.CLASSES, config=cfg)
  nn.set_train_conv_mfma(on)
  packing.clear_cache()
  tree = nn.tree_from_numpy(v, dev)

  def leaves(t):
    return {k: (leaves(s) if isinstance(s, dict) else s.detach().clone().requires_grad_(True)) for k, s in t.items()}

  params = leaves(tree["params"])
  routed = []                        # per conv connection launch: (input is a raster, tiled codes given)
  real = ops.conv_forward

  def spy(xx, geom, weight, *a, **kw):
    if geom.KH == 3:                   # (the read-out's connection comes through here as a 1x1)
      routed.append((isinstance(xx, ops.PackedSpikes), weight.wt is not None))
    return real(xx, geom, weight, *a, **kw)

  monkeypatch.setattr(ops, "conv_forward", spy)
  (logits, _), mut = model.apply({"params": params, "batch_stats": tree["batch_stats"]}, _t(x, dev), train=True,
                                 rng=11, mutable=["intermediates", "batch_stats"])
  labels = torch.arange(cr.BATCH, device=dev) % cr.CLASSES
  tu.mse_loss(logits, labels).backward()
  torch.cuda.synchronize()
  monkeypatch.setattr(ops, "conv_forward", real)
  # block 0 reads the uint8 frames; block 1 the raster, with the tiled codes iff the switch is on
  assert routed == [(False, False), (True, on)], routed
  grads = {}

  def walk(t, prefix):
    for k, s in t.items():
      if isinstance(s, dict):
        walk(s, prefix + (k,))
      else:
        grads[prefix + (k,)] = None if s.grad is None else s.grad.detach().cpu().numpy()

  walk(params, ())
  inter = {k: s[0].detach().cpu().numpy() for k, s in mut["intermediates"].items() if isinstance(s[0], torch.Tensor)}
  return logits.detach().cpu().numpy(), inter, grads


@pytest.mark.parametrize("channels,bits", [(cr.CHANNELS, cr.BITS), (40, 8)], ids=["c16-q4", "c40-q8"])
def test_training_bit_equal_switch_on_and_off(dev, monkeypatch, channels, bits):
  """Block 1 reads the bit-packed raster of block 0: Cin = 16 on the fp6 instruction, Cin = 40 with
  8-bit codes on the int8 one."""
  on = _train(dev, monkeypatch, channels, bits, True)
  off = _train(dev, monkeypatch, channels, bits, False)
  assert {"conv0_h", "conv1_h"} <= set(on[1])
  rate = float(on[1]["conv1_out"].mean())
  print("conv1 rate", rate)
  assert 0.0 < rate < 1.0
  for k in on[1]:
    assert on[1][k].tobytes() == off[1][k].tobytes(), k
  assert on[0].tobytes() == off[0].tobytes()
  assert set(on[2]) == set(off[2])
  n = 0
  for path, g in on[2].items():
    if g is None:
      assert off[2][path] is None, path
    else:
      assert g.tobytes() == off[2][path].tobytes(), path
      n += int(np.abs(g).max() > 0)
  assert n >= 6
