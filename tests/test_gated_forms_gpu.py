"""GPU suite: the gated ('gint') connections (csrc/conv_gated.hip, dense_gated.hip) alone, one
launch of snnqp_conv_gated_forward / snnqp_dense_gated_forward per row of tests/gated_cases.py --
every launch form, narrow and wide; every code value at every tap, position and channel; saturated
rasters; gates that are zero, negative, subnormal, huge, infinite or NaN -- bit for bit against the
oracle on raw codes, with framed operands and outputs."""
import ctypes
import time

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import gated_cases as gc
from tests.helpers import packbits_lastaxis, qweight_of
from tests.train_helpers import PAD, _frame_untouched, _framed, _np

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -12345.5
CODE_FILL = 0x5A                      # frame of the packed codes: bytes no pack kernel writes
P1 = ((1, 1), (1, 1))


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  L.lib()
  return torch.device("cuda:0")


def _t(a, dev):
  return torch.from_numpy(np.array(a)).to(dev)                  # (a copy: the shared data is read-only)


def _words(dev, s):
  """The raster as the kernels read it: spike words inside a frame of all-ones words (a read
  outside the raster would show as spikes): (whole, view [NB, H, W, CW] int32)."""
  w = packbits_lastaxis(s).view(np.int32)
  whole = torch.full((w.size + 2 * PAD,), -1, dtype=torch.int32, device=dev)
  view = whole[PAD:PAD + w.size].view(w.shape)
  view.copy_(torch.from_numpy(np.array(w)))
  return whole, view


def _pack(dev, kind, codes_d, C, HW, N, code_max):
  """The codes in the operand layout, packed by the library into a framed buffer: (whole, view)."""
  lib = L.lib()
  if kind == "conv":
    n = int(lib.snnqp_conv_gated_packed_bytes_ex(C, N, code_max))
  else:
    n = int(lib.snnqp_dense_gated_packed_bytes_ex(C, N, code_max))
  assert n == C * -(-N // 32) * 64 * (8 if kind == "conv" else 16)
  whole = torch.full((n + 2 * PAD,), CODE_FILL, dtype=torch.uint8, device=dev)
  view = whole[PAD:PAD + n]
  assert view.data_ptr() % 16 == 0
  if kind == "conv":
    L.check(lib.snnqp_pack_codes_gated_ex(ops._ptr(codes_d), C, N, code_max, ops._ptr(view), ops._stream()))
    same = ops.pack_codes_gated(codes_d, code_max)
  else:
    L.check(lib.snnqp_pack_codes_dense_gated_ex(ops._ptr(codes_d), C, HW, N, code_max, ops._ptr(view), ops._stream()))
    same = ops.pack_codes_dense_gated(codes_d, C, HW, code_max)
  torch.cuda.synchronize()
  assert bool((whole[:PAD] == CODE_FILL).all()) and bool((whole[PAD + n:] == CODE_FILL).all()), "pack wrote outside"
  assert torch.equal(same, view)
  return whole, view


class _Run:
  """One problem on the device: framed raster, gates and packed codes; launch() runs the forward
  into a fresh sentinel-framed output and checks every frame."""

  def __init__(self, dev, kind, s, gate, codes, code_max, Lq, m):
    self.dev, self.kind = dev, kind
    self.NB, self.H, self.W, self.C = s.shape
    self.N = codes.shape[-1]
    self.code_max = code_max
    self.keep_s, self.sv = _words(dev, s)
    self.keep_g, self.gv = _framed(dev, np.array(gate), np.nan)
    self.codes_d = _t(codes, dev)
    self.keep_p, self.pv = _pack(dev, kind, self.codes_d, self.C, self.H * self.W, self.N, code_max)
    self.weight = ops.Weight(L.W_I8, self.codes_d, L=Lq, m=m, code_max=code_max)
    self.packed_bytes = self.pv.clone()

  def launch(self, NB=None):
    NB = self.NB if NB is None else NB
    shape = (self.NB, self.H, self.W, self.N) if self.kind == "conv" else (self.NB, self.N)
    ow, ov = _framed(self.dev, np.full(shape, SENTINEL, F32), SENTINEL)
    w = self.weight.struct()
    if self.kind == "conv":
      g = ops.ConvGeom(self.H, self.W, self.C, self.N, 3, 3, (1, 1), P1).struct()
      L.check(L.lib().snnqp_conv_gated_forward(ops._ptr(self.sv), ops._ptr(self.gv), NB, ctypes.byref(g),
                                               ctypes.byref(w), ops._ptr(self.pv), ops._ptr(ov), ops._stream()))
    else:
      L.check(L.lib().snnqp_dense_gated_forward(ops._ptr(self.sv), ops._ptr(self.gv), NB, self.H * self.W, self.C,
                                                self.N, ctypes.byref(w), ops._ptr(self.pv), ops._ptr(ov),
                                                ops._stream()))
    torch.cuda.synchronize()
    assert _frame_untouched(ow, ov.numel(), SENTINEL), "wrote outside y"
    assert bool((self.keep_p[:PAD] == CODE_FILL).all()) and bool((self.keep_p[PAD + self.pv.numel():] == CODE_FILL).all())
    assert torch.equal(self.pv, self.packed_bytes), "the packed codes changed"
    return ov


def _run_of(dev, c):
  s, gate, codes = gc.data(c.name)
  Lq, m = gc.dequant(c)
  return _Run(dev, c.kind, s, gate, codes, c.code_max, Lq, m)


def _assert_same_bits(got, want, what):
  """Bit-equal, NaN meeting NaN (the payload of a NaN the arithmetic makes is not part of the
  contract)."""
  nan = np.isnan(want)
  np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what + ": NaN positions")
  np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg=what)


@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_row_bit_equal_reference(dev, c):
  t0 = time.perf_counter()
  want = gc.reference(c.name)
  t1 = time.perf_counter()
  run = _run_of(dev, c)
  plan = ops.conv_gated_plan(c.N, c.code_max) if c.kind == "conv" else ops.dense_gated_plan(c.N, c.code_max)
  assert plan == c.form
  got = _np(run.launch())
  nan = np.isnan(want)
  diff = int((got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan]).sum())
  print("%s: form %s: differing elements %d of %d (reference %.3f s, GPU part %.3f s)"
        % (c.name, c.form, diff, want.size, t1 - t0, time.perf_counter() - t1))
  assert not (got == SENTINEL).any(), "an output was not written"
  _assert_same_bits(got, want, c.name)
  if c.gates in ("inf", "nan"):
    img = gc.NONFINITE_AT[0]
    assert nan[img].any() if c.gates == "inf" else nan[img].all()
    assert not np.isfinite(got[img]).all()
    assert np.isfinite(np.delete(got, img, axis=0)).all(), "a non-finite gate of one image reached another"
  else:
    assert np.isfinite(got).all()
  again = _np(run.launch())
  np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))
  assert ops.device_status() == 0


@pytest.mark.parametrize("pair", gc.SAME_DATA, ids=[p[1] for p in gc.SAME_DATA])
def test_codes_to_7_give_the_same_bits_in_both_layouts(dev, pair):
  narrow, wide = (gc.BY_NAME[n] for n in pair)
  assert gc.dequant(narrow) == gc.dequant(wide)
  a = _np(_run_of(dev, narrow).launch())
  b = _np(_run_of(dev, wide).launch())
  np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
  np.testing.assert_array_equal(b.view(np.uint32), gc.reference(narrow.name).view(np.uint32))


@pytest.mark.parametrize("name", [d[0] for d in gc.DECODERS])
def test_decoder(dev, name):
  """Every code value -code_max..code_max at every tap / position of every channel, met by one
  spike alone under gate = L = m = 1: the current is the code, asserted from the index arithmetic."""
  _, kind, code_max = next(d for d in gc.DECODERS if d[0] == name)
  s, codes, expected = gc.decoder(name)
  gate = np.ones((s.shape[0], s.shape[-1]), F32)
  run = _Run(dev, kind, s, gate, codes, code_max, 1.0, 1.0)
  got = _np(run.launch())
  assert not (got == SENTINEL).any(), "an output was not written"
  msg = gc.decoder_mismatches(name, got)
  assert msg == "", "\n" + msg
  again = _np(run.launch())
  np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))
  assert ops.device_status() == 0


@pytest.mark.parametrize("name", ["n_nt4_1_cout129", "w_two_groups_2_cout300", "n_n513", "w_n70_codes_to_7"])
def test_no_images_write_nothing(dev, name):
  run = _run_of(dev, gc.BY_NAME[name])
  ov = run.launch(NB=0)                                     # rc OK (L.check), frames untouched
  assert bool((ov == SENTINEL).all())
  assert ops.device_status() == 0


def _leaf_of(c, codes, oracle):
  """A reference-style parameter leaf whose DuQ codes are the row's raw codes: kernel = code / L with
  a = 1 (q = round(hard_tanh(kernel) L) = code), c = the row's m."""
  Lq, m = gc.dequant(c)
  bits = {7: 4, 127: 8}[c.code_max]
  assert c.code_lim == c.code_max
  assert 2 ** (bits - 1) - 1 == Lq
  kernel = (codes.astype(F32) / F32(Lq)).astype(F32)
  leaf = {"kernel": kernel, "DuQ_0": {"a": np.array([1.0], F32), "c": np.array([m], F32)},
          "prune_0": {"mask": np.ones(kernel.shape, F32)}}
  qw = qweight_of(oracle, leaf, bits)
  np.testing.assert_array_equal(qw.q, codes.astype(F32))
  assert qw.L == F32(Lq) and qw.m == F32(m)
  return leaf, qw, bits


@pytest.mark.parametrize("name", gc.BLOCK_ROWS)
def test_row_as_a_spiking_block(dev, oracle, name):
  """Rows past one tile group (Cout > 128, narrow and wide) and past one workgroup of outputs
  (N > 512) as the model runs them: SpikingBlock with BatchNorm, the scan and pool 1 and 2 against
  oracle.gated_conv_block; the dense row against oracle.gated_dense_block."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import synthetic as syn
  from snnquantprune_amd.flax_qconv import QuantConv
  from snnquantprune_amd.flax_qdense import QuantDense
  from snnquantprune_amd.spiking_learning import SpikingBlock
  c = gc.BY_NAME[name]
  s, gate, codes = gc.data(name)
  leaf, qw, bits = _leaf_of(c, codes, oracle)
  T = 2 if c.kind == "conv" else 4
  B = c.NB // T
  assert T * B == c.NB
  s5, g3 = s.reshape((T, B) + s.shape[1:]), gate.reshape(T, B, c.C)
  np.testing.assert_array_equal(
      np.concatenate([(oracle.gated_conv if c.kind == "conv" else oracle.gated_dense)(s5[t], g3[t], qw) for t in range(T)]),
      gc.reference(name))
  x = ops.GatedSpikes(ops.pack_bits(_t(s5, dev)), _t(g3, dev))
  cfg = syn.make_config(bits=bits, prune_percentage=0.9)
  if c.kind == "dense":
    blk = SpikingBlock(connection_fn=QuantDense(c.N, use_bias=False, config=cfg.quant, bits=bits, g_scale=cfg.quant.g_scale),
                       neural_dynamics=cfg.neuron_dynamics(dtype=torch.float32), return_state=True)
    u, sp = blk.apply(nn.tree_from_numpy({"params": {"connection_fn": leaf}}, dev), None, x.flattened())
    eu, es = oracle.gated_dense_block(s5.astype(F32), g3, qw)
    assert 0.01 < es.mean() < 0.99
    np.testing.assert_array_equal(_np(sp.bits).view(np.uint32), packbits_lastaxis(es))
    np.testing.assert_array_equal(_np(u), eu)
  else:
    bp, bs = syn.bn_leaf(c.N, True, 972)
    bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
    eu, es = oracle.gated_conv_block(s5.astype(F32), g3, qw, bn)
    assert 0.01 < es.mean() < 0.99
    variables = nn.tree_from_numpy({"params": {"connection_fn": leaf, "norm_fn": {"scale": bn["scale"], "bias": bn["bias"]}},
                                    "batch_stats": {"norm_fn": {"mean": bn["mean"], "var": bn["var"]}}}, dev)
    for pool in (1, 2):
      blk = SpikingBlock(connection_fn=QuantConv(features=c.N, kernel_size=(3, 3), padding=P1, use_bias=False,
                                                 config=cfg.quant, bits=bits, g_scale=cfg.quant.g_scale),
                         neural_dynamics=cfg.neuron_dynamics(dtype=torch.float32),
                         norm_fn=nn.BatchNorm(use_running_average=True, momentum=0.9, epsilon=1e-5),
                         pool=pool, return_state=True)
      u, sp = blk.apply(variables, None, x)
      np.testing.assert_array_equal(_np(sp.bits).view(np.uint32),
                                    packbits_lastaxis(oracle.max_pool_2x2(es) if pool == 2 else es))
      np.testing.assert_array_equal(_np(u), eu)
  assert ops.device_status() == 0
