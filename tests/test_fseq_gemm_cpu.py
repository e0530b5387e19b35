"""CPU suite: the dispatch of the float32-MFMA connection and the reference its GPU test uses.

snnqp_conv_float_form is the decision run_fseq_gemm launches from and needs no device: every entry
of tests/fseq_cases.py must take the instantiation it claims, the table must reach all 14, and the
tile rule is pinned at its edges.  The im2col reference is checked against oracle.quant_conv and
against the float64 product."""
import time

import numpy as np
import pytest
import torch

from tests import fseq_cases as fc
from tests import train_reference as tr

F64 = np.float64
FAKE = 0x7F0000001000              # an address no one reads: 4 KiB aligned


def _ops():
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  L.lib()
  return L, ops


def _weight(L, ops, wtype=None):
  # (the query never reads through the pointer: any non-null one serves)
  return ops.Weight(L.W_F32 if wtype is None else wtype, torch.zeros(4))


def _form(c):
  L, ops = _ops()
  geom = ops.ConvGeom(c.H, c.W, c.Cin, c.Cout, c.ks[0], c.ks[1], (1, 1), c.pads)
  return ops.conv_float_form((FAKE + c.offset, fc.IN_TYPES[c.kind]), geom, _weight(L, ops), NB=c.NB)


@pytest.mark.parametrize("c", fc.CASES, ids=[c.name for c in fc.CASES])
def test_every_entry_takes_the_form_it_claims(c):
  assert _form(c) == (c.kind,) + c.form
  M, K, N = fc.dims(c)
  tiles = -(-M // 128) * -(-N // 128)
  assert (c.form[1] == 128) == (tiles >= 192 and N > 64)          # the rule as DESIGN.md states it
  assert M % 128 != 0 or c.form[1] == 64                          # large tile: a ragged last row tile


def test_the_table_reaches_all_14_forms():
  reached = {}
  for c in fc.CASES:
    reached.setdefault(_form(c), []).append(c.name)
  assert len(fc.ALL_FORMS) == 14
  assert set(reached) == fc.ALL_FORMS, sorted(fc.ALL_FORMS - set(reached))
  for form in sorted(reached):
    print("%-16s %s" % (form, ", ".join(reached[form])))


def test_the_table_covers_the_edges_of_tile_and_chunk():
  """The sizes the case table promises, so that an edit cannot drop one unnoticed."""
  small = [fc.dims(c) for c in fc.SMALL]
  assert {1, 63, 64, 65, 129} <= {m for m, _, _ in small}
  assert {1, 31, 33, 63, 64, 65} <= {n for _, _, n in small}
  ks = {k for _, k, _ in small}
  assert {1, 15, 16, 17, 33} <= ks and max(ks) >= 48
  for c in fc.LARGE:
    M, K, N = fc.dims(c)
    assert M % 128 != 0 and N % 128 != 0 and K <= 144
  rag = {fc.dims(c)[2] % 128 for c in fc.LARGE}
  assert any(0 < r < 64 for r in rag) and any(r > 64 for r in rag)
  assert any(fc.dims(c)[2] % 4 == 0 for c in fc.LARGE) and any(fc.dims(c)[2] % 4 for c in fc.LARGE)
  cin = lambda kind, mode: {c.Cin for c in fc.CASES if c.kind == kind and c.form[0] == mode and not c.offset}
  assert {16, 48} <= cin("f32", 0) and {4, 12} <= cin("f32", 1) and {1, 2, 3} <= cin("f32", 2)
  assert 2 in cin("u8", 2) and 40 in cin("bits", 2)
  assert {24, 16} <= cin("u8", 3) and {50, 16, 32, 48} <= cin("bits", 3)
  assert any(c.offset % 2 for c in fc.CASES if c.kind == "u8") and any(c.nonfinite for c in fc.CASES)


@pytest.mark.parametrize("e", fc.TILE_EDGES, ids=[e[0] for e in fc.TILE_EDGES])
@pytest.mark.parametrize("kind", ["f32", "u8", "bits"])
def test_tile_rule_at_its_edges(e, kind):
  L, ops = _ops()
  _, NB, N, tile = e
  got = ops.conv_float_form((FAKE, fc.IN_TYPES[kind]), ops.ConvGeom(1, 1, 16, N, 1, 1), _weight(L, ops), NB=NB)
  assert got == (kind, 0 if kind == "f32" else 3, tile)


def test_uint8_alignment_decides_between_modes_3_and_2():
  L, ops = _ops()
  w = _weight(L, ops)
  conv, dense = ops.ConvGeom(7, 9, 16, 33, 3, 3, (1, 1), fc.P1), ops.ConvGeom(1, 1, 24, 33, 1, 1)
  for off in range(16):
    mode = 3 if off % 8 == 0 else 2
    assert ops.conv_float_form((FAKE + off, L.U8), conv, w, NB=2) == ("u8", mode, 64)
    assert ops.conv_float_form((FAKE + off, L.U8), dense, w, NB=70) == ("u8", mode, 64)
  # a host tensor serves as x: only its address, type and leading size count
  x = torch.zeros((2, 7, 9, 16), dtype=torch.uint8)
  assert ops.conv_float_form(x, conv, w) == ("u8", 3 if x.data_ptr() % 8 == 0 else 2, 64)
  assert ops.conv_float_form(torch.zeros((2, 7, 9, 16)), conv, w) == ("f32", 0, 64)
  assert ops.conv_float_form(ops.PackedSpikes(torch.zeros((2, 7, 9, 1), dtype=torch.int32), 16), conv, w) == ("bits", 3, 64)


@pytest.mark.parametrize("d", fc.DIRECT, ids=[d[0] for d in fc.DIRECT])
def test_other_geometries_report_the_direct_form(d):
  L, ops = _ops()
  _, H, W, Cin, Cout, ks, stride, pads, k_dil = d
  geom = ops.ConvGeom(H, W, Cin, Cout, ks[0], ks[1], stride, pads, (1, 1), k_dil)
  assert not ops.fseq_gemm_supported(geom)
  for in_type in (L.F32, L.U8, L.BITS):
    assert ops.conv_float_form((FAKE, in_type), geom, _weight(L, ops), NB=3) == "direct"


def test_integer_codes_and_malformed_requests():
  L, ops = _ops()
  lib = L.lib()
  geom = ops.ConvGeom(8, 8, 16, 32, 3, 3, (1, 1), fc.P1)
  assert ops.conv_float_form((FAKE, L.BITS), geom, _weight(L, ops, L.W_I8), NB=3) == "direct"
  assert ops.conv_float_form((FAKE, L.F32), geom, _weight(L, ops), NB=0) == ("f32", 0, 64)
  g, w = geom.struct(), _weight(L, ops).struct()
  x = torch.zeros(1).data_ptr()
  byref = __import__("ctypes").byref
  assert lib.snnqp_conv_float_form(x, L.F32, 3, None, byref(w)) == L.EINVAL
  assert lib.snnqp_conv_float_form(x, L.F32, 3, byref(g), None) == L.EINVAL
  assert lib.snnqp_conv_float_form(None, L.F32, 3, byref(g), byref(w)) == L.EINVAL
  assert lib.snnqp_conv_float_form(x, L.F32, -1, byref(g), byref(w)) == L.EINVAL
  assert lib.snnqp_conv_float_form(x, L.F32, 1 << 31, byref(g), byref(w)) == L.EINVAL
  assert lib.snnqp_conv_float_form(x, L.EV1, 3, byref(g), byref(w)) == L.EINVAL
  null_w = L.WeightT(L.W_F32, None, 1.0, 1.0)
  assert lib.snnqp_conv_float_form(x, L.F32, 3, byref(g), byref(null_w)) == L.EINVAL
  bad = ops.ConvGeom(8, 8, 16, 32, 3, 3, (1, 1), fc.P1, groups=3).struct()     # 16 % 3 != 0
  assert lib.snnqp_conv_float_form(x, L.F32, 3, byref(bad), byref(w)) == L.EINVAL
  with pytest.raises(L.SnnqpError):
    ops.conv_float_form((0, L.F32), geom, _weight(L, ops), NB=3)
  with pytest.raises(ValueError):
    ops.conv_float_form((FAKE, L.F32), geom, _weight(L, ops))


@pytest.mark.parametrize("c", fc.CASES, ids=[c.name for c in fc.CASES])
def test_reference_against_the_oracle_and_float64(oracle, c):
  """The explicit im2col + C fmaf chain equals oracle.quant_conv(mode="fseq"), which gathers from a
  padded copy; and it lies within gamma_K sum |x||w| of the float64 product -- one rounding per
  fmaf (train_reference.gamma): derived, nothing tuned."""
  _, x, w = fc.data(c.name)
  M, K, N = fc.dims(c)
  t0 = time.perf_counter()
  ref = fc.reference(c.name)
  dt = time.perf_counter() - t0
  print("%s: M %d K %d N %d, reference in %.3f s" % (c.name, M, K, N, dt))
  assert ref.shape == (c.NB, c.H, c.W, N) and ref.dtype == np.float32
  want = oracle.quant_conv(x, oracle.QWeight(w), None, c.pads, mode="fseq")
  np.testing.assert_array_equal(ref, want)
  cols = fc.im2col(x, c.ks, c.pads)
  if c.nonfinite:
    bad = ~np.isfinite(cols).all(1)
    assert 0 < bad.sum() < M                                # some rows see inf / NaN, not all
    assert np.isnan(ref.reshape(M, N)[bad]).any() and np.isfinite(ref.reshape(M, N)[~bad]).all()
    cols = cols[~bad]
    ref = ref.reshape(M, N)[~bad]
  exact = cols.astype(F64) @ w.reshape(K, N).astype(F64)
  mag = np.abs(cols).astype(F64) @ np.abs(w.reshape(K, N)).astype(F64)
  err = np.abs(ref.reshape(exact.shape).astype(F64) - exact)
  assert (err <= tr.gamma(K) * mag).all(), float((err / np.maximum(mag, 1e-300)).max() / tr.gamma(K))
  if c.kind != "f32":
    assert (x == np.rint(x)).all() and x.min() >= 0 and x.max() == (255 if c.kind == "u8" else 1)
