"""CPU suite: the launch forms of the gated ('gint') connections and of the fused dense head, and
the references their GPU tests use.

snnqp_conv_gated_plan / snnqp_dense_gated_plan / snnqp_dense_wide_plan report the host functions
the launches read their form from and need no device: every row of tests/gated_cases.py must take
the form it names, the tables must reach every form, and the rules are pinned at their edges.  The
references (oracle.gated_conv / gated_dense on raw codes) are checked against a float64 evaluation,
and the decoder formulas against what they promise."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import gated_cases as gc
from tests import train_reference as tr

F32 = np.float32
F64 = np.float64
FAKE = 0x7F0000001000              # an address no one reads


def _ops():
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  L.lib()
  return L, ops


def _plan(c):
  _, ops = _ops()
  return ops.conv_gated_plan(c.N, c.code_max) if c.kind == "conv" else ops.dense_gated_plan(c.N, c.code_max)


@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_every_row_takes_the_form_it_names(c):
  assert _plan(c) == c.form
  OT = -(-c.N // 32)
  if c.kind == "conv":                                   # the rule as DESIGN.md states it
    assert c.form == (OT // 4, OT % 4, c.code_max > 7)
  else:
    assert c.form == (-(-OT // 16), c.code_max > 7)
  assert 0 < c.code_lim <= c.code_max <= 127
  s, gate, codes = gc.data(c.name)
  assert int(np.abs(codes.astype(np.int32)).max()) == c.code_lim


def test_the_conv_table_reaches_every_form():
  """NT = 1, 2, 3, 4 alone, four tiles followed by each remainder, two full groups (blockIdx.y = 1)
  with and without a remainder: each on the narrow and on the wide kernel."""
  reached = {}
  for c in gc.CONV_FORMS:
    reached.setdefault(_plan(c), []).append(c.name)
  assert len(gc.ALL_CONV_FORMS) == 18
  assert set(reached) == gc.ALL_CONV_FORMS, sorted(gc.ALL_CONV_FORMS ^ set(reached))
  for form in sorted(reached):
    print("conv  full %d rest %d %-6s %s" % (form[0], form[1], "wide" if form[2] else "narrow", ", ".join(reached[form])))


def test_the_dense_table_reaches_every_form():
  """grid_y 1, 2 and 3, and every live tile count 1..4 of a wave as well as a wave with none: each
  narrow and wide."""
  by_grid, by_live = {}, {}
  for c in gc.DENSE_FORMS:
    gy, wide = _plan(c)
    by_grid.setdefault((gy, wide), []).append(c.name)
    live = gc.live_tiles(c)
    assert len(live) == gy and sum(map(sum, live)) == -(-c.N // 32)
    for n in {n for row in live for n in row}:
      by_live.setdefault((n, wide), []).append(c.name)
  assert set(by_grid) == {(g, w) for g in (1, 2, 3) for w in (False, True)}
  assert set(by_live) == {(n, w) for n in range(5) for w in (False, True)}
  for gy, wide in sorted(by_grid):
    print("dense grid_y %d %-6s %s" % (gy, "wide" if wide else "narrow", ", ".join(by_grid[(gy, wide)])))
  for n, wide in sorted(by_live):
    print("dense live tiles %d %-6s %s" % (n, "wide" if wide else "narrow", ", ".join(by_live[(n, wide)])))


def test_the_tables_cover_the_sizes_they_promise():
  """So that an edit cannot drop one unnoticed."""
  cv, dn = gc.CONV_FORMS, gc.DENSE_FORMS
  assert {c.C for c in cv} == {32, 64, 96, 128} == {c.C for c in dn}
  for wide in (False, True):
    assert {c.C for c in cv if c.form[2] == wide} == {32, 64, 96, 128}
    assert {(c.H, c.W) for c in cv if c.form[2] == wide} >= {(1, 1), (4, 8), (3, 9)}
  assert {(c.H, c.W) for c in cv} == {(1, 1), (4, 8), (3, 9), (5, 11)}
  assert {c.code_max for c in cv} == {7, 8, 15, 31, 127}
  assert {1, 33} <= {c.N for c in cv} and {256, 300} <= {c.N for c in cv}
  npatch = [c.NB * -(-c.H // 4) * -(-c.W // 8) for c in cv]
  assert any(n % 4 for n in npatch) and any(n % 4 == 0 for n in npatch) and any(n > 4 for n in npatch)
  assert {c.N for c in dn} == {1, 32, 33, 70, 128, 160, 512, 513, 600, 1100}
  assert {c.H for c in dn} == {1, 5, 6, 10, 11, 15, 16} and all(c.W == 1 for c in dn)
  assert {c.NB for c in dn} == {1, 31, 32, 33, 65}
  for wide in (False, True):
    assert {6, 11} <= {c.H for c in dn if c.form[1] == wide}        # a straddling position is the last
  for a, b in gc.SAME_DATA:
    ca, cb = gc.BY_NAME[a], gc.BY_NAME[b]
    assert (ca.code_max, cb.code_max, cb.code_lim) == (7, 8, 7) and ca.form[-1] is False and cb.form[-1] is True
    for x, y in zip(gc.data(a), gc.data(b)):
      np.testing.assert_array_equal(x, y)
    assert gc.dequant(ca) == gc.dequant(cb)
    np.testing.assert_array_equal(gc.reference(a), gc.reference(b))
  for name in gc.BLOCK_ROWS:
    c = gc.BY_NAME[name]
    assert (c.N > 128 and c.H % 2 == 0 and c.W % 2 == 0) if c.kind == "conv" else c.N > 512
  assert {gc.BY_NAME[n].form[-1] for n in gc.BLOCK_ROWS if gc.BY_NAME[n].kind == "conv"} == {False, True}
  sat = {(c.kind, c.codes, c.code_max) for c in gc.SATURATION}
  assert sat == {(k, s, m) for k in ("conv", "dense") for s in ("plus", "minus", "alt") for m in (7, 127)}
  assert {(c.kind, c.gates) for c in gc.GATE_EDGES} == {(k, g) for k in ("conv", "dense") for g in ("edges", "inf", "nan")}


def test_rules_at_their_boundaries():
  _, ops = _ops()
  assert ops.conv_gated_plan(128, 7) == (1, 0, False) and ops.conv_gated_plan(128, 8) == (1, 0, True)
  assert ops.conv_gated_plan(129, 7) == (1, 1, False) and ops.conv_gated_plan(129, 127) == (1, 1, True)
  assert ops.conv_gated_plan(256, 7) == (2, 0, False) and ops.conv_gated_plan(257, 7) == (2, 1, False)
  assert ops.conv_gated_plan(32, 1) == (0, 1, False) and ops.conv_gated_plan(33, 1) == (0, 2, False)
  assert ops.conv_gated_plan(96, 8) == (0, 3, True) and ops.conv_gated_plan(97, 8) == (1, 0, True)
  assert ops.dense_gated_plan(512, 7) == (1, False) and ops.dense_gated_plan(513, 7) == (2, False)
  assert ops.dense_gated_plan(512, 8) == (1, True) and ops.dense_gated_plan(513, 8) == (2, True)
  assert ops.dense_gated_plan(1024, 127) == (2, True) and ops.dense_gated_plan(1025, 127) == (3, True)


def _i8_weight(L, ops, code_max, w=None):
  return ops.Weight(L.W_I8, torch.zeros(4, dtype=torch.int8) if w is None else w, L=7.0, m=0.5, code_max=code_max)


def test_refusals():
  """Host-only paths of the library: the plan queries, the pack calls (refused before any launch)
  and the forward calls on NB = 0 images (refused, or accepted, before any launch)."""
  L, ops = _ops()
  lib = L.lib()
  i32 = ctypes.c_int32
  a, b, c = i32(), i32(), i32()
  for code_max in (0, 128, -1):
    assert lib.snnqp_conv_gated_plan(64, code_max, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == L.EINVAL
    assert lib.snnqp_dense_gated_plan(64, code_max, ctypes.byref(a), ctypes.byref(b)) == L.EINVAL
    assert lib.snnqp_pack_codes_gated_ex(FAKE, 32, 64, code_max, FAKE, None) == L.EINVAL
    assert lib.snnqp_pack_codes_dense_gated_ex(FAKE, 32, 4, 64, code_max, FAKE, None) == L.EINVAL
    assert lib.snnqp_conv_gated_packed_bytes_ex(32, 64, code_max) == 0
    assert lib.snnqp_dense_gated_packed_bytes_ex(32, 64, code_max) == 0
    with pytest.raises(L.SnnqpError):
      ops.conv_gated_plan(64, code_max)
    with pytest.raises(L.SnnqpError):
      ops.dense_gated_plan(64, code_max)
  assert lib.snnqp_conv_gated_plan(0, 7, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == L.EINVAL
  assert lib.snnqp_conv_gated_plan(64, 7, None, ctypes.byref(b), ctypes.byref(c)) == L.EINVAL
  assert lib.snnqp_dense_gated_plan(0, 7, ctypes.byref(a), ctypes.byref(b)) == L.EINVAL
  assert lib.snnqp_dense_gated_plan(64, 7, ctypes.byref(a), None) == L.EINVAL
  assert lib.snnqp_pack_codes_dense_gated_ex(FAKE, 32, 17, 64, 7, FAKE, None) == L.EINVAL      # HW 17
  P1 = ((1, 1), (1, 1))

  def conv(cin, code_max):
    g, w = ops.ConvGeom(4, 8, cin, 64, 3, 3, (1, 1), P1).struct(), _i8_weight(L, ops, code_max).struct()
    return lib.snnqp_conv_gated_forward(None, None, 0, ctypes.byref(g), ctypes.byref(w), FAKE, None, None)

  def dense(hw, c, code_max):
    w = _i8_weight(L, ops, code_max).struct()
    return lib.snnqp_dense_gated_forward(None, None, 0, hw, c, 64, ctypes.byref(w), FAKE, None, None)
  assert conv(64, 7) == L.OK and conv(64, 127) == L.OK and dense(16, 64, 7) == L.OK and dense(16, 64, 127) == L.OK
  assert conv(48, 7) == L.EUNSUPPORTED and b"input channels" in lib.snnqp_last_error()
  assert conv(160, 7) == L.EUNSUPPORTED and conv(0, 7) == L.EUNSUPPORTED
  assert conv(64, 0) == L.EUNSUPPORTED and b"code range" in lib.snnqp_last_error()
  assert conv(64, 128) == L.EUNSUPPORTED
  assert dense(17, 64, 7) == L.EUNSUPPORTED and b"16 positions" in lib.snnqp_last_error()
  assert dense(0, 64, 7) == L.EUNSUPPORTED and dense(16, 48, 7) == L.EUNSUPPORTED
  assert dense(16, 64, 0) == L.EUNSUPPORTED and dense(16, 64, 128) == L.EUNSUPPORTED
  # images given, but no raster to read them from
  g, w = ops.ConvGeom(4, 8, 64, 64, 3, 3, (1, 1), P1).struct(), _i8_weight(L, ops, 7).struct()
  assert lib.snnqp_conv_gated_forward(None, None, 2, ctypes.byref(g), ctypes.byref(w), FAKE, None, None) == L.EINVAL
  assert lib.snnqp_dense_gated_forward(None, None, 2, 16, 64, 64, ctypes.byref(w), FAKE, None, None) == L.EINVAL


@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_reference_against_float64(oracle, c):
  """The oracle's currents on the raw codes lie within gamma_(C + 2) of the float64 evaluation of
  sum_c gate[c] I[c] / L * m, relative to sum_c |gate[c]| |I[c]| / L * m: one rounding per fmaf and
  two in the dequantisation (train_reference.gamma), plus half a float32 subnormal spacing,
  2^-150, for every rounding that may land below the normal range.  I is summed here with explicit
  index ranges in float64, exact.  Derived, nothing tuned."""
  s, gate, codes = gc.data(c.name)
  t0 = time.perf_counter()
  ref = gc.reference(c.name)
  dt = time.perf_counter() - t0
  print("%s: C %d N %d NB %d, reference in %.3f s" % (c.name, c.C, c.N, c.NB, dt))
  assert ref.dtype == np.float32 and ref.shape == ((c.NB, c.H, c.W, c.N) if c.kind == "conv" else (c.NB, c.N))
  I = gc.channel_sums(c, s, codes)
  L, m = (F64(F32(v)) for v in gc.dequant(c))
  lim = 9 if c.kind == "conv" else gc.hw(c)
  assert np.abs(I).max() <= lim * c.code_lim and (I == np.rint(I)).all()
  if c.raster == "ones":
    assert np.abs(I).max() == lim * c.code_lim if c.codes != "alt" else np.abs(I).max() <= c.code_lim
  keep = np.ones(c.NB, bool)
  if c.gates in ("inf", "nan"):
    img, ch = gc.NONFINITE_AT
    assert not np.isfinite(gate[img, ch]) and np.isfinite(np.delete(gate.reshape(-1), img * c.C + ch)).all()
    keep[img] = False
    assert not np.isfinite(ref[img]).all() and np.isfinite(ref[keep]).all()
    if c.gates == "nan":
      assert np.isnan(ref[img]).all()
    else:                                                   # inf x 0 = NaN where the channel's sum is zero
      np.testing.assert_array_equal(np.isnan(ref[img]), (I[img][..., ch, :] == 0))
  else:
    assert np.isfinite(ref).all()
  g64 = gate.astype(F64)[keep]
  gsh = g64[:, None, None, :, None] if c.kind == "conv" else g64[:, :, None]
  axis = 3 if c.kind == "conv" else 1
  with np.errstate(under="ignore"):
    exact = (gsh * I[keep]).sum(axis) / L * m
    mag = (np.abs(gsh) * np.abs(I[keep])).sum(axis) / L * m
  err = np.abs(ref[keep].astype(F64) - exact)
  bound = tr.gamma(c.C + 2) * mag + (c.C + 2) * 2.0 ** -150
  assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
  if c.gates == "edges":
    assert (gate == 0).any() and np.signbit(gate[gate == 0]).any() and (gate < 0).any()
    assert (np.abs(gate) == F32(2.0 ** -130)).any() and (np.abs(gate) == F32(2.0 ** 100)).any()
    tiny = np.abs(ref[0::4])
    assert ((tiny > 0) & (tiny < np.finfo(F32).tiny)).any()           # subnormal currents occur


@pytest.mark.parametrize("name", [d[0] for d in gc.DECODERS])
def test_decoder_cases_show_every_code_at_every_place(name):
  """The code formula meets all 2 code_max + 1 values at every (tap or position, channel); the
  one-spike rasters make the current the code itself: checked with the exact channel sums."""
  _, kind, code_max = next(d for d in gc.DECODERS if d[0] == name)
  s, codes, expected = gc.decoder(name)
  P = 9 if kind == "conv" else gc.DEC_HW
  per_place = codes.reshape(P, gc.DEC_C, gc.DEC_N) if kind == "conv" else codes.reshape(gc.DEC_C, P, gc.DEC_N)
  values = np.arange(-code_max, code_max + 1)
  for v in values:
    assert (per_place == v).any(-1).all(), v
  assert int(np.abs(codes.astype(np.int32)).max()) == code_max
  for v in (code_max, -code_max, 8, -8, 120, -120):
    if abs(v) <= code_max:
      assert (per_place == v).any(-1).all()
  c = gc._case(name, kind, gc.DEC_C, gc.DEC_N, code_max, s.shape[1], s.shape[2], s.shape[0], ())
  I = gc.channel_sums(c, s, codes)
  assert s.sum() == s.shape[0] and (s.reshape(s.shape[0], -1).sum(1) == 1).all()
  np.testing.assert_array_equal(I.sum(-2), expected.astype(F64))          # one channel per image: the sum is the code
  assert (np.count_nonzero(I, axis=-2) <= 1).all()
  assert gc.decoder_mismatches(name, expected) == ""
  wrong = expected.copy()
  wrong[-1, ..., 3] += 1
  msg = gc.decoder_mismatches(name, wrong)
  assert "channel 127" in msg and "output 3" in msg and "code" in msg and ("tap" in msg or "position" in msg)


def test_decoder_reference_is_the_oracle_too(oracle):
  """(the decoder's expectation is index arithmetic; the oracle on the same data agrees)"""
  for name, kind, code_max in gc.DECODERS:
    s, codes, expected = gc.decoder(name)
    if kind == "dense":
      s, codes, expected = s[:64], codes[:4 * gc.DEC_HW], expected[:64]
      s = s[..., :4]
    qw = gc.RawWeight(codes, 1.0, 1.0)
    gate = np.ones((s.shape[0], s.shape[-1]), F32)
    got = oracle.gated_conv(s, gate, qw) if kind == "conv" else oracle.gated_dense(s, gate, qw)
    np.testing.assert_array_equal(got, expected)


# ---- the fused dense head ---------------------------------------------------------------------------

def test_head_shapes_reach_all_seven_fused_forms():
  """plan_wide for the fused head, with its workspace: (RT, CT, csplit) over the shapes of
  test_dense_head_as_one_launch / test_dense_head_on_float32_rows.  RT = 1 is chosen by no shape
  at all: below four MFMAs per k-step a choice costs (rounds of workgroups) x 4 whatever RT is, RT =
  2 never needs more rounds than RT = 1, and cost ties go to the larger tile -- only the
  SNNQP_DENSE_WIDE_RT override gets there (the variable is read on every call:
  tests/test_dense_int8_plans_cpu.py queries the forced forms, tests/test_dense_int8_plans_gpu.py
  launches them)."""
  _, ops = _ops()
  reached = {}
  for (T, B, K, N1, N2), form in gc.HEAD_SHAPES.items():
    rt, ct, sph, cs = ops.dense_wide_plan(T, B, N1, fused=True, may_split=True)
    assert (rt, ct, cs) == form, ((T, B, K, N1, N2), (rt, ct, cs))
    assert 1 <= sph <= 16 * rt // T and (ct == 2) == (N1 > 256 and not cs)
    reached.setdefault(form, []).append((T, B, K, N1, N2))
  assert len(gc.ALL_HEAD_FORMS) == 7 and set(reached) == gc.ALL_HEAD_FORMS
  for form in sorted(reached):
    print("head (RT %d, CT %d, csplit %d): %s" % (form + (reached[form],)))
  import inspect
  from tests import test_parity_gpu as tp
  for fn in (tp.test_dense_head_as_one_launch, tp.test_dense_head_on_float32_rows):
    shapes = next(m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == "shape")
    assert set(shapes) <= set(gc.HEAD_SHAPES), inspect.getsourcelines(fn)[1]
    assert {gc.HEAD_SHAPES[s] for s in shapes} >= {(3, 1, 1), (2, 2, 0), (3, 2, 0)}
  both = {gc.HEAD_SHAPES[s] for s in next(m.args[1] for m in tp.test_dense_head_as_one_launch.pytestmark
                                           if m.name == "parametrize" and m.args[0] == "shape")}
  assert both == gc.ALL_HEAD_FORMS


def test_head_workspace_is_a_ticket_head_and_two_raster_halves_per_tile():
  """snnqp_dense_head_workspace_bytes as a contract, restated here and not read from the library:
  a column-split launch hands over, per tile of 2 sph samples, two halves of the hidden raster of
  32 rt rows x 8 words of 4 bytes, behind a fixed head of 4096 bytes of tickets; a launch that does
  not split needs no workspace."""
  L, ops = _ops()
  split = 0
  for (T, B, K, N1, N2) in gc.HEAD_SHAPES:
    rt, ct, sph, cs = ops.dense_wide_plan(T, B, N1, fused=True, may_split=True)
    tiles = -(-B // (2 * sph))
    expected = 4096 + tiles * 2 * (32 * rt) * 8 * 4 if cs else 0
    assert int(L.lib().snnqp_dense_head_workspace_bytes(T, B, N1)) == expected, (T, B, K, N1, N2)
    split += cs
  assert 0 < split < len(gc.HEAD_SHAPES)


def test_no_shape_takes_another_head_form():
  L, ops = _ops()
  seen = set()
  for T in range(1, 65):
    for B in (1, 2, 3, 5, 8, 16, 31, 64, 100, 128, 129, 255, 256, 257, 300, 512, 1000, 3000, 4096, 10000, 65536):
      for N in (32, 200, 256, 257, 512):
        for may_split in (True, False):
          rt, ct, sph, cs = ops.dense_wide_plan(T, B, N, fused=True, may_split=may_split)
          assert rt != 1 and (rt, ct, cs) in gc.ALL_HEAD_FORMS, (T, B, N, may_split, (rt, ct, sph, cs))
          assert may_split or not cs
          seen.add((rt, ct, cs))
  assert seen == gc.ALL_HEAD_FORMS
  i32 = ctypes.c_int32
  a, b, c, d = i32(), i32(), i32(), i32()
  refs = [ctypes.byref(v) for v in (a, b, c, d)]
  lib = L.lib()
  assert lib.snnqp_dense_wide_plan(65, 4, 300, 1, 1, *refs) == L.EUNSUPPORTED
  assert lib.snnqp_dense_wide_plan(20, 4, 513, 1, 1, *refs) == L.EUNSUPPORTED
  assert lib.snnqp_dense_wide_plan(20, 4, 513, 0, 0, *refs) == L.OK and (b.value, d.value) == (2, 0)
  assert lib.snnqp_dense_wide_plan(0, 4, 300, 1, 1, *refs) == L.EINVAL
  assert lib.snnqp_dense_wide_plan(20, 0, 300, 1, 1, *refs) == L.EINVAL
  assert lib.snnqp_dense_wide_plan(20, 4, 300, 1, 1, None, *refs[1:]) == L.EINVAL
