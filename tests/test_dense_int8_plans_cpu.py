"""CPU suite: the launch plans of the two int8 dense kernels as the library reports them --
snnqp_dense_mfma_plan (csrc/dense_mfma.hip, 128 columns per workgroup) and snnqp_dense_wide_plan
(csrc/dense_wide.hip), the functions the launches themselves read -- and the case table of
tests/dense_int8_plan_cases.py that the GPU file forces through SNNQP_DENSE_MFMA_RT and
SNNQP_DENSE_WIDE_RT.

Properties of the plans, not the cost models restated: what a plan may be, what the knobs may and
may not change, and that they are read on every call.  Then the table: every kernel instance has
cells, every K and N of its lists meets every rt, and the oracle's spike rate of every cell is in a
band where a wrong sum changes the raster.  No GPU call is made."""
import ctypes
import itertools
import os
import sys

import pytest

from tests import dense_int8_plan_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFMA_KNOB, WIDE_KNOB, NOSPLIT_KNOB = "SNNQP_DENSE_MFMA_RT", "SNNQP_DENSE_WIDE_RT", "SNNQP_DENSE_HEAD_NOSPLIT"


@pytest.fixture(scope="module")
def L():
  from snnquantprune_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
  _lib.lib()
  return _lib


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
  for k in (MFMA_KNOB, WIDE_KNOB, NOSPLIT_KNOB):
    monkeypatch.delenv(k, raising=False)


def _mfma(L, in_type, T, B, N, expect=0):
  v = [ctypes.c_int32(-99) for _ in range(4)]
  rc = L.lib().snnqp_dense_mfma_plan({"bits": L.BITS, "u8": L.U8}.get(in_type, in_type), T, B, N,
                                     *[ctypes.byref(x) for x in v])
  assert rc == expect, (rc, L.lib().snnqp_last_error())
  return tuple(x.value for x in v)


def _wide(L, T, B, N, fused=False, may_split=False, expect=0):
  v = [ctypes.c_int32(-99) for _ in range(4)]
  rc = L.lib().snnqp_dense_wide_plan(T, B, N, int(fused), int(may_split), *[ctypes.byref(x) for x in v])
  assert rc == expect, (rc, L.lib().snnqp_last_error())
  return tuple(x.value for x in v)


MFMA_GRID = list(itertools.product(("bits", "u8"), (1, 7, 20, 32, 33, 64, 65, 96), (1, 9, 130, 300, 801, 1024, 5000),
                                   (1, 33, 110, 128, 129, 700)))
WIDE_GRID = list(itertools.product((1, 3, 5, 16, 17, 20, 32, 33, 48, 49, 64), (1, 9, 17, 130, 300, 1024, 4096, 70000),
                                   (129, 256, 257, 512, 513, 700), (False, True)))


def _mfma_ok(in_type, T, B, N, plan):
  rt, sb, gx, gy = plan
  assert 1 <= rt <= (2 if in_type == "u8" else 3) and 32 * rt >= T, (in_type, T, B, N, plan)
  assert sb == 32 * rt // T and sb >= 1
  assert gx == dc.ceil_div(B, sb) and gy == dc.ceil_div(N, 128)


def _wide_ok(T, B, N, fused, plan):
  rt, ct, sph, cs = plan
  assert 1 <= rt <= 4 and 16 * rt >= T, (T, B, N, fused, plan)
  assert 1 <= sph <= 16 * rt // T and sph <= (8 if fused else 64)
  assert ct == (2 if N > 256 and not cs else 1)
  assert not cs or fused


def test_mfma_plan_properties_and_the_knob(L, monkeypatch):
  for in_type, T, B, N in MFMA_GRID:
    if in_type == "u8" and T > 64:
      _mfma(L, in_type, T, B, N, expect=L.EUNSUPPORTED)
      continue
    free = _mfma(L, in_type, T, B, N)
    _mfma_ok(in_type, T, B, N, free)
    for rt in (1, 2, 3):
      monkeypatch.setenv(MFMA_KNOB, str(rt))
      got = _mfma(L, in_type, T, B, N)
      _mfma_ok(in_type, T, B, N, got)
      if 32 * rt >= T and rt <= (2 if in_type == "u8" else 3):
        assert got[0] == rt, (in_type, T, B, N, rt, got)
      else:
        assert got == free, "an rt that holds no sample, or a third row tile for uint8 rows, is ignored"
    for bad in ("0", "4", "-1", "x", ""):
      monkeypatch.setenv(MFMA_KNOB, bad)
      assert _mfma(L, in_type, T, B, N) == free, bad
    monkeypatch.delenv(MFMA_KNOB)
    assert _mfma(L, in_type, T, B, N) == free, "unset: the default again, in the same process"


def test_the_mfma_query_refuses_what_the_launch_refuses(L):
  assert _mfma(L, "bits", 96, 4, 33)[0] == 3
  _mfma(L, "bits", 97, 4, 33, expect=L.EUNSUPPORTED)
  assert b"96" in L.lib().snnqp_last_error()
  assert _mfma(L, "u8", 64, 4, 33)[0] == 2
  _mfma(L, "u8", 65, 4, 33, expect=L.EUNSUPPORTED)
  for bad in ((0, 4, 33), (20, 0, 33), (20, 4, 0), (-1, 4, 33)):
    _mfma(L, "bits", *bad, expect=L.EINVAL)
  _mfma(L, L.F32, 20, 4, 33, expect=L.EINVAL)
  i32 = ctypes.c_int32
  a, b, c = i32(), i32(), i32()
  lib = L.lib()
  assert lib.snnqp_dense_mfma_plan(L.BITS, 20, 4, 33, None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == L.EINVAL
  assert lib.snnqp_dense_mfma_plan(L.BITS, 20, 4, 33, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), None) == L.EINVAL
  from snnquantprune_amd import ops
  assert ops.dense_mfma_plan(L.BITS, 20, 33, 70) == _mfma(L, "bits", 20, 33, 70)


def test_wide_plan_properties_and_the_knob(L, monkeypatch):
  for T, B, N, fused in WIDE_GRID:
    if fused and N > 512:
      _wide(L, T, B, N, fused, True, expect=L.EUNSUPPORTED)
      continue
    for may_split in ((False, True) if fused else (False,)):
      free = _wide(L, T, B, N, fused, may_split)
      _wide_ok(T, B, N, fused, free)
      assert free[2] == dc.wide_sph(free[0], T, fused)
      for rt in (1, 2, 3, 4):
        monkeypatch.setenv(WIDE_KNOB, str(rt))
        got = _wide(L, T, B, N, fused, may_split)
        _wide_ok(T, B, N, fused, got)
        if 16 * rt >= T:
          assert got[0] == rt and got[2] == dc.wide_sph(rt, T, fused), (T, B, N, fused, rt, got)
        else:
          assert got == free, "an rt that holds no sample is ignored"
      for bad in ("0", "5", "-2", "x", ""):
        monkeypatch.setenv(WIDE_KNOB, bad)
        assert _wide(L, T, B, N, fused, may_split) == free, bad
      monkeypatch.delenv(WIDE_KNOB)
      assert _wide(L, T, B, N, fused, may_split) == free, "unset: the default again, in the same process"


def test_the_head_knobs_are_read_on_every_call(L, monkeypatch):
  """The three fused forms at RT = 1 that no shape reaches by itself, the workspace query following
  the knobs, and all of it back to the default once they are unset."""
  lib = L.lib()
  T, B, N1 = 16, 17, 512
  free = _wide(L, T, B, N1, True, True)
  free_ws = int(lib.snnqp_dense_head_workspace_bytes(T, B, N1))
  assert free[0] != 1 and free[3] == 1 and free_ws > 0
  monkeypatch.setenv(WIDE_KNOB, "1")
  assert _wide(L, T, B, N1, True, True) == (1, 1, 1, 1)
  gx = dc.ceil_div(B, 2)
  assert int(lib.snnqp_dense_head_workspace_bytes(T, B, N1)) == 4096 + gx * 2 * 32 * 8 * 4
  assert _wide(L, T, B, N1, True, False) == (1, 2, 1, 0)
  monkeypatch.setenv(NOSPLIT_KNOB, "1")
  assert _wide(L, T, B, N1, True, True) == (1, 2, 1, 0)
  assert int(lib.snnqp_dense_head_workspace_bytes(T, B, N1)) == 0
  monkeypatch.delenv(NOSPLIT_KNOB)
  assert _wide(L, T, B, N1, True, True) == (1, 1, 1, 1)
  assert _wide(L, T, B, 160, True, True) == (1, 1, 1, 0)
  monkeypatch.delenv(WIDE_KNOB)
  assert _wide(L, T, B, N1, True, True) == free
  assert int(lib.snnqp_dense_head_workspace_bytes(T, B, N1)) == free_ws
  for form, (T, B, K, N1, N2) in dc.HEAD_CELLS.items():
    assert T <= 16 and B == 17 and K % 16 == 0
    monkeypatch.setenv(WIDE_KNOB, "1")
    rt, ct, _, cs = _wide(L, T, B, N1, True, bool(form[2]))
    assert (rt, ct, cs) == form
    monkeypatch.delenv(WIDE_KNOB)
    assert _wide(L, T, B, N1, True, True)[0] != 1
  T, B, K, N1, N2 = dc.HEAD_STATE_CELL
  assert 2 * T <= 16 and dc.HEAD_STATE_FORM[0] == 1


def test_the_defaults_leave_instances_to_the_knobs(L):
  """Why the knobs are needed.  Stand-alone wide kernel at B <= 300: one column tile only ever runs
  with four row tiles, two column tiles with two to four.  128-column kernel: three row tiles with
  several samples per workgroup only from about 200 SB samples upward (SB = 4 at T = 20: B > 796)."""
  seen = {1: set(), 2: set()}
  for T in range(1, 65):
    for B in range(1, 301):
      for N in dc.WIDE_N_ALL:
        rt, ct, sph, cs = _wide(L, T, B, N)
        seen[ct].add(rt)
  assert seen == {1: {4}, 2: {2, 3, 4}}, seen
  for T in range(1, 33):                        # SB > 1 at rt = 3 needs T <= 48; at T <= 32 rt = 1 holds a sample too
    sb = 96 // T
    for N in (33, 128):
      for B in (1, 9, 130, 199 * sb):
        rt, psb, gx, gy = _mfma(L, "bits", T, B, N)
        assert rt < 3 or psb == 1, (T, B, N, rt, psb)
      assert _mfma(L, "bits", T, 199 * sb + 1, N)[:2] == (3, sb)
  for (in_type, T, B, K, N), (rt, sb) in dc.SHIPPED_CELLS.items():
    got = _mfma(L, in_type, T, B, N)
    assert got[:2] == (rt, sb) and B % sb == 1 and got[2] == dc.ceil_div(B, sb), (got, "a one-sample last workgroup")
  # the suite's other shapes (B <= 130): a workgroup of rt 2 or 3 always holds ONE sample
  for T in range(1, 97):
    for B in (1, 16, 39, 130):
      rt, sb, _, _ = _mfma(L, "bits", T, B, 110)
      assert rt == 1 or sb == 1, (T, B, rt, sb)


def test_the_table_reaches_every_instance_k_and_n(L, monkeypatch):
  """Every (kernel, input type, rt[, ct]) instance has cells (printed: instance -> cells), every K of
  every list and every N meets every rt, every cell's batch has nine workgroups (or the even tail),
  and the plan each cell names is the plan the knob gives."""
  lines = []
  assert len(dc.MFMA_PLANS) == 5 and len(dc.WIDE_PLANS) * 3 == 4 * 2 * 3
  for in_type, rt in dc.MFMA_PLANS:
    cells = dc.mfma_cells(in_type, rt)
    lines.append("dense_mfma_kernel<%d, %s>: %d cells" % (rt, in_type, len(cells)))
    assert {K for _, _, K, _ in cells} == set(dc.mfma_k_list(in_type))
    for T, B in {(T, B) for T, B, _, _ in cells}:
      assert {K for t, b, K, _ in cells if (t, b) == (T, B)} == set(dc.mfma_k_list(in_type)), "every row shape at every K"
    want_n = set(dc.MFMA_N) | (set(dc.MFMA_N_LONG) if (in_type, rt) == ("bits", 3) else set())
    assert {N for *_, N in cells} == want_n
    sbs = {dc.mfma_sb(rt, T) for T, _, _, _ in cells}
    assert 1 in sbs and max(sbs) > 1, (in_type, rt, sbs)
    assert any(T == 32 * rt for T, _, _, _ in cells), "full row tiles"
    assert any(T == 20 for T, _, _, _ in cells)
    monkeypatch.setenv(MFMA_KNOB, str(rt))
    for T, B, K, N in cells:
      sb = dc.mfma_sb(rt, T)
      gx, gy = dc.mfma_grid(rt, T, B, N)
      assert _mfma(L, in_type, T, B, N) == (rt, sb, gx, gy)
      assert (gx == 9 and B == 8 * sb + 1) or (gx == 8 and B == 8 * sb), (T, B, "nine workgroups, or the even tail")
      if N > 128:
        # T <= 64 with N > 128 belongs to the wide kernel: these cells have more steps than it takes
        assert T > 64 and in_type == "bits"
        _wide(L, T, B, N, expect=L.EUNSUPPORTED)
    monkeypatch.delenv(MFMA_KNOB)
  assert any(B == 8 * dc.mfma_sb(2, T) for T, B, _, _ in dc.mfma_cells("bits", 2)), "the even-tailed batch"
  # T <= 64 and N > 128: the wide kernel's (its plan query succeeds), so the table keeps such cells out
  assert _wide(L, 64, 9, 129)[0] >= 1 and _wide(L, 20, 33, 160)[0] >= 1
  assert [dc.mfma_group_chunks(K) for K in dc.MFMA_K_BITS] == [1, 1, 1, 2, 3, 4, 5, 6, 7]
  assert [dc.mfma_group_chunks(K) for K in dc.MFMA_K_U8] == [1, 1, 1, 2, 3, 4, 5, 6, 7]
  assert all(K % 16 == 0 for K in dc.MFMA_K_U8 + dc.WIDE_K_U8)
  assert [dc.wide_chunks(K) for K in dc.WIDE_K_BITS] == [dc.wide_chunks(K) for K in dc.WIDE_K_U8] == [1, 1, 2, 3, 4, 5, 6, 7]

  for rt, ct in dc.WIDE_PLANS:
    for kind, in_types in (("bits", ("bits",)), ("u8", ("u8", "f32"))):
      cells = dc.wide_cells(rt, ct, kind)
      for it in in_types:
        lines.append("dense_wide_kernel<%d, %d, %s, false>: %d cells" % (rt, ct, it, len(cells)))
      assert {K for _, _, K, _ in cells} == set(dc.wide_k_list(kind))
      for T, B in dc.WIDE_ROWS[rt]:
        assert {K for t, b, K, N in cells if (t, b) == (T, B) and N <= 300} == set(dc.wide_k_list(kind))
      want_n = set(dc.WIDE_N[ct]) | (set(dc.WIDE_N_BLOCKS) if ct == 2 else set())
      assert {N for *_, N in cells} == want_n
      for N in dc.WIDE_N_BLOCKS if ct == 2 else ():
        assert len({K for *_, K, n in cells if n == N}) == 3
      assert all(dc.wide_ct(N) == ct for *_, N in cells)
      Ts = {T for T, _, _, _ in cells}
      assert 16 * rt in Ts and (Ts & {3, 5}) and (rt == 1 or 16 * (rt - 1) + 1 in Ts)
      monkeypatch.setenv(WIDE_KNOB, str(rt))
      for T, B, K, N in cells:
        sph = dc.wide_sph(rt, T)
        assert _wide(L, T, B, N) == (rt, ct, sph, 0)
        gx, gy = dc.wide_grid(rt, T, B, N)
        assert (gx == 9 and B == 16 * sph + 1) or (gx == 8 and B == 16 * sph)
        assert gy == (2 if N > 512 else 1)
      monkeypatch.delenv(WIDE_KNOB)
  assert {N for rt, ct in dc.WIDE_PLANS if rt == 1 for *_, N in dc.wide_cells(rt, ct, "bits")} == set(dc.WIDE_N_ALL)
  assert any(B == 16 * dc.wide_sph(2, T) for T, B, _, _ in dc.wide_cells(2, 1, "bits")), "the even-tailed batch"

  # the one-cell-per-plan tables
  assert {(c[0], c[1]) for c in dc.MFMA_BN_CELLS} == {(c[0], c[1]) for c in dc.MFMA_STRIDE_CELLS} == set(dc.MFMA_PLANS)
  assert {(c[0], c[1]) for c in dc.WIDE_BN_CELLS} == set(dc.WIDE_PLANS)
  assert {c[0] for c in dc.WIDE_STRIDE_CELLS} == {1, 2, 3, 4} and {c[1] for c in dc.WIDE_STRIDE_CELLS} == {1, 2}
  for in_type, rt, T, B, K, N in dc.MFMA_BN_CELLS + dc.MFMA_STRIDE_CELLS:
    assert 32 * rt >= T and K in dc.mfma_k_list(in_type) and (N <= 128 or T > 64)
  for rt, ct, kind, T, B, K, N in dc.WIDE_BN_CELLS:
    assert 16 * rt >= T and K in dc.wide_k_list(kind) and dc.wide_ct(N) == ct and (T, B) in dc.WIDE_ROWS[rt]
  for rt, ct, T, B, N in dc.WIDE_STRIDE_CELLS:
    assert dc.wide_ct(N) == ct and (T, B) in dc.WIDE_ROWS[rt]
  for form in dc.HEAD_CELLS:
    lines.append("dense_wide_kernel<1, %d, *, true> (csplit %d): 1 cell x 3 input types" % (form[1], form[2]))
  print("\n".join(lines))


def _band(o, T, B, K, N, data, names=("mslif", "silent")):
  for name in names:
    r = dc.expected(o, T, B, K, N, name, data)[2]
    if name == "silent":
      assert r == 0.0
    else:
      assert 0.005 <= r <= 0.6, (T, B, K, N, data, name, r)


@pytest.mark.parametrize("in_type,rt", dc.MFMA_PLANS)
def test_rate_band_of_the_128_column_cells(oracle, in_type, rt):
  for T, B, K, N in dc.mfma_cells(in_type, rt):
    _band(oracle, T, B, K, N, "binary")
    if in_type == "u8":
      _band(oracle, T, B, K, N, "counts")


@pytest.mark.parametrize("rt,ct", dc.WIDE_PLANS)
def test_rate_band_of_the_wide_cells(oracle, rt, ct):
  for T, B, K, N in dc.wide_cells(rt, ct, "bits"):
    _band(oracle, T, B, K, N, "binary", ("mslif", "silent", "no_state"))
  for T, B, K, N in dc.wide_cells(rt, ct, "u8"):
    _band(oracle, T, B, K, N, "binary", ("mslif",))
    _band(oracle, T, B, K, N, "counts", ("mslif", "silent", "no_state"))


def test_rate_band_of_the_other_cells(oracle):
  for in_type, rt, T, B, K, N in dc.MFMA_BN_CELLS:
    _band(oracle, T, B, K, N, "counts" if in_type == "u8" else "binary", ("bn_lif",))
  for rt, ct, kind, T, B, K, N in dc.WIDE_BN_CELLS:
    _band(oracle, T, B, K, N, "counts" if kind == "u8" else "binary", ("bn_lif", "no_state_bn"))
  for in_type, rt, T, B, K, N in dc.MFMA_STRIDE_CELLS:
    _band(oracle, T, B, K, N, "counts" if in_type == "u8" else "binary")
  for rt, ct, T, B, N in dc.WIDE_STRIDE_CELLS:
    _band(oracle, T, B, dc.WIDE_STRIDE_K["bits"], N, "binary")
    _band(oracle, T, B, dc.WIDE_STRIDE_K["u8"], N, "counts")
  for in_type, T, B, K, N in dc.SHIPPED_CELLS:
    _band(oracle, T, B, K, N, "counts" if in_type == "u8" else "binary", ("mslif",))
  for T, B, K, N1, N2 in list(dc.HEAD_CELLS.values()) + [(2 * dc.HEAD_STATE_CELL[0],) + dc.HEAD_STATE_CELL[1:]]:
    for data in ("binary", "counts"):
      e = dc.head_expected(oracle, T, B, K, N1, N2, data)
      assert 0.005 <= e["rate1"] <= 0.6 and 0.005 <= e["rate2"] <= 0.6, (T, B, K, N1, data, e["rate1"], e["rate2"])
