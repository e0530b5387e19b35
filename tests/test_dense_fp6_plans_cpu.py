"""CPU suite: the launch plan of the fp4 x fp6 dense kernel (csrc/dense_fp6.hip) as
snnqp_dense_fp6_plan reports it -- the function the launch itself reads -- and the case table of
tests/fp6_plan_cases.py that the GPU file forces through SNNQP_DENSE_FP6_PLAN.

Properties of the plan, not the cost model restated: what a plan may be, when K may be split, what
the workspace and the knob may and may not change.  The query makes no GPU call and never
dereferences the workspace address, so the addresses below are made up."""
import ctypes
import itertools
import os
import sys

import pytest

from tests import fp6_plan_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "SNNQP_DENSE_FP6_PLAN"
WS = 1 << 24                  # a 256-byte aligned address that is never read
AMPLE = 1 << 40


@pytest.fixture(scope="module")
def L():
  from snnquantprune_amd import _lib
  if not os.path.exists(_lib.LIB_PATH):
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
  _lib.lib()
  return _lib


def _plan(L, T, B, K, N, ws=WS, ws_bytes=AMPLE, expect=0):
  v = [ctypes.c_int32(-99) for _ in range(4)]
  rc = L.lib().snnqp_dense_fp6_plan(T, B, K, N, None if ws is None else ctypes.c_void_p(ws), ws_bytes,
                                    *[ctypes.byref(x) for x in v])
  assert rc == expect, (rc, L.lib().snnqp_last_error())
  return tuple(x.value for x in v)


def _fp6_weight(L):
  # int8 codes known to fit fp6, with fp6 tiles: all a size query looks at (never dereferenced)
  return L.WeightT(L.W_I8, 8, 7.0, 1.0, 0, 7, None, 8)


# (T, B, K, N): the shipped read-out (C3: 32768 -> 110 at T = 20) over its batches, the split
# tests' shapes, every edge of the split rule (K = 8192, 8 chunks per split), T at the row-tile
# edges, batches that would exceed the ticket head when split, wide N
GRID = sorted(set(
    [(20, B, 32768, 110) for B in (1, 2, 16, 64, 100, 128, 256, 1024, 4096)] +
    [(7, 20, 32768, 200), (33, 9, 40000, 70), (20, 64, 8192, 110), (20, 64, 8191, 110), (20, 64, 16384, 110),
     (20, 64, 16383, 110), (20, 64, 16385, 110), (1, 1, 8192, 1), (160, 3, 65536, 33), (20, 5000, 32768, 110),
     (20, 1100, 32768, 2000), (3, 20000, 40000, 110), (96, 7, 2000000, 129)] +
    list(itertools.product((1, 7, 32, 33, 64, 65, 96, 97, 128, 129, 160), (1, 9, 300), (31, 2305, 8192, 32768),
                           (33, 160, 513)))))


def test_plan_properties_without_the_knob(L, monkeypatch):
  monkeypatch.delenv(KNOB, raising=False)
  w = _fp6_weight(L)
  split = 0
  for T, B, K, N in GRID:
    rt, ks, gx, gcz = _plan(L, T, B, K, N)
    assert 1 <= rt <= 5 and rt * 32 >= T, (T, B, K, N, rt)
    assert ks in (1, 2, 4)
    sb = rt * 32 // T
    assert gx == fc.ceil_div(B, sb)
    assert gcz == fc.gcz_of(K, ks)
    tiles = gx * fc.ceil_div(N, 128)
    if ks > 1:
      split += 1
      chunks = fc.ceil_div(fc.ceil_div(K, 64), 4)
      assert K >= 8192 and chunks >= 8 * ks, (T, B, K, N, ks)
      assert tiles <= fc.MAX_TILES, (T, B, K, N, tiles)
      # no workgroup of a planned split is left without work
      assert min(fc.ngc_per_z(K, ks)) >= 1
    need = int(L.lib().snnqp_dense_workspace_bytes(L.BITS, T, B, K, N, ctypes.byref(w)))
    assert need == fc.workspace_bytes(rt, ks, T, B, N), (T, B, K, N, rt, ks)
    assert (need == 0) == (ks == 1)
    # exactly that much is enough; one byte less, a misaligned or a null workspace: no split
    assert _plan(L, T, B, K, N, WS, need) == (rt, ks, gx, gcz)
    unsplit = _plan(L, T, B, K, N, None, 0)
    assert unsplit[1] == 1 and unsplit[3] == 0 and unsplit[0] * 32 >= T
    assert _plan(L, T, B, K, N, None, AMPLE) == unsplit
    if ks > 1:
      assert _plan(L, T, B, K, N, WS, need - 1) == unsplit
      assert _plan(L, T, B, K, N, WS + 128, AMPLE) == unsplit
  assert split >= 8, "the grid is meant to reach split plans"
  # the read-out at the batches the split was made for, and the headline batch unsplit
  assert _plan(L, 20, 64, 32768, 110)[1] > 1
  assert _plan(L, 20, 1024, 32768, 110)[1] == 1


def test_the_query_refuses_what_the_launch_refuses(L, monkeypatch):
  monkeypatch.delenv(KNOB, raising=False)
  assert _plan(L, 160, 4, 513, 33)[0] == 5
  _plan(L, 161, 4, 513, 33, expect=L.EUNSUPPORTED)
  assert b"T too large" in L.lib().snnqp_last_error()
  for bad in ((0, 4, 513, 33), (20, 0, 513, 33), (20, 4, 0, 33), (20, 4, 513, 0), (-1, 4, 513, 33)):
    _plan(L, *bad, expect=L.EINVAL)
  i32 = ctypes.c_int32
  a, b, c = i32(), i32(), i32()
  assert L.lib().snnqp_dense_fp6_plan(20, 4, 513, 33, None, 0, None, ctypes.byref(a), ctypes.byref(b),
                                      ctypes.byref(c)) == L.EINVAL
  assert L.lib().snnqp_dense_fp6_plan(20, 4, 513, 33, None, 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                      None) == L.EINVAL


def test_the_knob_is_honoured_when_well_formed_and_usable(L, monkeypatch):
  for T, B, K, N in ((7, 33, 2305, 160), (20, 64, 32768, 110), (32, 9, 31, 33), (160, 9, 513, 129)):
    monkeypatch.delenv(KNOB, raising=False)
    free = _plan(L, T, B, K, N)
    unsplit = _plan(L, T, B, K, N, None, 0)
    for rt, ks in itertools.product(fc.RT_LIST, fc.KS_LIST):
      monkeypatch.setenv(KNOB, "%d,%d" % (rt, ks))
      got = _plan(L, T, B, K, N)
      if rt * 32 < T:
        assert got == free, "an rt too small for T is ignored"
        continue
      gx, _ = fc.grid(rt, T, B, N)
      assert got == (rt, ks, gx, fc.gcz_of(K, ks)), (T, B, K, N, rt, ks, got)
      need = fc.workspace_bytes(rt, ks, T, B, N)
      assert _plan(L, T, B, K, N, WS, max(need, 1)) == got
      # no workspace: the knob is not read; too little of it or a misaligned one: the answer
      # without the knob and without a workspace
      assert _plan(L, T, B, K, N, None, 0) == unsplit
      if ks > 1:
        assert _plan(L, T, B, K, N, WS, need - 1) == unsplit
        assert _plan(L, T, B, K, N, WS, 0) == unsplit
        assert _plan(L, T, B, K, N, WS + 128, AMPLE) == unsplit


@pytest.mark.parametrize("value", ["0,2", "6,1", "2,3", "x", "", "2", "2;4", "-1,2", "2,0", "2,8"])
def test_a_malformed_knob_is_ignored(L, monkeypatch, value):
  for T, B, K, N in ((7, 33, 2305, 160), (20, 64, 32768, 110)):
    monkeypatch.delenv(KNOB, raising=False)
    free = _plan(L, T, B, K, N)
    monkeypatch.setenv(KNOB, value)
    assert _plan(L, T, B, K, N) == free


def test_a_forced_split_of_more_tiles_than_tickets_is_dropped(L, monkeypatch):
  rt, ks, T, B, K, N = fc.TICKET_GUARD_CELL
  gx, gy = fc.grid(rt, T, B, N)
  assert gx * gy > fc.MAX_TILES
  monkeypatch.delenv(KNOB, raising=False)
  free = _plan(L, T, B, K, N)
  monkeypatch.setenv(KNOB, "%d,%d" % (rt, ks))
  got = _plan(L, T, B, K, N)
  assert got[1] == 1 or got[2] * gy <= fc.MAX_TILES, got
  assert got == free
  # one sample fewer along the batch fits the head: honoured; unsplit, the knob has no tile limit
  gx1, _ = fc.grid(rt, T, B - 1, N)
  assert _plan(L, T, B - 1, K, N) == (rt, ks, gx1, fc.gcz_of(K, ks))
  monkeypatch.setenv(KNOB, "%d,1" % rt)
  assert _plan(L, T, B, K, N) == (rt, 1, gx, 0)
  # two column blocks halve the batch that fits
  monkeypatch.setenv(KNOB, "1,4")
  assert _plan(L, 32, 512, 513, 160)[:2] == (1, 4)
  assert _plan(L, 32, 513, 513, 160)[1] == 1


def test_the_case_table_reaches_every_plan_and_chunk_count(L, monkeypatch):
  cells = fc.plan_cells()
  assert {(c[0], c[1]) for c in cells} == set(itertools.product(fc.RT_LIST, fc.KS_LIST))
  counts, raw_negative = set(), False
  for rt in fc.RT_LIST:
    mine = [c for c in cells if c[0] == rt]
    sbs = {fc.sb_of(rt, T) for _, _, T, _, _, _ in mine}
    assert 1 in sbs and max(sbs) > 1, (rt, sbs)
    assert any(T == 32 * rt for _, _, T, _, _, _ in mine), "full row tiles"
    assert {N for *_, N in mine} == set(fc.N_LIST)
    assert {K for _, _, _, _, K, _ in mine} == set(fc.K_LIST)
  for rt, ks, T, B, K, N in cells + [fc.TICKET_GUARD_CELL] + list(fc.BN_LIF_CELLS) + list(fc.INT8_CELLS):
    assert rt * 32 >= T
    sb = fc.sb_of(rt, T)
    gx, gy = fc.grid(rt, T, B, N)
    assert gx >= 9, "every value of blockIdx.x & 7"
    if sb > 1:
      assert B % sb != 0, "the last workgroup is partly filled"
    counts.update(fc.ngc_per_z(K, ks))
    raw_negative |= ks > 1 and fc.ngc_raw_last(K, ks) < 0
    # the plan each cell names is the plan a launch with its workspace takes
    if (rt, ks, T, B, K, N) != fc.TICKET_GUARD_CELL:
      monkeypatch.setenv(KNOB, "%d,%d" % (rt, ks))
      need = fc.workspace_bytes(rt, ks, T, B, N)
      assert _plan(L, T, B, K, N, WS, max(need, 256)) == (rt, ks, gx, fc.gcz_of(K, ks))
  assert counts == {0, 1, 2, 3, 4, 5}
  assert raw_negative, "the clamp of a workgroup beyond the end of K"
  assert fc.ngc_per_z(2305, 4) == [2, 2, 1, 0] and fc.ngc_raw_last(2305, 4) == -1
  assert fc.ngc_per_z(2305, 2) == [3, 2]
  assert [fc.ngc_all(K) for K in fc.K_LIST] == [1, 1, 1, 1, 2, 3, 4, 5]
  assert all(c[2] <= 96 for c in fc.INT8_CELLS), "the int8 kernel serves T <= 96"
  assert {c[0] for c in fc.INT8_CELLS} == {c[0] for c in fc.BN_LIF_CELLS} == set(fc.RT_LIST)
