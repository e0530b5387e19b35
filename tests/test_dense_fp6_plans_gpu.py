"""GPU suite: the fp4 x fp6 dense kernel (csrc/dense_fp6.hip) in every row-tile and K-split plan at
small K.

The launcher's cost model splits K only from K = 8192 on, so the rest of the suite reaches a handful
of (rt, ks) pairs at K = 32768.  Here SNNQP_DENSE_FP6_PLAN forces each of the 15 plans at K of 31 to
2305 (tests/fp6_plan_cases.py: the chunk counts 0..5 a workgroup can be left with, rotated K walks,
dead chunks, workgroups beyond the end of K), through snnqp_dense_lif_forward_ws on buffers the test
owns.  Before EVERY launch snnqp_dense_fp6_plan is asked with the same workspace and must report the
plan the case names: a case whose plan is not the one run is an error, not a pass.  Rasters and final
potentials equal the oracle's (exact integer sums, carried-in u0) bit for bit.

Contract of the input that is NOT tested against: include/snnqp.h requires zero bits beyond K in the
last spike word of a row ("SNNQP_BITS input (zero bits beyond K)"), so every row here has them zero.
Words BETWEEN rows (a row stride above ceil(K / 32)) belong to nobody and are all ones here."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from tests import fp6_plan_cases as fc
from tests.helpers import packbits_lastaxis

pytestmark = pytest.mark.gpu
F32 = np.float32
KNOB = "SNNQP_DENSE_FP6_PLAN"
GUARD = 64                     # sentinel words on either side of an output
S_FILL, U_FILL, G_FILL = 0x5A5A5A5A, 0x7FC0BEEF, 0x3C3C3C3C
POISON = 0xA5                  # every byte of a workspace allocation before a launch
POISON_WORD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()
  _lib.require_product_build()
  return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weight_of(dev):
  """(K, N) -> product-side packing of the case's leaf: int8 codes, int8 tiles and fp6 tiles."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  cache = {}

  def get(K, N):
    if (K, N) not in cache:
      leaf = fc.leaf(K, N)
      a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
      desc = QuantDesc(L.Q_DUQ, fc.BITS, a, c, float(2 ** (fc.BITS - 1) - 1), c)
      pk = packing.PackedKernel(torch.from_numpy(leaf["kernel"]).to(dev), desc,
                                torch.from_numpy(leaf["prune_0"]["mask"]).to(dev))
      w = pk.int_weight_mfma((N + 31) // 32 * 32)
      assert w.wt6 is not None and 0 < w.code_max <= 7
      cache[(K, N)] = w
    return cache[(K, N)]
  return get


def _t(a, dev):
  return torch.tensor(a).to(dev)            # (a copy: the case arrays are read-only)


def _i32(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def _fill(n, word, dev):
  return torch.full((n,), int(np.uint32(word).view(np.int32)), dtype=torch.int32, device=dev)


class Workspace:
  """`nbytes` of workspace inside a larger allocation, every byte of it poisoned; `shift` moves the
  256-byte aligned start."""

  def __init__(self, dev, nbytes, shift=0):
    lead, tail = 512, 4096
    self.raw = torch.full((lead + nbytes + tail + 512,), POISON, dtype=torch.uint8, device=dev)
    self.off = lead + (-(self.raw.data_ptr() + lead)) % 256 + shift
    self.nbytes = nbytes
    self.ptr = self.raw.data_ptr() + self.off

  def poison(self):
    self.raw.fill_(POISON)

  def outside_is_poison(self):
    raw = self.raw.cpu().numpy()
    return bool((raw[:self.off] == POISON).all() and (raw[self.off + self.nbytes:] == POISON).all())

  def words(self, n):
    return self.raw[self.off:self.off + 4 * n].cpu().numpy().view(np.uint32)

  def untouched(self):
    return bool((self.raw.cpu().numpy() == POISON).all())


def _rows(x, layout, dev):
  """Spike words of x [T, B, K] on the device in `layout` -> (tensor, word strides t, b).  The
  padded layouts give a row KW + 3 words, the three beyond the row all ones."""
  w = packbits_lastaxis(x)                                   # [T, B, KW], zero bits beyond K
  T, B, KW = w.shape
  if layout.startswith("bm"):
    w = np.swapaxes(w, 0, 1)
  if layout.endswith("pad"):
    w = np.concatenate([w, np.full(w.shape[:2] + (3,), 0xFFFFFFFF, np.uint32)], -1)
  rs = w.shape[-1]
  xs_t, xs_b = (rs, T * rs) if layout.startswith("bm") else (B * rs, rs)
  return _i32(w, dev), xs_t, xs_b


def _neuron(name, N, dev):
  """-> (ops.Neuron, ops.BnCoeffs or None) of a neuron form of fp6_plan_cases."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  cfg, bn = fc.form(name, N)
  b = None
  if bn is not None:
    mul = ((F32(1) / np.sqrt(bn["var"] + F32(1e-5))) * bn["scale"]).astype(F32)
    b = ops.BnCoeffs(torch.from_numpy(bn["mean"]).to(dev), torch.from_numpy(mul).to(dev),
                     torch.from_numpy(bn["bias"]).to(dev))
  if cfg["kind"] == "LIF":
    sig = (1.0 / (1.0 + np.exp(-cfg["tau_vec"].astype(np.float64)))).astype(F32)
    return ops.Neuron(L.NEURON_LIF, 1.0, cfg["v_threshold"], cfg["v_reset"],
                      decay=torch.from_numpy(sig).to(dev)), b
  return ops.Neuron(L.NEURON_MULTI_STEP_LIF, cfg["tau"], cfg["v_threshold"], cfg["v_reset"]), b


def _query(T, B, K, N, ws):
  from snnquantprune_amd import ops
  return ops.dense_fp6_plan(T, B, K, N, None if ws is None else ws.ptr, 0 if ws is None else ws.nbytes)


def _launch(dev, w, xd, xs_t, xs_b, T, B, K, N, u0d, name, ws):
  """One snnqp_dense_lif_forward_ws on framed outputs -> (u [B, N], spike words [T, B, CW]).  Guard
  words around both outputs must come back intact, every output word written, no spike bit at or
  beyond N."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  CW = (N + 31) // 32
  nrn, bn = _neuron(name, N, dev)
  ns, nu = T * B * CW, B * N
  sbuf = torch.cat([_fill(GUARD, G_FILL, dev), _fill(ns, S_FILL, dev), _fill(GUARD, G_FILL, dev)])
  ubuf = torch.cat([_fill(GUARD, G_FILL, dev), _fill(nu, U_FILL, dev), _fill(GUARD, G_FILL, dev)])
  ws_ = w.struct()
  nrn_, bn_ = nrn.struct(), (bn.struct() if bn is not None else None)
  # IMPL_MFMA without int8 tiles: a launch the fp6 kernel did not take is refused, not rerouted
  L.check(L.lib().snnqp_dense_lif_forward_ws(
      ctypes.c_void_p(xd.data_ptr()), L.BITS, xs_t, xs_b, T, B, K, N, ctypes.byref(ws_), None,
      None if bn_ is None else ctypes.byref(bn_), ctypes.byref(nrn_), ctypes.c_void_p(u0d.data_ptr()),
      ctypes.c_void_p(ubuf.data_ptr() + 4 * GUARD), ctypes.c_void_p(sbuf.data_ptr() + 4 * GUARD), L.BITS,
      L.IMPL_MFMA, None, None if ws is None else ctypes.c_void_p(ws.ptr), 0 if ws is None else ws.nbytes,
      ops._stream()))
  torch.cuda.synchronize()
  s = sbuf.cpu().numpy().view(np.uint32)
  u = ubuf.cpu().numpy().view(np.uint32)
  for buf, n in ((s, ns), (u, nu)):
    assert (buf[:GUARD] == G_FILL).all() and (buf[GUARD + n:] == G_FILL).all(), "a guard word was written"
  s = s[GUARD:GUARD + ns].reshape(T, B, CW)
  if N % 32:
    assert not (s[..., -1] >> np.uint32(N % 32)).any(), "spike bits at or beyond N"
  return u[GUARD:GUARD + nu].view(F32).reshape(B, N), s


def _check(got, exp, what):
  u, s = got
  eu, es, _ = exp
  np.testing.assert_array_equal(s, es, err_msg="raster: %s" % (what,))
  np.testing.assert_array_equal(u.view(np.uint32), eu.view(np.uint32), err_msg="u_T: %s" % (what,))


def _forced(monkeypatch, dev, rt, ks, T, B, K, N, ws=None):
  """Sets the knob, makes (or takes) the workspace of exactly the bytes the plan needs and asserts
  that the query reports the plan -> the workspace."""
  monkeypatch.setenv(KNOB, "%d,%d" % (rt, ks))
  if ws is None:
    # (an unsplit plan needs none, but the knob is only read when a workspace is given)
    ws = Workspace(dev, max(fc.workspace_bytes(rt, ks, T, B, N), 256))
  gx, _ = fc.grid(rt, T, B, N)
  assert _query(T, B, K, N, ws) == (rt, ks, gx, fc.gcz_of(K, ks)), "the launch would not take this plan"
  return ws


def _tickets_ok(ws, rt, ks, T, B, N):
  """After a launch: tickets [0, tiles) count ks arrivals, the rest of the head and everything
  outside the workspace still hold the poison."""
  if ks == 1:
    return ws.untouched()
  gx, gy = fc.grid(rt, T, B, N)
  head = ws.words(fc.MAX_TILES)
  return bool((head[:gx * gy] == ks).all() and (head[gx * gy:] == POISON_WORD).all() and ws.outside_is_poison())


@pytest.mark.parametrize("rt", fc.RT_LIST)
def test_every_plan_at_every_k_edge(dev, oracle, weight_of, monkeypatch, rt):
  """rt x ks in {1, 2, 4} x the K list x the row shapes of this rt: the default neuron, and a
  threshold nothing reaches (u_T then carries every current of every step)."""
  from snnquantprune_amd import ops
  assert ops.device_status() == 0
  seen = set()
  for _, T, B, K, N in [c for c in fc.row_cases() if c[0] == rt]:
    x, u0 = fc.inputs(T, B, K, N)
    xd, xs_t, xs_b = _rows(x, "tm", dev)
    u0d = _t(u0, dev)
    w = weight_of(K, N)
    exp = {name: fc.expected(oracle, T, B, K, N, name) for name in ("mslif", "silent")}
    assert 0.005 < exp["mslif"][2] < 0.6, exp["mslif"][2]
    assert exp["silent"][2] == 0.0
    for ks in fc.KS_LIST:
      ws = _forced(monkeypatch, dev, rt, ks, T, B, K, N)
      for name in ("mslif", "silent"):
        ws.poison()
        _check(_launch(dev, w, xd, xs_t, xs_b, T, B, K, N, u0d, name, ws), exp[name],
               (rt, ks, T, B, K, N, name, fc.ngc_per_z(K, ks)))
        assert _tickets_ok(ws, rt, ks, T, B, N), (rt, ks, T, B, K, N)
      seen.add((ks, K))
  assert seen == {(ks, K) for ks in fc.KS_LIST for K in fc.K_LIST}
  assert ops.device_status() == 0


def test_batchnorm_and_lif_with_decay_on_one_plan_per_rt(dev, oracle, weight_of, monkeypatch):
  from snnquantprune_amd import ops
  for rt, ks, T, B, K, N in fc.BN_LIF_CELLS:
    x, u0 = fc.inputs(T, B, K, N)
    xd, xs_t, xs_b = _rows(x, "tm", dev)
    exp = fc.expected(oracle, T, B, K, N, "bn_lif")
    assert 0.005 < exp[2] < 0.6, exp[2]
    ws = _forced(monkeypatch, dev, rt, ks, T, B, K, N)
    _check(_launch(dev, weight_of(K, N), xd, xs_t, xs_b, T, B, K, N, _t(u0, dev), "bn_lif", ws),
           exp, (rt, ks, T, B, K, N))
  assert ops.device_status() == 0


@pytest.mark.parametrize("layout", ["tm_pad", "bm", "bm_pad"])
def test_rows_with_strides(dev, oracle, weight_of, monkeypatch, layout):
  """Time-major and batch-major rows, dense and with a row stride of KW + 3 words whose padding is
  all ones: no word outside a row may reach a sum.  One split plan per rt at the ragged K edges (the
  dense time-major layout is the one every other test here uses)."""
  for rt, T, B in [(rt, *fc.ROWS[rt][0]) for rt in fc.RT_LIST] + [(2, 33, 9), (5, 160, 9)]:
    for K, N, ks in ((65, 33, 2), (2305, 160, 4)):
      x, u0 = fc.inputs(T, B, K, N)
      xd, xs_t, xs_b = _rows(x, layout, dev)
      exp = fc.expected(oracle, T, B, K, N, "silent")
      ws = _forced(monkeypatch, dev, rt, ks, T, B, K, N)
      _check(_launch(dev, weight_of(K, N), xd, xs_t, xs_b, T, B, K, N, _t(u0, dev), "silent", ws),
             exp, (layout, rt, ks, T, B, K, N))
      exp = fc.expected(oracle, T, B, K, N, "mslif")
      _check(_launch(dev, weight_of(K, N), xd, xs_t, xs_b, T, B, K, N, _t(u0, dev), "mslif", ws),
             exp, (layout, rt, ks, T, B, K, N))


def test_outputs_inside_sentinel_frames(dev, oracle, weight_of, monkeypatch):
  """Every launch of this file runs on framed outputs (_launch); here each N of the table -- a wave
  switched off inside a column block, a second block, a ragged last word -- with partly filled last
  workgroups, split and unsplit: guards intact, every word of both outputs written (the body is
  pre-filled with a pattern the oracle never produces), no bit at or beyond N."""
  for (rt, T, B), N in zip(((1, 7, 33), (2, 7, 73), (4, 20, 49), (5, 20, 65)), fc.N_LIST):
    for ks, K in ((1, 257), (4, 513)):
      x, u0 = fc.inputs(T, B, K, N)
      xd, xs_t, xs_b = _rows(x, "tm", dev)
      ws = _forced(monkeypatch, dev, rt, ks, T, B, K, N)
      u, s = _launch(dev, weight_of(K, N), xd, xs_t, xs_b, T, B, K, N, _t(u0, dev), "mslif", ws)
      assert not (u.view(np.uint32) == U_FILL).any() and not np.isnan(u).any()
      _check((u, s), fc.expected(oracle, T, B, K, N, "mslif"), (rt, ks, T, B, K, N))


@pytest.mark.parametrize("rt", fc.RT_LIST)
def test_the_workspace_as_a_contract(dev, oracle, weight_of, monkeypatch, rt):
  """Exactly the bytes the header's formula gives, inside a larger poisoned allocation, tickets and
  slabs pre-filled with garbage (the launch zeroes its own tickets): twice in a row on the same
  workspace the oracle's results, tickets [0, tiles) == ks, the rest of the ticket head and every
  byte outside still poison, nothing reported.  One byte less, or a start misaligned by 128 bytes:
  the query reports the unsplit plan, the launch leaves the workspace alone and still matches."""
  from snnquantprune_amd import ops
  assert ops.device_status() == 0
  T, B = fc.ROWS[rt][0]
  K, N = 2305, 160
  x, u0 = fc.inputs(T, B, K, N)
  xd, xs_t, xs_b = _rows(x, "tm", dev)
  u0d = _t(u0, dev)
  w = weight_of(K, N)
  exp = fc.expected(oracle, T, B, K, N, "mslif")
  monkeypatch.delenv(KNOB, raising=False)
  unsplit = _query(T, B, K, N, None)
  assert unsplit[1] == 1 and unsplit[3] == 0
  for ks in (2, 4):
    need = fc.workspace_bytes(rt, ks, T, B, N)
    ws = _forced(monkeypatch, dev, rt, ks, T, B, K, N)
    assert ws.nbytes == need and ws.ptr % 256 == 0
    for rep in range(2):                       # (the second launch meets the first one's tickets and slabs)
      if rep == 0:
        ws.poison()
      _check(_launch(dev, w, xd, xs_t, xs_b, T, B, K, N, u0d, "mslif", ws), exp, (rt, ks, "rep", rep))
      assert _tickets_ok(ws, rt, ks, T, B, N), (rt, ks, rep)
      assert ops.device_status() == 0
    for small in (Workspace(dev, need - 1), Workspace(dev, need, shift=128)):
      assert _query(T, B, K, N, small) == unsplit
      _check(_launch(dev, w, xd, xs_t, xs_b, T, B, K, N, u0d, "mslif", small), exp, (rt, ks, "unusable"))
      assert small.untouched()
  assert ops.device_status() == 0


def test_a_forced_split_cannot_overrun_the_ticket_head(dev, oracle, weight_of, monkeypatch):
  """1025 tiles, forced to split: the ticket head has 1024 words, ticket 1024 would be the first
  word of the first slab.  The shared plan function drops such a forced plan like the planner
  does, and the launch is the oracle's."""
  from snnquantprune_amd import ops
  rt, ks, T, B, K, N = fc.TICKET_GUARD_CELL
  gx, gy = fc.grid(rt, T, B, N)
  assert gx * gy > fc.MAX_TILES
  x, u0 = fc.inputs(T, B, K, N)
  xd, xs_t, xs_b = _rows(x, "tm", dev)
  ws = Workspace(dev, fc.workspace_bytes(rt, ks, T, B, N))
  monkeypatch.setenv(KNOB, "%d,%d" % (rt, ks))
  prt, pks, pgx, _ = _query(T, B, K, N, ws)
  assert pks == 1 or pgx * gy <= fc.MAX_TILES, (prt, pks, pgx)
  exp = fc.expected(oracle, T, B, K, N, "mslif")
  assert 0.005 < exp[2] < 0.6
  _check(_launch(dev, weight_of(K, N), xd, xs_t, xs_b, T, B, K, N, _t(u0, dev), "mslif", ws),
         exp, "ticket guard")
  assert ws.outside_is_poison()
  assert ops.device_status() == 0


def test_forced_plans_agree_with_the_int8_formulation(dev, oracle, weight_of, monkeypatch):
  """The one comparison with another kernel: the same codes with the fp6 tiles withheld run on the
  int8 MFMA kernel (dense_mfma.hip, T <= 96); one forced plan per rt must give its bits, as
  test_dense_block_fp6_mfma ties the two routes together at the planner's own plans."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  for rt, ks, T, B, K, N in fc.INT8_CELLS:
    x, u0 = fc.inputs(T, B, K, N)
    xd, xs_t, xs_b = _rows(x, "tm", dev)
    u0d = _t(u0, dev)
    w = weight_of(K, N)
    ws = _forced(monkeypatch, dev, rt, ks, T, B, K, N)
    u, s = _launch(dev, w, xd, xs_t, xs_b, T, B, K, N, u0d, "mslif", ws)
    _check((u, s), fc.expected(oracle, T, B, K, N, "mslif"), (rt, ks, T, B, K, N))
    w8 = dataclasses.replace(w, wt6=None)
    assert w8.wt is not None
    nrn, _ = _neuron("mslif", N, dev)
    u8, s8 = ops.dense_lif_forward(ops.pack_bits(_t(x, dev)), w8, K, N, nrn, u0=u0d,
                                   packed_out=True, impl=L.IMPL_MFMA)
    np.testing.assert_array_equal(s8.bits.cpu().numpy().view(np.uint32), s)
    np.testing.assert_array_equal(u8.cpu().numpy().view(np.uint32), u.view(np.uint32))
