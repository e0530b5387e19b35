"""GPU suite: the two int8 dense kernels -- csrc/dense_mfma.hip (128 columns per workgroup) and
csrc/dense_wide.hip (256 or 512 columns, stand-alone and as the fused head) -- in every row-tile
plan at small K.

The launchers choose a handful of plans for the small batches of the rest of the suite; here
SNNQP_DENSE_MFMA_RT and SNNQP_DENSE_WIDE_RT force each plan over the table of
tests/dense_int8_plan_cases.py: every count of K chunks at which prologue, ring and unrolled body
meet dead chunks, row tiles filled exactly and with dead rows, nine workgroups along the batch (a
rotated K walk, a last workgroup of one sample), N with waves switched off and a second column
block.  Launches go through snnqp_dense_lif_forward / snnqp_dense_head_forward by ctypes with
IMPL_MFMA on buffers the test owns; before EVERY launch the plan query must report the plan the
case names.  Outputs are framed by guard words and pre-filled with a pattern the oracle never
produces.  Rasters and final potentials equal the oracle's bit for bit: exact integer sums, then
the oracle's own float32 steps -- no tolerances.

The leaves are 8-bit (tests/dense_int8_plan_cases.py): their packing carries no fp6 tiles, so no
launch here can be taken by csrc/dense_fp6.hip."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dense_int8_plan_cases as dc
from tests.helpers import packbits_lastaxis

pytestmark = pytest.mark.gpu
F32 = np.float32
MFMA_KNOB, WIDE_KNOB, NOSPLIT_KNOB = "SNNQP_DENSE_MFMA_RT", "SNNQP_DENSE_WIDE_RT", "SNNQP_DENSE_HEAD_NOSPLIT"
GUARD = 64                     # sentinel words on either side of an output
S_FILL, U_FILL, G_FILL = 0x5A5A5A5A, 0x7FC0BEEF, 0x3C3C3C3C
POISON = 0xA5                  # every byte of a workspace allocation before a launch


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()
  _lib.require_product_build()
  return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def context(dev, monkeypatch):
  """No knob set from outside, nothing reported by the device and no block handed to the
  direct-form kernel, before and after each test."""
  from snnquantprune_amd import ops
  for k in (MFMA_KNOB, WIDE_KNOB, NOSPLIT_KNOB):
    monkeypatch.delenv(k, raising=False)
  assert ops.device_status() == 0
  before = ops.fallback_counts()["dense_blocks"]
  yield
  torch.cuda.synchronize()
  assert ops.device_status() == 0
  assert ops.fallback_counts()["dense_blocks"] == before


def _pack(leaf, dev):
  """Product-side packing of an 8-bit leaf: int8 codes, int8 tiles, column sums, NO fp6 tiles."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  desc = QuantDesc(L.Q_DUQ, dc.BITS, a, c, float(2 ** (dc.BITS - 1) - 1), c)
  pk = packing.PackedKernel(torch.from_numpy(leaf["kernel"]).to(dev), desc,
                            torch.from_numpy(leaf["prune_0"]["mask"]).to(dev))
  N = leaf["kernel"].shape[-1]
  w = pk.int_weight_mfma((N + 31) // 32 * 32)
  assert w.wt6 is None and w.code_max > 7, "codes that fit fp6 would run the fp4 x fp6 kernel"
  assert w.wt is not None and w.col_sum is not None
  return w


@pytest.fixture(scope="module")
def weight_of(dev):
  cache = {}

  def get(K, N):
    if (K, N) not in cache:
      cache[(K, N)] = _pack(dc.leaf(K, N), dev)
    return cache[(K, N)]
  return get


def _t(a, dev):
  return torch.tensor(a).to(dev)            # (a copy: the case arrays are read-only)


def _fill(n, word, dev):
  return torch.full((n,), int(np.uint32(word).view(np.int32)), dtype=torch.int32, device=dev)


class Frame:
  """`n` 32-bit words of output between two runs of guard words, pre-filled with `word`."""

  def __init__(self, dev, n, word):
    self.n, self.word = n, word
    self.buf = torch.cat([_fill(GUARD, G_FILL, dev), _fill(n, word, dev), _fill(GUARD, G_FILL, dev)])
    self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

  def words(self):
    b = self.buf.cpu().numpy().view(np.uint32)
    assert (b[:GUARD] == G_FILL).all() and (b[GUARD + self.n:] == G_FILL).all(), "a guard word was written"
    return b[GUARD:GUARD + self.n]


class Workspace:
  """`nbytes` of workspace, 256-byte aligned, inside a larger allocation with every byte poisoned."""

  def __init__(self, dev, nbytes):
    lead, tail = 512, 4096
    self.raw = torch.full((lead + nbytes + tail + 512,), POISON, dtype=torch.uint8, device=dev)
    self.off = lead + (-(self.raw.data_ptr() + lead)) % 256
    self.nbytes = nbytes
    self.ptr = self.raw.data_ptr() + self.off

  def outside_is_poison(self):
    raw = self.raw.cpu().numpy()
    return bool((raw[:self.off] == POISON).all() and (raw[self.off + self.nbytes:] == POISON).all())

  def words(self, n):
    return self.raw[self.off:self.off + 4 * n].cpu().numpy().view(np.uint32)


def _rows(x, kind, layout, dev):
  """x uint8 [T, B, K] on the device as `kind` rows ("bits" spike words, "u8" bytes, "f32" float32
  holding the same integers) in `layout` -> (tensor, element strides t, b).  The padded layouts
  lengthen every row by elements nobody owns: 3 words of all ones for bit rows, 16 bytes of 0xFF for
  uint8 rows, 4 NaN (16 bytes) for float32 rows."""
  if kind == "bits":
    w = packbits_lastaxis(x)                                 # zero bits beyond K (snnqp.h)
    pad = np.full(w.shape[:2] + (3,), 0xFFFFFFFF, np.uint32)
  elif kind == "u8":
    w = np.ascontiguousarray(x)
    pad = np.full(w.shape[:2] + (16,), 0xFF, np.uint8)
  else:
    w = x.astype(F32)
    pad = np.full(w.shape[:2] + (4,), np.nan, F32)
  T, B = w.shape[:2]
  if layout.startswith("bm"):
    w, pad = np.swapaxes(w, 0, 1), np.swapaxes(pad, 0, 1)
  if layout.endswith("pad"):
    w = np.concatenate([w, pad], -1)
  w = np.ascontiguousarray(w)
  rs = w.shape[-1]
  xs_t, xs_b = (rs, T * rs) if layout.startswith("bm") else (B * rs, rs)
  if kind == "bits":
    w = w.view(np.int32)
  return torch.tensor(w).to(dev), xs_t, xs_b            # (a copy: the case arrays are read-only)


def _neuron(name, N, dev):
  """-> (ops.Neuron, ops.BnCoeffs or None, carried-in state?) of a neuron form of the case table."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  cfg, bn, state = dc.form(name, N)
  b = None
  if bn is not None:
    mul = ((F32(1) / np.sqrt(bn["var"] + F32(1e-5))) * bn["scale"]).astype(F32)
    b = ops.BnCoeffs(torch.from_numpy(bn["mean"]).to(dev), torch.from_numpy(mul).to(dev),
                     torch.from_numpy(bn["bias"]).to(dev))
  if cfg["kind"] == "LIF":
    sig = (1.0 / (1.0 + np.exp(-cfg["tau_vec"].astype(np.float64)))).astype(F32)
    return ops.Neuron(L.NEURON_LIF, 1.0, cfg["v_threshold"], cfg["v_reset"],
                      decay=torch.from_numpy(sig).to(dev)), b, state
  return ops.Neuron(L.NEURON_MULTI_STEP_LIF, cfg["tau"], cfg["v_threshold"], cfg["v_reset"]), b, state


def _in_type(kind):
  from snnquantprune_amd import _lib as L
  return {"bits": L.BITS, "u8": L.U8, "f32": L.F32}[kind]


def _launch(dev, w, kind, rows, T, B, K, N, u0d, name, flags=None, compare=True):
  """One snnqp_dense_lif_forward_ws with IMPL_MFMA on framed outputs -> (u [B, N] or None, spike
  words [T, B, CW]).  Guard words intact, every output word written, no spike bit at or beyond N.
  A form without state passes u0 and u_out as null."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  xd, xs_t, xs_b = rows
  CW = (N + 31) // 32
  nrn, bn, state = _neuron(name, N, dev)
  sf = Frame(dev, T * B * CW, S_FILL)
  uf = Frame(dev, B * N, U_FILL) if state else None
  w_, nrn_ = w.struct(), nrn.struct()
  bn_ = bn.struct() if bn is not None else None
  # IMPL_MFMA: a launch no MFMA kernel takes is refused, not handed to the direct-form kernel
  L.check(L.lib().snnqp_dense_lif_forward_ws(
      ctypes.c_void_p(xd.data_ptr()), _in_type(kind), xs_t, xs_b, T, B, K, N, ctypes.byref(w_),
      ctypes.c_void_p(w.wt.data_ptr()), None if bn_ is None else ctypes.byref(bn_), ctypes.byref(nrn_),
      ctypes.c_void_p(u0d.data_ptr()) if state else None, uf.ptr if state else None, sf.ptr, L.BITS,
      L.IMPL_MFMA, None if flags is None else ctypes.c_void_p(flags.data_ptr()), None, 0, ops._stream()))
  torch.cuda.synchronize()
  s = sf.words().reshape(T, B, CW)
  u = uf.words().view(F32).reshape(B, N) if state else None
  if compare:
    assert not (s == S_FILL).any(), "a raster word was not written"
    assert u is None or not (u.view(np.uint32) == U_FILL).any(), "a potential was not written"
    if N % 32:
      assert not (s[..., -1] >> np.uint32(N % 32)).any(), "spike bits at or beyond N"
  return u, s


def _check(got, exp, what):
  u, s = got
  eu, es, _ = exp
  np.testing.assert_array_equal(s, es, err_msg="raster: %s" % (what,))
  if u is not None:
    np.testing.assert_array_equal(u.view(np.uint32), eu.view(np.uint32), err_msg="u_T: %s" % (what,))


def _force_mfma(monkeypatch, in_type, rt, T, B, N):
  from snnquantprune_amd import ops
  monkeypatch.setenv(MFMA_KNOB, str(rt))
  assert ops.dense_mfma_plan(_in_type(in_type), T, B, N) == (rt, dc.mfma_sb(rt, T)) + dc.mfma_grid(rt, T, B, N), \
      "the launch would not take this plan"


def _force_wide(monkeypatch, rt, ct, T, B, N):
  from snnquantprune_amd import ops
  monkeypatch.setenv(WIDE_KNOB, str(rt))
  assert ops.dense_wide_plan(T, B, N, fused=False, may_split=False) == (rt, ct, dc.wide_sph(rt, T), 0), \
      "the launch would not take this plan"


def _flags(dev):
  return torch.full((1,), 0x55, dtype=torch.int32, device=dev)      # (the launch zeroes the word itself)


@pytest.mark.parametrize("in_type,rt", dc.MFMA_PLANS)
def test_128_column_kernel_every_plan_at_every_k_edge(dev, oracle, weight_of, monkeypatch, in_type, rt):
  """(input type, rt) x the row shapes of this rt x the K list: the default neuron, and a threshold
  nothing reaches (u_T then carries every current of every step).  uint8 rows: spikes and counts."""
  seen = set()
  for T, B, K, N in dc.mfma_cells(in_type, rt):
    w = weight_of(K, N)
    _force_mfma(monkeypatch, in_type, rt, T, B, N)
    for data in (("binary",) if in_type == "bits" else ("binary", "counts")):
      x, u0 = dc.inputs(T, B, K, N, data)
      rows = _rows(x, in_type, "tm", dev)
      u0d = _t(u0, dev)
      for name in ("mslif", "silent"):
        exp = dc.expected(oracle, T, B, K, N, name, data)
        print("%s rt %d T %d B %d K %d N %d %s %s: rate %.4f" % (in_type, rt, T, B, K, N, data, name, exp[2]))
        _check(_launch(dev, w, in_type, rows, T, B, K, N, u0d, name), exp,
               (in_type, rt, T, B, K, N, data, name, dc.mfma_group_chunks(K)))
    seen.add(K)
  assert seen == set(dc.mfma_k_list(in_type))


@pytest.mark.parametrize("rt,ct", dc.WIDE_PLANS)
def test_wide_kernel_every_plan_at_every_k_edge(dev, oracle, weight_of, monkeypatch, rt, ct):
  """(rt, ct) x the row shapes of this rt x the K lists: bit rows, uint8 rows (spikes and counts) and
  float32 rows holding the counts; the default neuron, the unreachable threshold, and the walk
  without state (u0 and u_out null).  After every float32 launch the flag word reads 0."""
  forms = ("mslif", "silent", "no_state")
  seen = set()
  for kind in ("bits", "u8"):
    for T, B, K, N in dc.wide_cells(rt, ct, kind):
      w = weight_of(K, N)
      _force_wide(monkeypatch, rt, ct, T, B, N)
      runs = [("bits", "binary", forms)] if kind == "bits" else \
          [("u8", "binary", ("mslif",)), ("u8", "counts", forms), ("f32", "counts", forms)]
      for row_kind, data, names in runs:
        x, u0 = dc.inputs(T, B, K, N, data)
        rows = _rows(x, row_kind, "tm", dev)
        u0d = _t(u0, dev)
        for name in names:
          exp = dc.expected(oracle, T, B, K, N, name, data)
          flags = _flags(dev) if row_kind == "f32" else None
          _check(_launch(dev, w, row_kind, rows, T, B, K, N, u0d, name, flags), exp,
                 (row_kind, rt, ct, T, B, K, N, data, name, dc.wide_chunks(K)))
          if flags is not None:
            assert int(flags.item()) == 0, (rt, ct, T, B, K, N, name)
      seen.add((kind, K))
  assert seen == {("bits", K) for K in dc.WIDE_K_BITS} | {("u8", K) for K in dc.WIDE_K_U8}


def test_batchnorm_and_lif_with_decay_on_every_plan(dev, oracle, weight_of, monkeypatch):
  """One cell per plan of both kernels with BatchNorm in front of the LIF neuron with per-feature
  decay; the wide kernel also without state behind BatchNorm."""
  for in_type, rt, T, B, K, N in dc.MFMA_BN_CELLS:
    data = "counts" if in_type == "u8" else "binary"
    x, u0 = dc.inputs(T, B, K, N, data)
    _force_mfma(monkeypatch, in_type, rt, T, B, N)
    _check(_launch(dev, weight_of(K, N), in_type, _rows(x, in_type, "tm", dev), T, B, K, N, _t(u0, dev), "bn_lif"),
           dc.expected(oracle, T, B, K, N, "bn_lif", data), (in_type, rt, T, B, K, N))
  monkeypatch.delenv(MFMA_KNOB)
  for rt, ct, kind, T, B, K, N in dc.WIDE_BN_CELLS:
    data = "counts" if kind == "u8" else "binary"
    x, u0 = dc.inputs(T, B, K, N, data)
    _force_wide(monkeypatch, rt, ct, T, B, N)
    for row_kind in (("bits",) if kind == "bits" else ("u8", "f32")):
      rows = _rows(x, row_kind, "tm", dev)
      for name in ("bn_lif", "no_state_bn"):
        flags = _flags(dev) if row_kind == "f32" else None
        _check(_launch(dev, weight_of(K, N), row_kind, rows, T, B, K, N, _t(u0, dev), name, flags),
               dc.expected(oracle, T, B, K, N, name, data), (row_kind, rt, ct, T, B, K, N, name))
        assert flags is None or int(flags.item()) == 0


@pytest.mark.parametrize("layout", ["tm_pad", "bm", "bm_pad"])
def test_rows_with_strides(dev, oracle, weight_of, monkeypatch, layout):
  """Time-major and batch-major rows, dense and with 16 bytes between rows that belong to nobody --
  all ones, 0xFF, NaN --: nothing outside a row may reach a sum, and float32 padding must not
  raise SNNQP_FLAG_NOT_INTEGER.  One plan per rt of both kernels at the raggedest K (the dense
  time-major layout is the one every other test here uses)."""
  for in_type, rt, T, B, K, N in dc.MFMA_STRIDE_CELLS:
    data = "counts" if in_type == "u8" else "binary"
    x, u0 = dc.inputs(T, B, K, N, data)
    rows = _rows(x, in_type, layout, dev)
    _force_mfma(monkeypatch, in_type, rt, T, B, N)
    for name in ("silent", "mslif"):
      _check(_launch(dev, weight_of(K, N), in_type, rows, T, B, K, N, _t(u0, dev), name),
             dc.expected(oracle, T, B, K, N, name, data), (layout, in_type, rt, T, B, K, N, name))
  monkeypatch.delenv(MFMA_KNOB)
  for rt, ct, T, B, N in dc.WIDE_STRIDE_CELLS:
    _force_wide(monkeypatch, rt, ct, T, B, N)
    for row_kind in ("bits", "u8", "f32"):
      K = dc.WIDE_STRIDE_K["bits" if row_kind == "bits" else "u8"]
      data = "binary" if row_kind == "bits" else "counts"
      x, u0 = dc.inputs(T, B, K, N, data)
      rows = _rows(x, row_kind, layout, dev)
      for name in ("silent", "mslif"):
        flags = _flags(dev) if row_kind == "f32" else None
        _check(_launch(dev, weight_of(K, N), row_kind, rows, T, B, K, N, _t(u0, dev), name, flags),
               dc.expected(oracle, T, B, K, N, name, data), (layout, row_kind, rt, ct, T, B, K, N, name))
        assert flags is None or int(flags.item()) == 0, "padding between rows reached the integer check"


def test_float32_rows_report_what_is_not_a_count(dev, weight_of, monkeypatch):
  """0.5, 256.0, -1.0 and NaN in turn at the last element of the last live row of the last workgroup
  (a workgroup of one sample): each raises SNNQP_FLAG_NOT_INTEGER; the rows without it do not."""
  from snnquantprune_amd import _lib as L
  rt, ct, T, B, N = dc.WIDE_STRIDE_CELLS[1]
  K = dc.WIDE_STRIDE_K["u8"]
  _force_wide(monkeypatch, rt, ct, T, B, N)
  x, u0 = dc.inputs(T, B, K, N, "counts")
  for bad in (None, 0.5, 256.0, -1.0, float("nan")):
    xf = x.astype(F32)
    if bad is not None:
      xf[T - 1, B - 1, K - 1] = bad
    flags = _flags(dev)
    rows = (torch.from_numpy(xf).to(dev), B * K, K)
    _launch(dev, weight_of(K, N), "f32", rows, T, B, K, N, _t(u0, dev), "mslif", flags, compare=False)
    assert int(flags.item()) == (0 if bad is None else L.FLAG_NOT_INTEGER), bad


# ---- the fused head at RT = 1 ------------------------------------------------------------------------

def _head(dev, kind, x, K, N1, N2, w1, w2, ws, state=None):
  """snnqp_dense_head_forward (state: (u1, u2, counts) device tensors -> the _state entry) on framed
  rasters and logits -> (s1 words, s2 words, logits)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  T, B = x.shape[:2]
  xd, xs_t, xs_b = _rows(x, kind, "tm", dev)
  CW1, CW2, NC = (N1 + 31) // 32, (N2 + 31) // 32, N2 // dc.HEAD_GROUP
  f1, f2, fl = Frame(dev, T * B * CW1, S_FILL), Frame(dev, T * B * CW2, S_FILL), Frame(dev, B * NC, U_FILL)
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0).struct()
  a, b = w1.struct(), w2.struct()
  flags = _flags(dev) if kind == "f32" else None
  carried = () if state is None else tuple(ctypes.c_void_p(t.data_ptr()) for t in state)
  entry = L.lib().snnqp_dense_head_forward if state is None else L.lib().snnqp_dense_head_forward_state
  L.check(entry(ctypes.c_void_p(xd.data_ptr()), _in_type(kind), xs_t, xs_b, T, B, K, N1, ctypes.byref(a),
                ctypes.c_void_p(w1.wt.data_ptr()), ctypes.byref(nrn), N2, ctypes.byref(b),
                ctypes.c_void_p(w2.wt.data_ptr()), ctypes.byref(nrn), dc.HEAD_GROUP, *carried, f1.ptr, f2.ptr, fl.ptr,
                None if flags is None else ctypes.c_void_p(flags.data_ptr()),
                None if ws is None else ctypes.c_void_p(ws.ptr), 0 if ws is None else ws.nbytes, ops._stream()))
  torch.cuda.synchronize()
  assert flags is None or int(flags.item()) == 0
  s1, s2, lg = f1.words().reshape(T, B, CW1), f2.words().reshape(T, B, CW2), fl.words()
  assert not (s1 == S_FILL).any() and not (s2 == S_FILL).any() and not (lg == U_FILL).any(), "an output word was not written"
  for s, n in ((s1, N1), (s2, N2)):
    assert n % 32 == 0 or not (s[..., -1] >> np.uint32(n % 32)).any(), "spike bits at or beyond N"
  return s1, s2, lg.view(F32).reshape(B, NC)


def _force_head(monkeypatch, dev, form, T, B, N1, how):
  """Sets the knobs for a fused form at RT = 1 -> the workspace the launch gets (or None).  The split
  form gets exactly snnqp_dense_head_workspace_bytes, asked after the knob is set; the unsplit
  two-column-tile form is reached by the no-split knob with a workspace at hand, or with none."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  monkeypatch.setenv(WIDE_KNOB, "1")
  monkeypatch.delenv(NOSPLIT_KNOB, raising=False)
  if how == "nosplit":
    monkeypatch.setenv(NOSPLIT_KNOB, "1")
  need = int(L.lib().snnqp_dense_head_workspace_bytes(T, B, N1))
  ws = None
  if form[2]:
    assert need == 4096 + dc.ceil_div(B, 2 * dc.wide_sph(1, T, True)) * 2 * 32 * 8 * 4
    ws = Workspace(dev, need)
  elif how == "nosplit":
    assert need == 0
    ws = Workspace(dev, 1 << 20)
  rt, ct, sph, cs = ops.dense_wide_plan(T, B, N1, fused=True, may_split=ws is not None)
  assert (rt, ct, cs) == form and sph == dc.wide_sph(1, T, True), "the launch would not take this form"
  return ws


@pytest.mark.parametrize("form,how", [((1, 1, 0), "ws"), ((1, 2, 0), "nosplit"), ((1, 2, 0), "no_ws"), ((1, 1, 1), "ws")],
                         ids=["ct1", "ct2_nosplit_knob", "ct2_no_workspace", "column_split"])
def test_fused_head_at_one_row_tile(dev, oracle, monkeypatch, form, how):
  """The fused head with ONE row tile, which no shape reaches by itself: one and two column tiles and
  the column split, on uint8 (counts), bit and float32 rows; both rasters and the logits equal
  oracle.dense2_forward.  The split hands over through a workspace of exactly the bytes the query
  names and leaves two arrivals in every tile's ticket."""
  T, B, K, N1, N2 = dc.HEAD_CELLS[form]
  l1, l2 = dc.head_leaves(K, N1, N2)
  w1, w2 = _pack(l1, dev), _pack(l2, dev)
  for kind, data in (("u8", "counts"), ("bits", "binary"), ("f32", "counts")):
    e = dc.head_expected(oracle, T, B, K, N1, N2, data)
    ws = _force_head(monkeypatch, dev, form, T, B, N1, how if form != (1, 1, 0) else "no_ws")
    s1, s2, lg = _head(dev, kind, dc.head_inputs(T, B, K, data), K, N1, N2, w1, w2, ws)
    np.testing.assert_array_equal(s1, e["s1"], err_msg=str((form, how, kind)))
    np.testing.assert_array_equal(s2, e["s2"], err_msg=str((form, how, kind)))
    np.testing.assert_array_equal(lg.view(np.uint32), e["logits"].view(np.uint32), err_msg=str((form, how, kind)))
    if ws is not None:
      assert ws.outside_is_poison()
    if form[2]:
      gx = dc.ceil_div(B, 2 * dc.wide_sph(1, T, True))
      assert (ws.words(gx) == 2).all(), "every tile's ticket counts its two workgroups"


def test_stateful_head_at_one_row_tile_over_two_windows(dev, oracle, monkeypatch):
  """snnqp_dense_head_forward_state at a forced RT = 1 form over two windows of T steps against one
  stateless window of 2 T: the rasters joined, the carried potentials and the counts."""
  form = dc.HEAD_STATE_FORM
  T, B, K, N1, N2 = dc.HEAD_STATE_CELL
  l1, l2 = dc.head_leaves(K, N1, N2)
  w1, w2 = _pack(l1, dev), _pack(l2, dev)
  for kind, data in (("u8", "counts"), ("bits", "binary")):
    x = dc.head_inputs(2 * T, B, K, data)
    e = dc.head_expected(oracle, 2 * T, B, K, N1, N2, data)
    ws = _force_head(monkeypatch, dev, form, 2 * T, B, N1, "ws")
    s1, s2, lg = _head(dev, kind, x, K, N1, N2, w1, w2, ws)
    np.testing.assert_array_equal(s1, e["s1"])
    np.testing.assert_array_equal(s2, e["s2"])
    np.testing.assert_array_equal(lg.view(np.uint32), e["logits"].view(np.uint32))
    state = (torch.zeros((B, N1), dtype=torch.float32, device=dev), torch.zeros((B, N2), dtype=torch.float32, device=dev),
             torch.zeros((B, N2), dtype=torch.int32, device=dev))
    ws = _force_head(monkeypatch, dev, form, T, B, N1, "ws")
    parts = [_head(dev, kind, np.ascontiguousarray(x[i * T:(i + 1) * T]), K, N1, N2, w1, w2, ws, state) for i in (0, 1)]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), s1, err_msg=kind)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), s2, err_msg=kind)
    np.testing.assert_array_equal(state[0].cpu().numpy().view(np.uint32), e["u1"].view(np.uint32))
    np.testing.assert_array_equal(state[1].cpu().numpy().view(np.uint32), e["u2"].view(np.uint32))
    np.testing.assert_array_equal(state[2].cpu().numpy(), e["counts"])


def test_plans_that_ship_without_the_knob(dev, oracle, weight_of):
  """The 128-column kernel as large batches run it: rt = 3 with four samples per workgroup on bit
  rows, rt = 2 with three on uint8 rows, the last workgroup holding one sample -- by the launcher's
  own rule, no knob set."""
  from snnquantprune_amd import ops
  for (in_type, T, B, K, N), (rt, sb) in dc.SHIPPED_CELLS.items():
    assert ops.dense_mfma_plan(_in_type(in_type), T, B, N) == (rt, sb, dc.ceil_div(B, sb), 1) and B % sb == 1
    data = "counts" if in_type == "u8" else "binary"
    x, u0 = dc.inputs(T, B, K, N, data)
    _check(_launch(dev, weight_of(K, N), in_type, _rows(x, in_type, "tm", dev), T, B, K, N, _t(u0, dev), "mslif"),
           dc.expected(oracle, T, B, K, N, "mslif", data), (in_type, T, B, K, N))
