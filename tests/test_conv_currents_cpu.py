"""CPU checks around the currents form of the bit-input MFMA conv: the cases of
tests/currents_cases.py are what they claim to be, snnqp_conv_forward_ex refuses on the host what
its kernel cannot serve (no launch is reached without a GPU), and the Python switch and routing."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import currents_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
  from snnquantprune_amd import _lib as L
  if not os.path.exists(L.LIB_PATH):
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
  return L


# ---- the cases ---------------------------------------------------------------------------------

@pytest.mark.parametrize("c", cc.CASES, ids=cc.IDS)
def test_oracle_accumulators_equal_float64_conv2d(c):
  e = cc.expected(c)
  x = torch.from_numpy(e["x"].astype(np.float64)).permute(0, 3, 1, 2)
  w = torch.from_numpy(np.asarray(e["qw"].q, np.float64)).permute(3, 2, 0, 1)
  ref = torch.nn.functional.conv2d(x, w, padding=1).permute(0, 2, 3, 1).numpy()
  assert ref.shape == e["acc"].shape == (c["NB"], c["H"], c["W"], c["cout"])
  np.testing.assert_array_equal(e["acc"].astype(np.float64), ref)
  assert e["y"].dtype == np.float32 and e["y"].shape == e["acc"].shape
  # the codes are what the instruction of the case holds
  cmax = int(np.abs(e["qw"].q).max())
  assert (cmax <= 7) == cc.fp6(c) and cmax <= 127
  assert (float(e["qw"].L) == 1.0) == (c["quant"] == "q2")


@pytest.mark.parametrize("c", cc.CASES, ids=cc.IDS)
def test_cases_exercise_the_accumulator(c):
  """Every case but the all-zero raster has accumulators of both signs and more than half of them
  non-zero."""
  acc = cc.expected(c)["acc"]
  if c["raster"] == "zeros":
    assert not acc.any()
    return
  assert acc.min() < 0 < acc.max(), (acc.min(), acc.max())
  assert np.count_nonzero(acc) > acc.size / 2, (np.count_nonzero(acc), acc.size)


def test_cases_reach_the_accumulator_ranges():
  big = {True: 0, False: 0}
  zeros = 0
  for c in cc.CASES:
    acc = cc.expected(c)["acc"]
    big[cc.fp6(c)] = max(big[cc.fp6(c)], int(np.abs(acc).max()))
    if c["raster"] != "zeros" and (acc == 0).any():
      zeros += 1
  print("largest |acc|: fp6 %d, int8 %d; cases with exact zeros among non-zeros: %d" % (big[True], big[False], zeros))
  assert big[True] > 2047          # beyond the fused kernel's dequantisation table
  assert big[False] > 32767        # beyond 16 bits
  assert zeros >= 1


def test_grid_touches_every_value_once_per_instruction():
  for fp6 in (True, False):
    g = [c for c in cc.GRID if cc.fp6(c) == fp6]
    assert {c["cin"] for c in g} == {1, 16, 17, 32, 33, 48, 64, 79, 96, 100, 128}
    assert {c["cout"] for c in g} == {1, 31, 32, 33, 128, 129, 160}
    assert {(c["H"], c["W"]) for c in g} == {(1, 1), (3, 5), (4, 8), (5, 9), (13, 17)}
    assert {c["NB"] for c in g} == {1, 3}
  assert {c["quant"] for c in cc.GRID} == set(cc.QUANTS)
  n40 = [c for c in cc.FURTHER if c["NB"] == 40]
  assert len(n40) == 1 and n40[0]["NB"] * (n40[0]["H"] // 4) * (n40[0]["W"] // 8) == 640


# ---- refusals of snnqp_conv_forward_ex -----------------------------------------------------------

def _geom(L, **kw):
  f = dict(H=8, W=8, Cin=64, Cout=32, KH=3, KW=3, stride_h=1, stride_w=1, pad_h_lo=1, pad_h_hi=1,
           pad_w_lo=1, pad_w_hi=1, in_dil_h=1, in_dil_w=1, k_dil_h=1, k_dil_w=1, groups=1)
  f.update(kw)
  return L.ConvGeomT(**f)


def _weight(L, wtype=None, wt_cin=0):
  w = L.WeightT(L.W_I8 if wtype is None else wtype, 8, 7.0, 1.0, 10, 7)
  w.wt_cin = wt_cin
  return w


# (what is wrong with the request, keyword changes, a piece of the reason)
REFUSALS = [
    ("float32 weights", dict(wtype=0), b"not int8 codes"),
    ("5x5 kernel", dict(geom=dict(KH=5, KW=5, pad_h_lo=2, pad_h_hi=2, pad_w_lo=2, pad_w_hi=2)), b"not 3x3"),
    ("stride 2", dict(geom=dict(stride_h=2, stride_w=2)), b"stride is not 1"),
    ("valid padding", dict(geom=dict(pad_h_lo=0, pad_h_hi=0, pad_w_lo=0, pad_w_hi=0)), b"padding is not"),
    ("kernel dilation", dict(geom=dict(k_dil_h=2, k_dil_w=2)), b"dilated"),
    ("input dilation", dict(geom=dict(in_dil_h=2)), b"dilated"),
    ("groups", dict(geom=dict(groups=2)), b"grouped"),
    ("uint8 input", dict(in_type=1), b"bit-packed"),
    ("Cin 129", dict(geom=dict(Cin=129)), b"Cin <= 128"),
    ("no wt", dict(wt=None), b"`wt` not given"),
    ("wt_cin 48", dict(wt_cin=48), b"wt_cin"),
    ("wt_cin below Cin", dict(wt_cin=32), b"wt_cin"),
    ("wt_cin 160", dict(wt_cin=160), b"wt_cin"),
    ("2^30 patches", dict(NB=1 << 30, geom=dict(H=4, W=8)), b"2^30 patches"),
]


def _call(L, impl, in_type=None, geom=None, wtype=None, wt=8, wt_cin=0, NB=2, x=None, y=None):
  g = _geom(L, **(geom or {}))
  w = _weight(L, wtype, wt_cin)
  return L.lib().snnqp_conv_forward_ex(x, L.BITS if in_type is None else in_type, NB, ctypes.byref(g),
                                       ctypes.byref(w), None if wt is None else ctypes.c_void_p(wt),
                                       y, None, impl, None)


@pytest.mark.parametrize("what,kw,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_mfma_refuses_before_any_launch(what, kw, reason):
  """Null tensors: a call that got as far as a launch, or as the null-pointer check, would say so."""
  L = _lib()
  rc = _call(L, L.IMPL_MFMA, **kw)
  err = L.lib().snnqp_last_error()
  assert rc == L.EUNSUPPORTED, (what, rc, err)
  assert b"conv_forward_ex: MFMA kernel" in err and reason in err, (what, err)


@pytest.mark.parametrize("what,kw,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_auto_hands_the_same_requests_to_the_generic_route(what, kw, reason):
  """... whose own argument checks answer (null tensors; groups that do not divide)."""
  L = _lib()
  rc = _call(L, L.IMPL_AUTO, **kw)
  err = L.lib().snnqp_last_error()
  assert rc == L.EINVAL, (what, rc, err)
  assert b"MFMA kernel" not in err
  assert b"null pointer" in err or b"feature_group_count" in err, (what, err)
  # and GENERIC says the same as snnqp_conv_forward
  rc2 = _call(L, L.IMPL_GENERIC, **kw)
  assert rc2 == rc and L.lib().snnqp_last_error() == err


def test_entry_point_argument_checks():
  L = _lib()
  lib = L.lib()
  assert lib.snnqp_version() == 507 == L.ABI_VERSION
  for impl in (-1, 3, 99):
    assert _call(L, impl) == L.EINVAL and b"unknown impl" in lib.snnqp_last_error()
  assert _call(L, L.IMPL_MFMA, NB=-1) == L.EINVAL
  w = _weight(L)
  assert lib.snnqp_conv_forward_ex(None, L.BITS, 1, None, ctypes.byref(w), ctypes.c_void_p(8), None, None,
                                   L.IMPL_MFMA, None) == L.EINVAL
  # a request the kernel serves, with null tensors: its own null-pointer check, still no launch
  assert _call(L, L.IMPL_MFMA) == L.EINVAL and b"conv3x3 currents: null pointer" in lib.snnqp_last_error()
  assert _call(L, L.IMPL_AUTO) == L.EINVAL and b"conv3x3 currents: null pointer" in lib.snnqp_last_error()
  # an empty batch has no buffers and enqueues nothing
  assert _call(L, L.IMPL_MFMA, NB=0) == L.OK
  assert _call(L, L.IMPL_AUTO, NB=0) == L.OK
  # the fallback counters belong to the fused blocks
  cb, db = ctypes.c_int64(-1), ctypes.c_int64(-1)
  lib.snnqp_fallback_counts(ctypes.byref(cb), ctypes.byref(db), None, 0, 1)
  _call(L, L.IMPL_AUTO, geom=dict(Cin=129))
  lib.snnqp_fallback_counts(ctypes.byref(cb), ctypes.byref(db), None, 0, 0)
  assert cb.value == 0 and db.value == 0


# ---- Python ----------------------------------------------------------------------------------------

def test_switch_returns_the_previous_value():
  from snnquantprune_amd import linen as nn
  assert nn.train_conv_mfma() is True                     # the default
  try:
    assert nn.set_train_conv_mfma(False) is True
    assert nn.train_conv_mfma() is False
    assert nn.set_train_conv_mfma(False) is False
    assert nn.set_train_conv_mfma(True) is False
    assert nn.train_conv_mfma() is True
  finally:
    nn.set_train_conv_mfma(True)


def test_conv_forward_mfma_needs_tiled_codes_and_a_raster():
  L = _lib()
  from snnquantprune_amd import ops
  geom = ops.ConvGeom(4, 8, 32, 32, 3, 3, (1, 1), ((1, 1), (1, 1)))
  codes = torch.zeros((3, 3, 32, 32), dtype=torch.int8)
  x = ops.PackedSpikes(torch.zeros((1, 4, 8, 1), dtype=torch.int32), 32)
  w = ops.Weight(L.W_I8, codes, 7.0, 1.0, code_max=7)
  with pytest.raises(L.SnnqpError, match="`wt` not given") as ei:
    ops.conv_forward(x, geom, w, impl="mfma")
  assert ei.value.code == L.EUNSUPPORTED
  wt = ops.Weight(L.W_I8, codes, 7.0, 1.0, wt=torch.zeros(9 * 1024, dtype=torch.int8), code_max=7)
  with pytest.raises(L.SnnqpError, match="bit-packed"):
    ops.conv_forward(torch.zeros((1, 4, 8, 32), dtype=torch.uint8), geom, wt, impl="mfma")
  with pytest.raises(ValueError):
    ops.conv_forward(x, geom, wt, impl="fast")
  # with both, on the CPU: as far as the device check of every op
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.conv_forward(x, geom, wt, impl="mfma")
