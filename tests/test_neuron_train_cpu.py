"""Training of the PLIF and LIF neurons, the part that needs no GPU: the hand recurrences of
tests/neuron_train_reference.py against float64 autograd of the reference's formulas, the
conditions on the cases of tests/neuron_train_cases.py, the host-side refusals and queries of the
new entry points, and which form the training forwards choose with and without
config.learn_neuron_params."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from tests import neuron_train_cases as nc
from tests import neuron_train_reference as nr
from tests import train_reference as tr

F32, F64 = np.float32, np.float64
CASES = nc.all_cases()
_ids = [c[0] for c in CASES]


def _rel(got, ref):
  got, ref = np.asarray(got, F64), np.asarray(ref, F64)
  scale = np.abs(ref).max()
  return 0.0 if scale == 0 and np.abs(got).max() == 0 else np.abs(got - ref).max() / scale


def _ref64(c, name):
  """(gI, EI, gh, Eh, factor, per_feature) of a case by the float64 hand recurrence."""
  if c["kind"] == "plif":
    out = nr.plif_backward_ref64(c["h"], c["gs"], c["par"], c["vth"], name)
    return out + (nr.plif_difference(c["h"], c["x"], c["vth"], c["vr"]), False)
  out = nr.lif_backward_ref64(c["h"], c["gs"], c["par"], c["vth"], name)
  return out + (nr.carried_state(c["h"], c["vth"], c["vr"]), True)


# ---- 1. the hand recurrences are autograd of the reference's formulas ---------------------------

@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_hand_recurrence_is_autograd_of_the_reference(case):
  """gI, Gm and Gd_c of the float64 recurrences against torch.autograd on
  spiking_learning.py:381-385 / :432-436 (the saved float32 values planted), to 1e-12 of the
  largest magnitude, as tests/test_train_reference_cpu.py holds its two derivations together.
  PLIF's keep = fl(1 - m) is exact for m in [0.5, 1], so both sides hold the same number."""
  _, kind, shape, vr, which = case
  c = nc.case(kind, shape, vr, which)
  if kind == "plif":
    assert float(F32(1) - c["par"]) == 1.0 - float(c["par"])
  for name in tr.SURROGATES:
    gI, _, gh, _, factor, per_feature = _ref64(c, name)
    gpar, _ = nr.param_sum(gh, factor, per_feature)
    agI, agp = nr.torch_scan_grads(kind, c["h"], c["x"], c["gs"], c["par"], c["vth"], vr, name)
    assert _rel(gI, agI) <= 1e-12, (name, _rel(gI, agI))
    assert _rel(np.asarray(gpar).reshape(-1), agp.reshape(-1)) <= 1e-12, name


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_float32_recurrence_inside_the_float64_bound(case):
  """The float32 recurrence the kernels are held to lies inside the a-priori bound of the
  float64 one, for every surrogate (the bound is what slayer's kernel output is checked with)."""
  _, kind, shape, vr, which = case
  c = nc.case(kind, shape, vr, which)
  for name in tr.SURROGATES:
    ref, bound = _ref64(c, name)[:2]
    fn = nr.plif_backward_ref32 if kind == "plif" else nr.lif_backward_ref32
    gI32, _ = fn(c["h"], c["gs"], c["par"], c["vth"], name)
    assert (np.abs(gI32.astype(F64) - ref) <= bound).all(), name


# ---- 2. conditions on the cases -----------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_cases_straddle_the_threshold(case):
  """At least a quarter of the potentials on either side of the threshold, so that a wrong
  (1 - s) or a wrong u_{t-1} select changes the result.  The single-element shape cannot hold
  both: its two v_reset cases take one side each."""
  _, kind, shape, vr, which = case
  c = nc.case(kind, shape, vr, which)
  spikes = (c["h"] - F32(c["vth"])) >= 0
  if spikes.size == 1:
    assert bool(spikes.reshape(-1)[0]) == (vr == 0.0)
    return
  assert 0.25 <= spikes.mean() <= 0.75, spikes.mean()
  if kind == "lif":
    d = c["par"]
    assert d.dtype == F32 and (d == F32(0.5)).any() and ((1 - d.astype(F64)) < 2.0 ** -10).any()
    assert (d < 1).all() and (d > 0).all()
  else:
    assert float(c["par"]) in (0.5, float(F32(1 / (1 + np.exp(-np.float64(F32(0.3)))))))


@pytest.mark.parametrize("case", [c for c in CASES if c[2][1] > 1], ids=[c[0] for c in CASES if c[2][1] > 1])
def test_a_dropped_row_breaks_the_sum_bound(case):
  """What the GPU test's bound on the parameter sums can see: leaving out the row that
  contributes most moves the sum by far more than gamma_n sum |term|."""
  _, kind, shape, vr, which = case
  c = nc.case(kind, shape, vr, which)
  T, R, C = shape
  for name in nc.NON_SLAYER:
    gI, _, gh, Eh, factor, per_feature = _ref64(c, name)
    fn = nr.plif_backward_ref32 if kind == "plif" else nr.lif_backward_ref32
    _, gh32 = fn(c["h"], c["gs"], c["par"], c["vth"], name)
    full, mag = nr.param_sum(gh32, factor, per_feature)
    n = T * R * (1 if per_feature else C)
    bound = nr.param_sum_bound(gh32, np.zeros_like(Eh), factor, per_feature, n)
    np.testing.assert_allclose(bound, n * 2.0 ** -53 / (1 - n * 2.0 ** -53) * mag, rtol=1e-14)
    rows = np.abs((gh32.astype(F64) * factor.astype(F64)).sum(axis=(0, 2)))
    part, _ = nr.param_sum(gh32, factor, per_feature, skip_row=int(rows.argmax()))
    assert rows.max() > 0
    assert (np.abs(np.asarray(part) - np.asarray(full)) > bound).any(), name


# ---- 3. the entry points without a GPU ----------------------------------------------------------

def _lib():
  from tests.test_host_cpu import _lib as lib_of
  return lib_of()


def test_queries_and_refusals_without_a_gpu():
  L = _lib()
  lib = L.lib()
  # splits: shapes only, 1..max(R, 1), about 262144 lanes; the same answer every time
  for T, R, C in nc.SHAPES + [(4, 0, 7), (0, 9, 7), (20, 1 << 20, 128), (20, 1 << 33, 1), (3, 5, 1 << 20)]:
    s = lib.snnqp_neuron_backward_splits(T, R, C)
    assert s == lib.snnqp_neuron_backward_splits(T, R, C) == lib.snnqp_neuron_backward_splits(T + 1, R, C)
    assert 1 <= s <= max(R, 1)
    assert s == max(1, min(max(R, 1), -(-262144 // C)))
    groups = -(-s // 32) if s > 32 else 0          # ranges are added in groups of 32, then the groups
    for kind, extra in ((L.NEURON_PARAMETRIC_LEAKY_IF, 1), (L.NEURON_LIF, 0)):
      assert lib.snnqp_neuron_backward_workspace_bytes(T, R, C, s, kind) == 8 * C * (s + groups + extra)
  # small R: one lane per element, today's mapping
  assert lib.snnqp_neuron_backward_splits(7, 5, 30) == 5
  for bad in ((-1, 1, 1), (1, -1, 1), (1, 1, 0)):
    assert lib.snnqp_neuron_backward_splits(*bad) == L.EINVAL
    assert lib.snnqp_neuron_backward_workspace_bytes(*bad, 1, L.NEURON_LIF) == L.EINVAL
  assert lib.snnqp_neuron_backward_workspace_bytes(3, 4, 5, 0, L.NEURON_LIF) == L.EINVAL
  assert lib.snnqp_neuron_backward_workspace_bytes(3, 4, 5, 5, L.NEURON_LIF) == L.EINVAL
  assert lib.snnqp_neuron_backward_workspace_bytes(3, 0, 5, 1, L.NEURON_LIF) == 40
  assert lib.snnqp_neuron_backward_workspace_bytes(3, 4, 5, 4, L.NEURON_MULTI_STEP_LIF) == L.EUNSUPPORTED

  p = ctypes.c_void_p(64)                         # never dereferenced: every call below is refused
  plif = L.NeuronT(L.NEURON_PARAMETRIC_LEAKY_IF, 0.5, 1.0, 0.0, None)
  lif = L.NeuronT(L.NEURON_LIF, 0.0, 1.0, 0.0, p)
  lif_bare = L.NeuronT(L.NEURON_LIF, 0.0, 1.0, 0.0, None)
  msl = L.NeuronT(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0, None)
  none = L.NeuronT(L.NEURON_NONE, 2.0, 1.0, 0.0, None)
  big = 1 << 40

  def fwd(T, R, C, n):
    return lib.snnqp_neuron_forward_save(p, T, R, C, None if n is None else ctypes.byref(n), p, p, None)

  def bwd(T=3, R=4, C=30, n=plif, gs=p, gl=None, group=10, surr=L.SURR_ATAN, splits=2, ws=big,
          gparam=p, h=p, x=p, gI=p, wsp=p):
    return lib.snnqp_neuron_backward(h, x, gs, gl, group, T, R, C, None if n is None else ctypes.byref(n),
                                     surr, splits, gI, gparam, wsp, ws, None)

  assert fwd(3, 4, 0, plif) == L.EINVAL and fwd(-1, 4, 5, plif) == L.EINVAL
  assert fwd(3, 4, 5, None) == L.EINVAL
  assert fwd(3, 4, 5, msl) == L.EUNSUPPORTED and b"snnqp_lif_forward_save" in lib.snnqp_last_error()
  assert fwd(3, 4, 5, none) == L.EUNSUPPORTED
  assert fwd(3, 4, 5, lif_bare) == L.EINVAL and b"decay" in lib.snnqp_last_error()
  assert lib.snnqp_neuron_forward_save(None, 3, 4, 5, ctypes.byref(plif), p, p, None) == L.EINVAL
  assert fwd(0, 4, 5, plif) == L.OK and fwd(3, 0, 5, lif) == L.OK       # empty: nothing launched
  assert fwd(1, 1 << 40, 1, plif) == L.EINVAL and b"grid too large" in lib.snnqp_last_error()

  assert bwd(C=0) == L.EINVAL and bwd(T=-1) == L.EINVAL and bwd(R=-1) == L.EINVAL
  assert bwd(n=None) == L.EINVAL
  assert bwd(n=msl) == L.EUNSUPPORTED and b"snnqp_lif_backward" in lib.snnqp_last_error()
  assert bwd(n=none) == L.EUNSUPPORTED
  assert bwd(n=lif_bare) == L.EINVAL
  assert bwd(gs=p, gl=p) == L.EINVAL and bwd(gs=None, gl=None) == L.EINVAL
  assert bwd(gs=None, gl=p, group=7) == L.EINVAL and bwd(gs=None, gl=p, group=0) == L.EINVAL
  assert bwd(surr=99) == L.EINVAL and b"surrogate" in lib.snnqp_last_error()
  assert bwd(splits=0) == L.EINVAL and bwd(splits=5) == L.EINVAL and bwd(R=0, splits=2) == L.EINVAL
  need = lib.snnqp_neuron_backward_workspace_bytes(3, 4, 30, 2, L.NEURON_PARAMETRIC_LEAKY_IF)
  assert bwd(ws=need - 1) == L.EINVAL and b"workspace" in lib.snnqp_last_error()
  for missing in ("gparam", "h", "x", "gI", "wsp"):
    assert bwd(**{missing: None}) == L.EINVAL, missing
  assert bwd(n=lif, x=None, h=None) == L.EINVAL                       # h is needed, x is not
  assert bwd(T=1, R=1 << 20, C=1 << 20, splits=1 << 12) == L.EINVAL      # 2^32 lanes
  assert b"grid too large" in lib.snnqp_last_error()


# ---- 4. which form the training forwards choose -------------------------------------------------

def test_neuron_train_form_with_and_without_the_switch():
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import spiking_learning as sl, synthetic as syn
  from snnquantprune_amd.dense_train import neuron_train_form, surrogate_of
  msl = sl.multi_step_LIF(tau=2.0, spike_fn=sl.slayer)
  plif = sl.parametric_leaky_IF(init_tau=2.0, spike_fn=sl.atan)
  lif = sl.LIF(init_tau=2.0, spike_fn=sl.fast_sigmoid)
  off = [syn.make_config(), syn.make_config(learn_neuron_params=False), None]
  on = syn.make_config(learn_neuron_params=True)
  for cfg in off + [on]:
    assert neuron_train_form(msl, cfg) == (L.SURR_SLAYER, L.NEURON_MULTI_STEP_LIF)
  for cfg in off:
    for dyn in (plif, lif):
      with pytest.raises(NotImplementedError, match="multi_step_LIF neuron only"):
        neuron_train_form(dyn, cfg)
  assert neuron_train_form(plif, on) == (L.SURR_ATAN, L.NEURON_PARAMETRIC_LEAKY_IF)
  assert neuron_train_form(lif, on) == (L.SURR_FAST_SIGMOID, L.NEURON_LIF)
  with pytest.raises(NotImplementedError, match="no surrogate gradient"):
    neuron_train_form(sl.LIF(init_tau=2.0, spike_fn=lambda x: x), on)
  with pytest.raises(NotImplementedError):                            # surrogate_of keeps its refusal
    surrogate_of(lif)


def test_models_refuse_without_the_switch():
  """Without config.learn_neuron_params a training call with PLIF or LIF is refused as before, in
  DenseSNN and ConvDenseSNN (CextNet's call asks for the GPU first; its blocks are ConvDenseSNN's
  and ask neuron_train_form, which the test above holds)."""
  from snnquantprune_amd import models, spiking_learning as sl, synthetic as syn
  v ={"params": {}, "batch_stats": {}}
  dyns = (partial(sl.parametric_leaky_IF, init_tau=2.0, spike_fn=sl.atan),
          partial(sl.LIF, init_tau=2.0, spike_fn=sl.atan))
  for dyn in dyns:
    for extra in ({}, {"learn_neuron_params": False}):
      cfg = syn.make_config(bits=8, prune_percentage=0.5, hidden=32, dropout=0.9, **extra)
      cfg.neuron_dynamics = dyn
      with pytest.raises(NotImplementedError, match="multi_step_LIF"):
        models.DenseSNN(num_classes=2, config=cfg).apply(v, torch.zeros((2, 3, 64), dtype=torch.uint8),
                                                         train=True, rng=0)
      cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=16, num_conv_blocks=2, dropout=0.9, **extra)
      cfg.neuron_dynamics = dyn
      x = torch.zeros((2, 3, 8, 8, 2), dtype=torch.uint8)
      with pytest.raises(NotImplementedError, match="multi_step_LIF"):
        models.ConvDenseSNN(num_classes=2, config=cfg).apply(v, x, train=True, rng=0)
    # with the switch the form is chosen and the call goes on to the parameters, which this tree lacks
    cfg = syn.make_config(bits=8, prune_percentage=0.5, hidden=32, dropout=0.9, learn_neuron_params=True)
    cfg.neuron_dynamics = dyn
    with pytest.raises(KeyError):
      models.DenseSNN(num_classes=2, config=cfg).apply(v, torch.zeros((2, 3, 64), dtype=torch.uint8),
                                                       train=True, rng=0)
