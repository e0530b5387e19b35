"""Training over windows of a recording without a GPU: in the references
themselves the windowed chain is the whole run; the cases of tests/train_state_cases.py are not
vacuous (they fire, carry non-trivial membranes over every boundary, and a restart from zeros flips
a spike in every later window, so the GPU tests cannot pass on scans that start from zero); the
refusals of a training call with a u_state; and train_step_windows on a stand-in model."""
import numpy as np
import pytest
import torch

from tests import neuron_train_reference as nr
from tests import train_reference as tr
from tests import train_state_cases as sc
from tests import train_state_reference as sr

F32, F64 = np.float32, np.float64
CASES = sc.kernel_cases()
_ids = [c[0] for c in CASES]
SUM_CASES = [c for c in sc.kernel_cases(sc.SHAPES_C) if c[1] in ("plif", "lif")]
_sum_ids = [c[0] for c in SUM_CASES]
SPLIT_IDS = [sc.split_id(s) for s in sc.SPLITS]


@pytest.mark.parametrize("split", sc.SPLITS, ids=SPLIT_IDS)
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_windowed_references_equal_the_whole_run(case, split):
  """Forward values and the chained gI exactly; the final gu0 is the whole run's."""
  c = sc.kernel_case(*case[1:])
  u, hs, ss = None, [], []
  for (t0, t1), want_u0 in zip(sr.windows(sc.T, split), sc.boundary_states(c, split)):
    np.testing.assert_array_equal(np.zeros_like(want_u0) if u is None else u, want_u0)
    h, s, u = sr.save_ref(c["kind"], c["cur"][t0:t1], c["par"], c["vth"], c["vr"], u)
    np.testing.assert_array_equal(u, sr.last_state(h, c["vth"], c["vr"], want_u0))
    hs.append(h)
    ss.append(s)
  np.testing.assert_array_equal(np.concatenate(hs), c["h"])
  np.testing.assert_array_equal(np.concatenate(ss), c["s"])
  np.testing.assert_array_equal(u, c["u_T"])
  whole_gI, whole_gh, whole_gu0 = sr.backward_ref32(c["kind"], c["h"], c["gs"], c["par32"], c["vth"], sc.SURROGATE)
  chain = sc.chained_reference(c, split)
  np.testing.assert_array_equal(np.concatenate([w[4] for w in chain]), whole_gI)
  np.testing.assert_array_equal(np.concatenate([w[5] for w in chain]), whole_gh)
  np.testing.assert_array_equal(chain[0][6], whole_gu0)
  if c["kind"] == sr.MSL:                    # and the whole run is the references' the suite already has
    np.testing.assert_array_equal(whole_gI, tr.lif_backward_ref32(c["h"], c["gs"], c["par"], c["vth"], sc.SURROGATE))
    np.testing.assert_array_equal(c["h"], tr.lif_save_ref(c["cur"], c["par"], c["vth"], c["vr"])[0])
  else:
    np.testing.assert_array_equal(c["h"], nr.neuron_save_ref(c["kind"], c["cur"], c["par"], c["vth"], c["vr"])[0])


@pytest.mark.parametrize("split", sc.SPLITS, ids=SPLIT_IDS)
@pytest.mark.parametrize("case", SUM_CASES, ids=_sum_ids)
def test_window_parameter_sums_add_up_and_need_u0(case, split):
  """The windows' parameter sums (u_{-1} = u0) add up to the whole run's within param_sum_bound;
  with u0 ignored a window after the first is off by more than its own bound."""
  c = sc.kernel_case(*case[1:])
  kind, per_feature = c["kind"], c["kind"] == sr.LIF
  R, C = c["h"].shape[1:]
  _, whole_gh, _ = sr.backward_ref32(kind, c["h"], c["gs"], c["par32"], c["vth"], sc.SURROGATE)
  whole_f = sr.param_factor(kind, c["h"], c["cur"], c["vth"], c["vr"])
  whole, _ = nr.param_sum(whole_gh, whole_f, per_feature)
  n = sc.T * R * (1 if per_feature else C)
  total, broke = 0.0, []
  for t0, t1, u0, gu_T, gI, gh, gu0 in sc.chained_reference(c, split):
    f = sr.param_factor(kind, c["h"][t0:t1], c["cur"][t0:t1], c["vth"], c["vr"], u0)
    np.testing.assert_array_equal(f, whole_f[t0:t1])
    total = total + nr.param_sum(gh, f, per_feature)[0]
    if t0 > 0 and t1 > t0:
      nw = (t1 - t0) * R * (1 if per_feature else C)
      bound = nr.param_sum_bound(gh, np.zeros(gh.shape), f, per_feature, nw)
      f0 = sr.param_factor(kind, c["h"][t0:t1], c["cur"][t0:t1], c["vth"], c["vr"], None)
      off = np.abs(nr.param_sum(gh, f0, per_feature)[0] - nr.param_sum(gh, f, per_feature)[0])
      broke.append(bool((off > bound).any()))
  bound = nr.param_sum_bound(whole_gh, np.zeros(whole_gh.shape), whole_f, per_feature, n)
  assert (np.abs(total - whole) <= bound).all()
  assert all(broke), broke


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_cases_fire_carry_and_would_flip(case):
  c = sc.kernel_case(*case[1:])
  n = c["h"][0].size
  if n > 1:
    rate = float(c["s"].mean())
    assert 0.02 <= rate <= 0.30, rate
  u = sr.carried_state(c["h"], c["vth"], c["vr"])
  for t in range(1, sc.T):
    # at every boundary some membrane is neither 0 nor v_reset
    assert ((u[t] != 0) & (u[t] != F32(c["vr"]))).any(), t
  # in every window after the first a restart from zeros flips a spike of that window (of the
  # single element, which never fires: moves its potential)
  for split in sc.SPLITS:
    for t0, t1 in sr.windows(sc.T, split):
      if t0 == 0 or t1 == t0:
        continue
      h0, s0, _ = sr.save_ref(c["kind"], c["cur"][t0:t1], c["par"], c["vth"], c["vr"], None)
      if n > 1:
        assert (s0 != c["s"][t0:t1]).any(), (split, t0)
      else:
        assert (h0 != c["h"][t0:t1]).all(), (split, t0)
  assert np.abs(c["gs"]).min() > 0


# ---- the models' refusals ----------------------------------------------------------------------------

def _models():
  from snnquantprune_amd import models, synthetic as syn
  dense = models.DenseSNN(num_classes=2, config=syn.make_config(bits=8, prune_percentage=0.5, hidden=16, dropout=0.9))
  conv = models.ConvDenseSNN(num_classes=2, config=syn.make_config(bits=4, prune_percentage=0.9, channels=16,
                                                                    num_conv_blocks=2, dropout=0.9))
  cext = models.CextNet(num_classes=2, config=syn.make_config(dropout=0.9))
  xd = torch.zeros((2, 3, 8), dtype=torch.uint8)
  xc = torch.zeros((2, 3, 8, 8, 2), dtype=torch.uint8)
  return [(dense, xd), (conv, xc), (cext, torch.zeros((2, 3, 32, 32, 2), dtype=torch.uint8))]


def _untouched(st):
  return st.membranes == [] and st.counts is None and st.row_steps is None and st.steps == 0


def test_refusals_leave_the_state_alone():
  from snnquantprune_amd import models, synthetic as syn
  v = {"params": {}, "batch_stats": {}}
  for model, x in _models():
    st = models.StreamState()
    with pytest.raises(NotImplementedError, match="carried state"):
      model.apply(v, x, train=True, rng=0, u_state=[0])
    with pytest.raises(NotImplementedError, match="online"):
      model.apply(v, x, train=True, rng=0, u_state=st, online=True)
    with pytest.raises(NotImplementedError, match="rng"):
      model.apply(v, x, train=True, rng=None, u_state=st)
    assert _untouched(st)
  cext, xc = _models()[2]
  st = models.StreamState()
  with pytest.raises(NotImplementedError, match="TCJA"):
    cext.apply(v, xc, train=True, rng=0, u_state=st)
  assert _untouched(st)
  for model, x in _models()[:2]:
    st = models.StreamState()
    model.config.density_probes = True
    with pytest.raises(NotImplementedError, match="density probes"):
      model.apply(v, x, train=True, rng=0, u_state=st, mutable=["intermediates"])
    assert _untouched(st)
  # a sized state of another batch size: ValueError from the fit, before the parameters are looked at
  dense, xd = _models()[0]
  st = models.StreamState.zeros([(3, 16), (3, 20)], 20)
  before = [t.clone() for t in st._tensors()]
  with pytest.raises(ValueError, match="batch rows"):
    dense.apply(v, xd, train=True, rng=0, u_state=st)
  assert all(torch.equal(a, b) for a, b in zip(before, st._tensors())) and st.steps == 0


# ---- train_step_windows on a stand-in model -----------------------------------------------------------

class _Config(dict):
  __getattr__ = dict.__getitem__


def _stand_in():
  """A TrainState whose apply_fn is a linear read-out of the window's mean input: it takes the
  keywords train_step passes, records them, and books the window in a given StreamState."""
  from snnquantprune_amd import train_utils as tu
  torch.manual_seed(3)
  params = {"w": torch.randn(5, 3)}
  calls = []

  def apply_fn(variables, x, trgt=None, train=False, rng=None, mutable=(), rngs=None, u_state=None):
    calls.append((tuple(x.shape), rng, u_state))
    g = torch.Generator().manual_seed(int(rng))
    noise = torch.rand((), generator=g)
    logits = x.to(torch.float32).mean(1) @ variables["params"]["w"] + noise
    if u_state is not None:
      u_state.steps += x.shape[1]
    return (logits, u_state), {"batch_stats": {}}

  tx = tu.make_optimizer(_Config(optimizer="adam"), [params["w"]])
  return tu.TrainState(apply_fn=apply_fn, params={"params": params}, batch_stats={}, tx=tx, step=0), calls


def test_train_step_windows_on_a_stand_in():
  from snnquantprune_amd import models
  from snnquantprune_amd import train_utils as tu
  x = torch.arange(2 * 6 * 5, dtype=torch.float32).reshape(2, 6, 5) / 10
  batch = {"dvs_matrix": x, "label": torch.tensor([0, 2])}
  args = (lambda step: 1e-2, 0.0, 0.0, tu.mse_loss)
  # window >= T is one train_step
  for window in (6, 9):
    a, calls_a = _stand_in()
    b, calls_b = _stand_in()
    a, m = tu.train_step(a, batch, 7, *args)
    b, ms, st = tu.train_step_windows(b, batch, 7, *args, window=window)
    assert len(ms) == 1 and a.step == b.step == 1 and st.steps == 6
    assert torch.equal(a.params["params"]["w"], b.params["params"]["w"])
    assert torch.equal(ms[0]["loss"], m["loss"])
    assert calls_a[0][:2] == calls_b[0][:2] and calls_a[0][2] is None
    assert isinstance(calls_b[0][2], models.StreamState)
  # windows of 4: 4 + 2 steps, one update each, one state, seeds a function of (seed, window)
  runs = []
  for _ in range(2):
    s, calls = _stand_in()
    s, ms, st = tu.train_step_windows(s, batch, 7, *args, window=4)
    assert [c[0] for c in calls] == [(2, 4, 5), (2, 2, 5)] and s.step == 2 and st.steps == 6
    assert calls[0][2] is st and calls[1][2] is st
    assert calls[0][1] == 7 == tu.window_rng(7, 0) and calls[1][1] == tu.window_rng(7, 1) != 8
    runs.append((s.params["params"]["w"].clone(), [float(m["loss"]) for m in ms]))
  assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
  g = torch.Generator()
  assert tu.window_rng(g, 3) is g
  with pytest.raises(ValueError, match="window"):
    tu.train_step_windows(_stand_in()[0], batch, 7, *args, window=0)
