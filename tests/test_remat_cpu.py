"""Training with rematerialised blocks without a GPU: the references of the two
kernels against the ones the suite already has; the cases of tests/remat_cases.py are not vacuous
(they fire, carry non-trivial membranes over the chunk boundaries, and a restart from zeros flips a
spike in a later chunk, so the GPU tests cannot pass on scans that start from zero); remat_chunks;
in the float64 block model the chunked backward with chained gu0 is the whole-run backward, and
with the chain cut it is not; the refusals of the models and of the two C entries."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_train_reference as cr
from tests import remat_cases as rc
from tests import remat_reference as rr
from tests import train_state_reference as sr

F32, F64 = np.float32, np.float64
CASES = rc.scan_cases()
_ids = [c[0] for c in CASES]
POOLS = rc.pool_cases()


# ---- the reference of the fused scan -------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fused_reference_is_normalise_then_scan(case):
  """Exactly train_state_reference's forward on a numpy bn_normalise: whole, and chunk by chunk from
  the carried membrane for every W."""
  c = rc.scan_case(*case[1:])
  y = rr.bn_normalise(c["cur"], c["mean"], c["mul"], c["bias"])
  h, s, u_T = sr.save_ref(sr.MSL, y, c["tau"], c["vth"], c["vr"])
  np.testing.assert_array_equal(c["h"], h)
  np.testing.assert_array_equal(c["s"], s)
  np.testing.assert_array_equal(c["u_T"], u_T)
  np.testing.assert_array_equal(c["starts"][-1], u_T)
  for W in rc.SPLITS:
    u, hs, ss = None, [], []
    for t0, t1 in rr.chunks(rc.T, W):
      np.testing.assert_array_equal(c["starts"][t0], np.zeros_like(u_T) if u is None else u)
      hk, sk, u = rr.fused_ref(c["cur"][t0:t1], c["mean"][t0:t1], c["mul"][t0:t1], c["bias"], c["tau"],
                               c["vth"], c["vr"], u)
      want = sr.save_ref(sr.MSL, y[t0:t1], c["tau"], c["vth"], c["vr"], c["starts"][t0])
      for a, b in zip((hk, sk, u), want):
        np.testing.assert_array_equal(a, b)
      hs.append(hk)
      ss.append(sk)
    np.testing.assert_array_equal(np.concatenate(hs), c["h"])
    np.testing.assert_array_equal(np.concatenate(ss), c["s"])
    np.testing.assert_array_equal(u, c["u_T"])


def test_multiplier_and_normalise_are_the_packages():
  """Given the multiplier (a tensor the kernel takes as it is), the three roundings are conv_train's
  torch ones, bit for bit; the numpy multiplier is within two roundings of torch's."""
  from snnquantprune_amd import conv_train as ct
  c = rc.scan_case("msl2", 27, 19, 0.1)
  mul = ct.bn_multiplier(torch.from_numpy(np.array(c["var"])), torch.from_numpy(np.array(c["scale"])), rc.EPS)
  np.testing.assert_allclose(mul.numpy(), c["mul"], rtol=2.0 ** -22, atol=0)
  mul = torch.from_numpy(np.array(c["mul"]))
  y = ct.bn_normalise(torch.from_numpy(np.array(c["cur"])), torch.from_numpy(np.array(c["mean"])), mul,
                      torch.from_numpy(np.array(c["bias"])))
  np.testing.assert_array_equal(y.numpy(), rr.bn_normalise(c["cur"], c["mean"], c["mul"], c["bias"]))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_cases_fire_carry_and_would_flip(case):
  c = rc.scan_case(*case[1:])
  n = c["h"][0].size
  rate = float(c["s"].mean(dtype=F64))
  assert 0.02 <= rate <= 0.30, rate
  u = c["starts"]
  # some boundary membrane is neither 0 nor v_reset
  assert any(((u[t] != 0) & (u[t] != F32(c["vr"]))).any() for t in range(1, rc.T))
  # a restart from zeros in a later chunk flips a spike (of the single element: moves its potential)
  flipped = moved = False
  for W in rc.SPLITS:
    for t0, t1 in rr.chunks(rc.T, W)[1:]:
      h0, s0, _ = rr.fused_ref(c["cur"][t0:t1], c["mean"][t0:t1], c["mul"][t0:t1], c["bias"], c["tau"],
                               c["vth"], c["vr"], None)
      flipped |= bool((s0 != c["s"][t0:t1]).any())
      moved |= bool((h0 != c["h"][t0:t1]).any())
  assert moved and (flipped or n == 1)


# ---- the pool's routing read from h --------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", POOLS, ids=[p[0] for p in POOLS])
def test_pool_routing_from_h(name, shape):
  c = rc.pool_case(shape)
  h, gp = c["h"], c["gp"]
  s = ((h - F32(c["vth"])) >= 0).astype(F32)
  want = cr.pool_vjp_first_max(s, gp)
  np.testing.assert_array_equal(rr.pool_route_h(h, c["vth"], gp), want)
  NB, H, W, C = shape
  assert h.size < 64 or (h == F32(c["vth"])).any()          # planted ties fire
  if H >= 2 and W >= 6:
    assert (want[:, 0, 0] == gp[:, 0, 0]).all() and not want[:, 0:2, 1].any()     # none fired: the first
    assert (want[:, 0, 2] == gp[:, 0, 1]).all() and not want[:, 1, 2:4].any()     # all fired: the first
    assert (want[:, 0, 4] == gp[:, 0, 2]).all()                                   # all on the threshold
  if H % 2:
    assert not want[:, H - 1].any()
  if W % 2:
    assert not want[:, :, W - 1].any()
  # every gp element lands exactly once
  np.testing.assert_array_equal(
      want[:, :H // 2 * 2, :W // 2 * 2].reshape(NB, H // 2, 2, W // 2, 2, C).sum((2, 4)), gp)


# ---- remat_chunks ----------------------------------------------------------------------------------------

def test_remat_chunks():
  from snnquantprune_amd import conv_train as ct
  for T in (0, 1, 5, 6, 20):
    for W in (1, 2, 3, 4, 6, 7, 100):
      ch = ct.remat_chunks(T, W)
      assert ch == rr.chunks(T, W)
      assert [t for t0, t1 in ch for t in range(t0, t1)] == list(range(T))     # in order, no overlap
      assert all(0 < t1 - t0 <= W for t0, t1 in ch)
      assert len(ch) == (1 if W >= T and T else -(-T // W))
  assert ct.remat_chunks(0, 3) == []
  assert ct.remat_chunks(6, 4) == [(0, 4), (4, 6)]
  for W in (0, -1, 2.0, None, True, "2"):
    with pytest.raises(ValueError, match="remat"):
      ct.remat_chunks(6, W)


# ---- chunked whole, float64 ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def block64():
  rng = np.random.default_rng(5)
  T, B, HW, Cin, C = 6, 2, 6, 3, 5
  x = (rng.random((T, B, HW, HW, Cin)) < 0.3).astype(F64)
  wq = 0.5 * rng.standard_normal((3, 3, Cin, C))
  scale = 1.5 + 0.2 * rng.standard_normal(C)
  bias = 0.5 + 0.1 * rng.standard_normal(C)
  b = rr.Block64(x, wq, scale, bias)
  gp = rng.standard_normal((T, B, HW // 2, HW // 2, C))
  return b, gp, b.backward(gp)


@pytest.mark.parametrize("W", rc.SPLITS)
def test_chunked_backward_is_the_whole_run_in_float64(block64, W):
  """The tolerance tests/test_conv_train_reference_cpu.py holds float64 to; with gu_T dropped at the
  chunk boundaries some gradient is off by more than that."""
  b, gp, whole = block64
  rate = float(b.s.mean())
  assert 0.02 <= rate <= 0.30, rate
  got = b.backward(gp, W)
  for k, want in whole.items():
    assert np.abs(want).max() > 0, k
    np.testing.assert_allclose(got[k], want, rtol=1e-12, atol=1e-12, err_msg=k)
  if W < 6:
    cut = b.backward(gp, W, chain=False)
    assert any(np.abs(cut[k] - whole[k]).max() > 1e-12 + 1e-12 * np.abs(whole[k]).max() for k in whole)
    assert np.abs(cut["x"] - whole["x"]).max() > 1e-6


# ---- the models' refusals --------------------------------------------------------------------------------

def _models(**extra):
  from snnquantprune_amd import models, synthetic as syn
  dense = models.DenseSNN(num_classes=2, config=syn.make_config(bits=8, prune_percentage=0.5, hidden=16,
                                                                dropout=0.9, **extra))
  conv = models.ConvDenseSNN(num_classes=2, config=syn.make_config(bits=4, prune_percentage=0.9, channels=16,
                                                                    num_conv_blocks=2, dropout=0.9, **extra))
  cext = models.CextNet(num_classes=2, config=syn.make_config(dropout=0.9, **extra))
  return [(dense, torch.zeros((2, 3, 8), dtype=torch.uint8)),
          (conv, torch.zeros((2, 3, 8, 8, 2), dtype=torch.uint8)),
          (cext, torch.zeros((2, 3, 32, 32, 2), dtype=torch.uint8))]


def _untouched(st):
  return st.membranes == [] and st.counts is None and st.row_steps is None and st.steps == 0


V = {"params": {}, "batch_stats": {}}


def test_dense_and_cextnet_refuse_the_key():
  from snnquantprune_amd import models
  (dense, xd), _, (cext, xc) = _models(remat=2)
  st = models.StreamState()
  with pytest.raises(NotImplementedError, match="remat.*weight-sized"):
    dense.apply(V, xd, train=True, rng=0, u_state=st)
  assert _untouched(st)
  with pytest.raises(NotImplementedError, match="remat"):
    dense.apply(V, xd, train=True, rng=0)
  with pytest.raises(NotImplementedError, match="remat.*float64 chain"):
    cext.apply(V, xc, train=True, rng=0)
  # also with a value that is no chunk length: the model's refusal comes first
  (dense, xd), _, (cext, xc) = _models(remat=0)
  with pytest.raises(NotImplementedError, match="remat"):
    dense.apply(V, xd, train=True, rng=0)
  with pytest.raises(NotImplementedError, match="remat"):
    cext.apply(V, xc, train=True, rng=0)


@pytest.mark.parametrize("W", [0, -3, 2.5, "4", None, True])
def test_a_bad_chunk_length_is_a_value_error_before_any_launch(W):
  from snnquantprune_amd import models
  conv, x = _models(remat=W)[1]
  st = models.StreamState()
  with pytest.raises(ValueError, match="remat"):
    conv.apply(V, x, train=True, rng=0, u_state=st)          # (empty parameters: nothing was looked at)
  assert _untouched(st)
  with pytest.raises(ValueError, match="remat"):
    conv.apply(V, x, train=True, rng=0)


def test_existing_refusals_are_unchanged_with_the_key():
  from snnquantprune_amd import models
  for (model, x), (plain, _) in zip(_models(remat=2), _models()):
    calls = [dict(rng=0, u_state=[0]), dict(rng=0, u_state=models.StreamState(), online=True),
             dict(rng=None, u_state=models.StreamState()), dict(rng=0, online=True)]
    bad = x[0] if x.ndim == 5 else torch.zeros((2, 3, 4, 8), dtype=torch.uint8)
    for inputs, kw in [(x, k) for k in calls] + [(bad, dict(rng=0))]:
      errs = []
      for m in (plain, model):
        st = kw.get("u_state")
        with pytest.raises((NotImplementedError, ValueError)) as e:
          m.apply(V, inputs, train=True, **kw)
        errs.append((e.type, str(e.value)))
        assert not isinstance(st, models.StreamState) or _untouched(st)
      assert errs[0] == errs[1] and "remat" not in errs[0][1], errs
  for k, (model, x) in enumerate(_models(remat=2)):
    st = models.StreamState()
    if k == 2:
      with pytest.raises(NotImplementedError, match="TCJA"):
        model.apply(V, x, train=True, rng=0, u_state=st)
    else:
      model.config.density_probes = True
      with pytest.raises(NotImplementedError, match="density probes"):
        model.apply(V, x, train=True, rng=0, u_state=st, mutable=["intermediates"])
    assert _untouched(st)
  for model, x in _models(remat=2):
    del model.config["dropout"]
    with pytest.raises(ValueError, match="config.dropout"):
      model.apply(V, x, train=True, rng=0)


# ---- host refusals of the two C entries --------------------------------------------------------------------

P = ctypes.c_void_p(4096)            # an invented pointer: nothing below reaches a launch


def _neuron(kind, k=2.0):
  from snnquantprune_amd import _lib as L
  return L.NeuronT(kind, k, 1.0, 0.0, None)


def test_bn_lif_forward_state_refuses_on_the_host():
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  f = lib.snnqp_bn_lif_forward_state
  msl = ctypes.byref(_neuron(L.NEURON_MULTI_STEP_LIF))
  err = lambda: lib.snnqp_last_error().decode()   # noqa: E731
  assert f(P, P, P, P, -1, 4, 30, msl, P, P, P, P, None) == L.EINVAL and "bad shape" in err()
  assert f(P, P, P, P, 3, -1, 30, msl, P, P, P, P, None) == L.EINVAL
  assert f(P, P, P, P, 3, 4, 0, msl, P, P, P, P, None) == L.EINVAL
  for k, name in enumerate(("cur", "mean", "mul", "bias")):
    args = [P, P, P, P]
    args[k] = None
    assert f(*args, 3, 4, 30, msl, P, P, P, P, None) == L.EINVAL, name
    assert "null argument" in err()
  # another neuron kind, or none: the entry that serves it is named
  for kind in (L.NEURON_PARAMETRIC_LEAKY_IF, L.NEURON_LIF):
    assert f(P, P, P, P, 3, 4, 30, ctypes.byref(_neuron(kind, 0.5)), P, P, P, P, None) == L.EUNSUPPORTED
    assert "snnqp_neuron_forward_save" in err() and err().startswith("bn_lif_forward_state")
  assert f(P, P, P, P, 3, 4, 30, None, P, P, P, P, None) == L.EUNSUPPORTED
  # too large a grid: 2^31 workgroups of 256 lanes
  assert f(P, P, P, P, 1, 1 << 39, 1, msl, P, P, P, P, None) == L.EINVAL and "grid too large" in err()
  assert f(P, P, P, P, 1, 1 << 40, 1 << 30, msl, P, P, P, P, None) == L.EINVAL
  # nothing to do: no element, or no step and no u_out -- nothing is launched, no pointer looked at
  assert f(None, None, None, None, 3, 0, 30, msl, None, None, None, None, None) == L.OK
  assert f(None, None, None, None, 0, 4, 30, msl, P, None, P, P, None) == L.OK


def test_maxpool2x2_backward_h_refuses_on_the_host():
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  f = lib.snnqp_maxpool2x2_backward_h
  err = lambda: lib.snnqp_last_error().decode()   # noqa: E731
  assert f(P, 1.0, P, 1, 4, 4, 0, P, None) == L.EINVAL and "bad shape" in err()
  assert f(P, 1.0, P, -1, 4, 4, 3, P, None) == L.EINVAL
  assert f(P, 1.0, P, 1, -4, 4, 3, P, None) == L.EINVAL
  assert f(None, 1.0, P, 1, 4, 4, 3, P, None) == L.EINVAL and "null argument" in err()
  assert f(P, 1.0, None, 1, 4, 4, 3, P, None) == L.EINVAL
  assert f(P, 1.0, P, 1, 4, 4, 3, None, None) == L.EINVAL
  assert f(P, 1.0, P, 1 << 39, 1, 1, 1, P, None) == L.EINVAL and "grid too large" in err()
  assert f(P, 1.0, P, 1 << 40, 1 << 20, 1 << 20, 8, P, None) == L.EINVAL and "too large" in err()
  # an empty batch or image launches nothing
  assert f(None, 1.0, None, 0, 4, 4, 3, None, None) == L.OK
  assert f(None, 1.0, None, 2, 0, 4, 3, None, None) == L.OK
  with pytest.raises(RuntimeError, match="GPU only"):
    from snnquantprune_amd import ops
    ops.maxpool2x2_backward_h(torch.zeros(1, 4, 4, 2), 1.0, torch.zeros(1, 2, 2, 2))
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.bn_lif_forward(torch.zeros(2, 4, 3), torch.zeros(2, 3), torch.ones(2, 3), torch.zeros(3),
                       ops.Neuron(L.NEURON_MULTI_STEP_LIF))
