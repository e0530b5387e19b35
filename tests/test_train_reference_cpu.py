"""Keeps tests/train_reference.py honest without a GPU: two derivations of DenseSNN's backward
(torch.autograd on the literal float64 forward, and the rules written out by hand) must agree,
the T = 1 closed form needs neither, and the float32 references stay inside their own bounds."""
import numpy as np
import pytest
import torch

from snnquantprune_amd import synthetic as syn
from tests import train_reference as tr
from tests.helpers import qweight_of

F32, F64 = np.float32, np.float64


def _rel(got, ref):
  got, ref = np.asarray(got, F64), np.asarray(ref, F64)
  scale = np.abs(ref).max()
  return 0.0 if scale == 0 and np.abs(got).max() == 0 else np.abs(got - ref).max() / scale


def _case(oracle, seed, T, B, K, hidden, out, tau, vth, vr, quantized, prune_p, keep=0.8,
          counts=False):
  """A float32 forward by the oracle (fseq currents, lif_save_ref) whose h, s and masks stand in
  for what the GPU would have saved."""
  rng = np.random.default_rng(seed)
  v = syn.dense_net_variables(K, hidden, out, quantized, prune_p, seed=seed)
  p = v["params"]
  x = (rng.poisson(0.8, (B, T, K)) if counts else rng.random((B, T, K)) < 0.3).astype(F32)
  m0 = (rng.random((B, T, K)) < keep).astype(F32)
  m1 = (rng.random((T, B, hidden)) < keep).astype(F32)
  w1 = qweight_of(oracle, p["QuantDense_0"], 8, quantized)
  w2 = qweight_of(oracle, p["QuantDense_1"], 8, quantized)
  x0 = np.swapaxes(x * m0, 0, 1)
  h1, s1 = tr.lif_save_ref(oracle.quant_dense(x0, w1, "fseq"), tau, vth, vr)
  h2, s2 = tr.lif_save_ref(oracle.quant_dense(s1 * m1, w2, "fseq"), tau, vth, vr)
  gL = rng.standard_normal((B, out // 10))
  return dict(p=p, x=x, m0=m0, m1=m1, h1=h1, s1=s1, h2=h2, s2=s2, gL=gL)


def _autograd(c, tau, vth, vr, name):
  m = tr.TorchDenseSNN64(c["p"], tau, vth, vr, name)
  logits = m.forward(c["x"], c["m0"], c["m1"], c["h1"], c["s1"], c["h2"], c["s2"])
  (logits * torch.from_numpy(c["gL"])).sum().backward()
  return m, logits


CASES = [
    dict(name="atan"), dict(name="fast_sigmoid", tau=3.0), dict(name="slayer", vth=0.7),
    dict(name="smooth_step", vr=0.1, tau=3.0), dict(name="piecewise_linear", counts=True),
    dict(name="atan", quantized=False, prune_p=-1.0, vr=0.1),
    dict(name="smooth_step", T=1), dict(name="atan", T=7, B=3, hidden=100, out=30, vth=0.7),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("%s=%s" % kv for kv in sorted(c.items())))
def test_autograd_equals_hand_derivation(oracle, case):
  case = dict(case)
  name = case.pop("name")
  tau, vth, vr = case.pop("tau", 2.0), case.pop("vth", 1.0), case.pop("vr", 0.0)
  quantized, prune_p = case.pop("quantized", True), case.pop("prune_p", 0.5)
  c = _case(oracle, 77, case.pop("T", 5), case.pop("B", 4), 48, case.pop("hidden", 40),
            case.pop("out", 20), tau, vth, vr, quantized, prune_p, **case)
  assert 0.02 < c["s1"].mean() < 0.9 and 0.02 < c["s2"].mean() < 0.9      # both layers spike
  m, logits = _autograd(c, tau, vth, vr, name)
  want_logits = c["s2"].astype(F64).mean(0).reshape(logits.shape[0], -1, 10).mean(-1)
  assert _rel(logits.detach().numpy(), want_logits) <= 1e-14
  hand = tr.hand_gradients(c["p"], c["x"], c["m0"], c["m1"], c["h1"], c["s1"], c["h2"], c["s2"],
                           c["gL"], m.wq[1].detach().numpy(), float(F32(tau)), vth, name,
                           quantized)
  auto = m.grads()
  for i in (0, 1):
    assert np.abs(hand[i][0]).max() > 0
    for k, what in enumerate(("kernel", "a", "c")):
      assert _rel(auto[i][k], hand[i][k]) <= 1e-12, (what, i, auto[i][k], hand[i][k])
  if not quantized:
    assert auto[0][1] == 0.0 and auto[0][2] == 0.0


@pytest.mark.parametrize("name", tr.SURROGATES)
def test_autograd_equals_closed_form_at_one_step(oracle, name):
  """T = 1: the read-out layer's gW = x1^T (gs sigma'(h - vth) / tau), with no scan to derive."""
  tau, vth, vr = 3.0, 0.7, 0.1
  c = _case(oracle, 5, 1, 6, 48, 40, 20, tau, vth, vr, True, 0.5)
  m, _ = _autograd(c, tau, vth, vr, name)
  gs = np.repeat(c["gL"], 10, axis=1) / 10.0                            # the two means, T = 1
  x = (c["h2"][0] - F32(vth)).astype(F64)
  want = (c["s1"][0] * c["m1"][0]).astype(F64).T @ (gs * tr.sg64(name, x) / float(F32(tau)))
  assert np.abs(want).max() > 0
  assert _rel(m.wq[1].grad.numpy(), want) <= 1e-12


def test_float64_forward_refuses_a_spike_it_cannot_explain(oracle):
  c = _case(oracle, 5, 3, 4, 48, 40, 20, 2.0, 1.0, 0.0, True, 0.5)
  far = np.argwhere(np.abs(c["h2"] - 1.0) > 0.1)[0]
  c["s2"][tuple(far)] = 1.0 - c["s2"][tuple(far)]
  with pytest.raises(AssertionError, match="disagrees with the saved spike"):
    _autograd(c, 2.0, 1.0, 0.0, "atan")


@pytest.mark.parametrize("name", tr.SURROGATES)
@pytest.mark.parametrize("tau,vth", [(2.0, 1.0), (3.0, 0.7), (1.5, 1.0)])
def test_float32_backward_inside_its_bound(name, tau, vth):
  rng = np.random.default_rng(3)
  h, reached = tr.planted_h(rng, (33, 7, 30), vth)
  assert reached >= ({-0.5, 0.0, 0.5, 0.25, -0.25} if vth == 1.0 else {-0.5, 0.0, 0.25, -0.25})
  gs = (rng.standard_normal(h.shape) * 2.0 ** rng.integers(-6, 7, h.shape)).astype(F32)
  g32 = tr.lif_backward_ref32(h, gs, tau, vth, name)
  g64, bound = tr.lif_backward_ref64(h, gs, tau, vth, name)
  err = np.abs(g32.astype(F64) - g64)
  assert (err <= bound).all(), (err / bound).max()
  assert np.abs(g64).max() > 0 and (bound <= 1e-4 * np.abs(g64).max()).all()   # a bound that binds


def test_backward_recurrence_by_hand():
  """Two steps, one element, numbers a reader can check: tau 2, threshold 1, piecewise_linear."""
  h = np.array([[0.75], [1.25]], F32)                  # x = -0.25 (no spike), 0.25 (spike)
  gs = np.array([[4.0], [8.0]], F32)
  # t = 1: gh = 8 * 0.5 = 4, gI = 2, gu = 2;  t = 0: gh = 4 * 0.5 + 2 * 1 = 4, gI = 2
  assert tr.lif_backward_ref32(h, gs, 2.0, 1.0, "piecewise_linear").tolist() == [[2.0], [2.0]]
  # had t = 0 spiked, nothing would come back through its reset: gh = 4 * 0.5 = 2
  h[0] = 1.25
  assert tr.lif_backward_ref32(h, gs, 2.0, 1.0, "piecewise_linear").tolist() == [[1.0], [2.0]]
  assert tr.lif_backward_ref64(h, gs, 2.0, 1.0, "piecewise_linear")[0].tolist() == [[1.0], [2.0]]


def test_surrogate_edges_float32():
  x = np.array([-0.5, np.nextafter(F32(-0.5), F32(-1)), 0.5, np.nextafter(F32(0.5), F32(0)),
                -0.0, 0.0], F32)
  assert tr.sg32("smooth_step", x).tolist() == [1.0, 0.0, 0.0, 1.0, 1.0, 1.0]
  pl = tr.sg32("piecewise_linear", x)
  assert pl[0] == 0.0 and pl[2] == 0.0 and pl[4] == 1.0 and 0 < pl[3] < 1e-6 and pl[1] == 0.0
  for name in tr.SURROGATES:
    e = np.abs(tr.sg32(name, x).astype(F64) - tr.sg64(name, x))
    assert (e <= tr.sg_rel_err(name, x) * tr.sg64(name, x)).all(), name


@pytest.mark.parametrize("R,I,J", [(0, 3, 5), (1, 1, 1), (17, 65, 33), (5120, 130, 110)])
def test_gemm_chain_inside_gamma_bound(R, I, J):
  rng = np.random.default_rng(R + I)
  a = (rng.standard_normal((R, I)) * 2.0 ** rng.integers(-6, 7, (R, I))).astype(F32)
  b = (rng.standard_normal((R, J)) * 2.0 ** rng.integers(-6, 7, (R, J))).astype(F32)
  c = tr.gemm_chain(a, b)
  assert c.shape == (I, J) and c.dtype == F32
  err = np.abs(c.astype(F64) - tr.gemm_f64(a, b))
  assert (err <= tr.gamma(R) * tr.gemm_mag(a, b)).all()
  if R == 0:
    assert not c.any()
  if R >= 17:
    # the order matters: the reversed chain is another float32 matrix
    assert (tr.gemm_chain(a[::-1], b[::-1]) != c).mean() > 0.5

