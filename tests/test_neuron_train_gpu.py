"""Training of the PLIF and LIF neurons on the GPU (csrc/train_neuron.hip and the blocks above it):
the two kernels one at a time on the cases of tests/neuron_train_cases.py, bit for bit against
the float32 recurrences of tests/neuron_train_reference.py and inside derived float64 bounds where
bits cannot be promised (slayer's expf, the order of a float64 sum); then the three models with
config.learn_neuron_params: the training forward against the eval forward, the `tau` gradients
against a float64 yardstick, train_step, the stale-decay check and an interrupted training run."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import neuron_train_cases as nc
from tests import neuron_train_reference as nr
from tests import train_reference as tr
from tests.helpers import qweight_of
from tests.train_helpers import _grad_tree, _np, _run_train, mixed

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SURR = {"fast_sigmoid": L.SURR_FAST_SIGMOID, "atan": L.SURR_ATAN, "slayer": L.SURR_SLAYER,
        "smooth_step": L.SURR_SMOOTH_STEP, "piecewise_linear": L.SURR_PIECEWISE_LINEAR}
CASES = nc.all_cases()
_ids = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _neuron(kind, par, vth, vr, dev):
  if kind == "plif":
    return ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, float(par), vth, vr)
  return ops.Neuron(L.NEURON_LIF, 0.0, vth, vr, decay=_t(np.asarray(par, F32), dev))


# ---- 1. forward, saving the residual ---------------------------------------------------------------

@pytest.mark.parametrize("vr", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_forward_save_bit_equal_oracle_and_eval(dev, kind, vr):
  """h, s against the oracle's neuron stepped over the currents, and s and the last state against
  ops.lif_forward (the eval scan) on the same currents."""
  vth = 1.0
  for T in (0, 1, 2, 9):
    for R, C in ((1, 1), (3, 85), (16, 16), (1, 257), (70, 110)):
      rng = np.random.default_rng(T * 1000 + R * C + (kind == "lif"))
      cur = (0.7 + 1.2 * rng.standard_normal((T, R, C))).astype(F32)
      tau = np.array([0.3], F32) if kind == "plif" else nc.lif_taus(rng, C, vr)
      par = nr.oracle.sigmoid_f32(tau[0] if kind == "plif" else tau)
      nrn = _neuron(kind, par, vth, vr, dev)
      h, s = ops.neuron_forward_save(_t(cur, dev), nrn)
      assert tuple(h.shape) == (T, R, C) and tuple(s.shape) == (T, R, C)
      if T == 0:
        continue
      want_h, want_s = nr.neuron_save_ref(kind, cur, tau, vth, vr)
      if R * C > 16 and T > 1:
        assert 0.02 < want_s.mean() < 0.98
      np.testing.assert_array_equal(_np(h), want_h, err_msg="h T=%d R=%d C=%d" % (T, R, C))
      np.testing.assert_array_equal(_np(s), want_s, err_msg="s T=%d R=%d C=%d" % (T, R, C))
      u_eval, s_eval = ops.lif_forward(_t(cur, dev), nrn)
      assert torch.equal(s_eval, s)
      u_last = torch.where(s[-1] != 0, torch.full_like(h[-1], float(F32(vr))), h[-1])
      assert torch.equal(u_eval, u_last)
  h, s = ops.neuron_forward_save(torch.empty((5, 0, 7), device=dev), _neuron("plif", 0.5, 1.0, 0.0, dev))
  assert tuple(h.shape) == (5, 0, 7) and tuple(s.shape) == (5, 0, 7)


# ---- 2. backward: gI and the parameter sums --------------------------------------------------------

def _refs(c, name):
  """float32 recurrence (gI, gh), float64 one with bounds, and the factor of the parameter sum."""
  if c["kind"] == "plif":
    f32 = nr.plif_backward_ref32(c["h"], c["gs"], c["par"], c["vth"], name)
    f64 = nr.plif_backward_ref64(c["h"], c["gs"], c["par"], c["vth"], name)
    return f32, f64, nr.plif_difference(c["h"], c["x"], c["vth"], c["vr"]), False
  f32 = nr.lif_backward_ref32(c["h"], c["gs"], c["par"], c["vth"], name)
  f64 = nr.lif_backward_ref64(c["h"], c["gs"], c["par"], c["vth"], name)
  return f32, f64, nr.carried_state(c["h"], c["vth"], c["vr"]), True


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_backward_every_surrogate_and_splits(dev, case):
  """gI: assert_array_equal against the float32 recurrence for the four surrogates without expf,
  inside the float64 bound for slayer -- for every `splits` the interface takes of {1, 2, 3, R,
  default}.  The parameter sum: |got - ref64| <= gamma_n sum |term|, n = T R C (PLIF) or T R (LIF),
  the reference being the float64 sum of the same exact products (for slayer, of the float64
  recurrence's, with sum E_gh |factor| added); two calls give equal bits.  Largest error / bound
  measured on MI355X: gI (slayer) 0.67 (plif-2x257x130-vr0.1-m1), sums 0.28 (lif-4x3x33-vr0)."""
  _, kind, shape, vr, which = case
  c = nc.case(kind, shape, vr, which)
  T, R, C = shape
  nrn = _neuron(kind, c["par"], c["vth"], vr, dev)
  h, x, gs = _t(c["h"], dev), _t(c["x"], dev), _t(c["gs"], dev)
  default = ops.neuron_backward_splits(T, R, C)
  n = T * R * (C if kind == "plif" else 1)
  worst_gi = worst_sum = 0.0
  for name in tr.SURROGATES:
    (gI32, gh32), (gI64, EI, gh64, Eh), factor, per_feature = _refs(c, name)
    if name == "slayer":
      ref, _ = nr.param_sum(gh64, factor, per_feature)
      bound = nr.param_sum_bound(gh64, Eh, factor, per_feature, n)
    else:
      ref, mag = nr.param_sum(gh32, factor, per_feature)
      bound = nr.param_sum_bound(gh32, np.zeros_like(Eh), factor, per_feature, n)
      np.testing.assert_allclose(bound, n * 2.0 ** -53 / (1 - n * 2.0 ** -53) * mag, rtol=1e-14)
    for splits in nc.splits_of(R, default):
      got, gp = ops.neuron_backward(h, x, nrn, SURR[name], gs=gs, splits=splits)
      again, gp2 = ops.neuron_backward(h, x, nrn, SURR[name], gs=gs, splits=splits)
      assert torch.equal(got, again) and torch.equal(gp, gp2)
      assert gp.dtype == torch.float64 and tuple(gp.shape) == ((C,) if per_feature else (1,))
      got, gp = _np(got), _np(gp)
      if name == "slayer":
        ratio = np.abs(got.astype(F64) - gI64) / EI
        worst_gi = max(worst_gi, float(ratio.max()))
        assert (ratio <= 1.0).all(), (name, splits, ratio.max())
      else:
        np.testing.assert_array_equal(got, gI32, err_msg="%s splits=%d" % (name, splits))
      err = np.abs(gp - np.asarray(ref).reshape(gp.shape))
      b = np.asarray(bound).reshape(gp.shape)
      assert (err <= b).all(), (name, splits, err, b)
      worst_sum = max(worst_sum, float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0)
  print("%s: slayer gI error / bound %.4f, sums error / bound %.4f" % (case[0], worst_gi, worst_sum))


@pytest.mark.parametrize("kind", ["plif", "lif"])
@pytest.mark.parametrize("C,group", [(C, g) for C in (10, 110, 30) for g in sorted({1, 10, C})])
@pytest.mark.parametrize("name", ["atan", "slayer"])
def test_backward_vote_equals_expanded_upstream(dev, name, C, group, kind):
  T, R = 7, 5
  rng = np.random.default_rng(C + group)
  h, _ = tr.planted_h(rng, (T, R, C), 1.0, shift=0.0)
  x = (0.5 + rng.standard_normal((T, R, C))).astype(F32)
  gl = mixed(rng, (R, C // group))
  gs = np.broadcast_to((np.repeat(gl, group, axis=1) / F32(group * T)).astype(F32)[None], (T, R, C)).copy()
  par = F32(0.5744425) if kind == "plif" else nr.oracle.sigmoid_f32(nc.lif_taus(rng, C, 0.0))
  nrn = _neuron(kind, par, 1.0, 0.1, dev)
  ht, xt = _t(h, dev), _t(x, dev)
  for splits in (1, 3, None):
    fused, fp = ops.neuron_backward(ht, xt, nrn, SURR[name], glogits=_t(gl, dev), group=group, splits=splits)
    plain, pp = ops.neuron_backward(ht, xt, nrn, SURR[name], gs=_t(gs, dev), splits=splits)
    assert torch.equal(fused, plain) and torch.equal(fp, pp)
  if name != "slayer":
    fn = nr.plif_backward_ref32 if kind == "plif" else nr.lif_backward_ref32
    np.testing.assert_array_equal(_np(fused), fn(h, gs, par, 1.0, name)[0])


def test_backward_refusals_and_empties(dev):
  plif = _neuron("plif", 0.5, 1.0, 0.0, dev)
  lif = _neuron("lif", np.full(30, 0.5, F32), 1.0, 0.0, dev)
  msl = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  h = torch.zeros((3, 4, 30), device=dev)
  gs, gl = torch.zeros((3, 4, 30), device=dev), torch.zeros((4, 3), device=dev)
  for kw in (dict(glogits=torch.zeros((4, 4), device=dev), group=7), dict(gs=gs, glogits=gl), dict()):
    with pytest.raises(L.SnnqpError) as e:
      ops.neuron_backward(h, h, plif, L.SURR_ATAN, **kw)
    assert e.value.code == L.EINVAL
  with pytest.raises(L.SnnqpError):
    ops.neuron_backward(h, h, plif, 99, gs=gs)
  for splits in (0, 5):
    with pytest.raises(L.SnnqpError):
      ops.neuron_backward(h, h, plif, L.SURR_ATAN, gs=gs, splits=splits)
  with pytest.raises(ValueError):
    ops.neuron_backward(h, None, plif, L.SURR_ATAN, gs=gs)               # PLIF reads the currents
  # multi_step_LIF is refused, naming the entry points that serve it
  for call in (lambda: ops.neuron_forward_save(h, msl), lambda: ops.neuron_backward(h, h, msl, L.SURR_ATAN, gs=gs)):
    with pytest.raises(L.SnnqpError, match="snnqp_lif_") as e:
      call()
    assert e.value.code == L.EUNSUPPORTED
  gI, gp = ops.neuron_backward(h, None, lif, L.SURR_ATAN, gs=gs)          # LIF does not
  assert tuple(gp.shape) == (30,) and not _np(gp).any() and not _np(gI).any()
  for shape in ((0, 4, 30), (3, 0, 30)):
    e = torch.empty(shape, device=dev)
    for nrn, n in ((plif, 1), (lif, 30)):
      gI, gp = ops.neuron_backward(e, e, nrn, L.SURR_ATAN, gs=e)
      assert tuple(gI.shape) == shape and tuple(gp.shape) == (n,) and not _np(gp).any()
      gle = torch.zeros((shape[1], 3), device=dev)
      gI, gp = ops.neuron_backward(e, e, nrn, L.SURR_ATAN, glogits=gle, group=10)
      assert tuple(gI.shape) == shape and not _np(gp).any()
  # the raw entry point writes the zero sums itself
  import ctypes
  gp = torch.full((30,), 7.0, dtype=torch.float64, device=dev)
  p = ctypes.c_void_p(gp.data_ptr())
  rc = L.lib().snnqp_neuron_backward(None, None, p, None, 10, 0, 4, 30, ctypes.byref(lif.struct()), L.SURR_ATAN,
                                     1, None, p, None, 1 << 20,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == L.OK and not _np(gp).any()


# ---- 3. the models ---------------------------------------------------------------------------------

def _dynamics(kind, surrogate="atan", v_reset=0.0):
  from snnquantprune_amd import spiking_learning as sl
  cls = sl.parametric_leaky_IF if kind == "plif" else sl.LIF
  return partial(cls, init_tau=2.0, spike_fn=getattr(sl, surrogate), v_reset=v_reset), cls.__name__


def _with_taus(v, kind, widths, seed=17):
  """The variables with a `tau` leaf per block, in the blocks' order: PLIF's scalars spread around
  0 (m near 0.5), LIF's vectors uniform in [-1, 2]."""
  rng = np.random.default_rng(seed)
  name = _dynamics(kind)[1]
  for i, w in enumerate(widths):
    tau = rng.uniform(-0.5, 0.8, 1) if kind == "plif" else rng.uniform(-1.0, 2.0, w)
    v["params"]["%s_%d" % (name, i)] = {"tau": tau.astype(F32)}
  return v


def _dense_setup(dev, kind, surrogate="atan", v_reset=0.0, dropout=1.0, T=6, B=4, K=256, hidden=96, out=110,
                 seed=941):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  v = _with_taus(syn.dense_net_variables(K, hidden, out, True, 0.5), kind, (hidden, out))
  x = syn.poisson_spikes((B, T, K), 0.2, seed=seed)
  cfg = syn.make_config(bits=8, prune_percentage=0.5, hidden=hidden, dropout=dropout, learn_neuron_params=True)
  cfg.neuron_dynamics = _dynamics(kind, surrogate, v_reset)[0]
  model = models.DenseSNN(num_classes=out // 10, config=cfg)
  return model, v, nn.tree_from_numpy(v, dev), _t(x, dev)


def _conv_setup(dev, kind, dropout=None):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  from tests import conv_train_reference as cr
  v, x = cr.fixture(True, "uint8")
  flat_out = cr.CLASSES * 10
  v = _with_taus(v, kind, (cr.CHANNELS,) * cr.NBLOCKS + (flat_out,))
  cfg = syn.make_config(bits=cr.BITS, prune_percentage=0.9, channels=cr.CHANNELS, tau=cr.TAU,
                        num_conv_blocks=cr.NBLOCKS, dropout=cr.KEEP if dropout is None else dropout,
                        learn_neuron_params=True)
  cfg.neuron_dynamics = _dynamics(kind)[0]
  model = models.ConvDenseSNN(num_classes=cr.CLASSES, config=cfg)
  return model, v, nn.tree_from_numpy(v, dev), _t(x, dev)


def _dense(s):
  return s.to_dense() if hasattr(s, "to_dense") else s


def _tau_paths(params):
  return sorted(p for p in _grad_tree(params) if p[-1] == "tau")


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_dense_train_forward_bit_equal_eval(dev, kind):
  model, v, variables, x = _dense_setup(dev, kind, dropout=1.0)
  (want, _), mut = model.apply(variables, x, train=False, rng=None, mutable=["intermediates"])
  want_s2 = _np(_dense(mut["intermediates"]["dense2_out"][0])).astype(F32)
  _, logits, inter = _run_train(model, variables, x, rng=3, batch_stats=False)
  assert 0.01 < float(want_s2.mean()) < 0.99
  np.testing.assert_array_equal(_np(logits), _np(want))
  np.testing.assert_array_equal(_np(inter["dense2_out"]), want_s2)
  assert float(_np(inter["dropout_1"]).min()) == 1.0


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_conv_train_forward_bit_equal_eval_on_the_batch_statistics(dev, kind):
  """ConvDenseSNN at test_conv_train_gpu.py's shapes, dropout keep 1.0.  Training normalises every
  step with that step's batch statistics and eval with one running set, so the two forwards are
  the same function at T = 1 with the sown statistics as the running ones: there the eval forward
  gives the training forward's spikes and logits."""
  from tests import conv_train_reference as cr
  model, v, variables, x = _conv_setup(dev, kind, dropout=1.0)
  x1 = x[:, :1].contiguous()
  _, logits1, inter1, _ = _run_train(model, variables, x1, rng=3)
  stats = {"BatchNorm_%d" % i: {"mean": inter1["bn%d_mean" % i][0].clone(), "var": inter1["bn%d_var" % i][0].clone()}
           for i in range(cr.NBLOCKS)}
  (want, _), mut = model.apply({"params": variables["params"], "batch_stats": stats}, x1, train=False, rng=None,
                               mutable=["intermediates"])
  s_eval = _np(_dense(mut["intermediates"]["dense_out"][0])).astype(F32)
  assert 0.0 < float(_np(inter1["conv0_out"]).mean()) < 1.0
  np.testing.assert_array_equal(_np(inter1["dense_out"]), s_eval)
  np.testing.assert_array_equal(_np(logits1), _np(want))


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_conv_block_recomputes_the_forwards_scan_input(dev, kind, monkeypatch):
  """PLIF's backward reads the scan's input again; the conv block recomputes it from the saved
  currents and statistics.  Every tensor neuron_backward receives is the one neuron_forward_save
  consumed, bit for bit (LIF's backward is handed none)."""
  from snnquantprune_amd import train_utils as tu
  seen = {"fwd": [], "bwd": []}
  fwd, bwd = ops.neuron_forward_save, ops.neuron_backward

  def spy_fwd(x, neuron):
    seen["fwd"].append(x.detach().clone())
    return fwd(x, neuron)

  def spy_bwd(h, x, neuron, surrogate, **kw):
    seen["bwd"].append(None if x is None else x.detach().clone())
    return bwd(h, x, neuron, surrogate, **kw)

  monkeypatch.setattr(ops, "neuron_forward_save", spy_fwd)
  monkeypatch.setattr(ops, "neuron_backward", spy_bwd)
  model, v, variables, x = _conv_setup(dev, kind)
  params, logits, _, _ = _run_train(model, variables, x, rng=11)
  tu.mse_loss(logits, torch.arange(x.shape[0], device=dev) % 2).backward()
  assert len(seen["fwd"]) == len(seen["bwd"]) == 3                     # two conv blocks and the read-out
  for f, b in zip(seen["fwd"], reversed(seen["bwd"])):
    if kind == "plif":
      assert b is not None and torch.equal(f.reshape(b.shape), b)
    else:
      assert b is None


# float64 yardstick of DenseSNN's gradients with learnt neurons: the vote, the float64 recurrences of
# tests/neuron_train_reference.py (held to autograd by tests/test_neuron_train_cpu.py), the two
# products and tr.duq_vjp, fed the saved float32 forward values.

def _dense_yardstick(oracle, v, kind, x_bt, inter, gL, vth, vr, name, group=10):
  p = v["params"]
  dyn = _dynamics(kind)[1]
  m0, m1 = _np(inter["dropout_0"]).astype(F64), _np(inter["dropout_1"]).astype(F64)
  s1 = _np(inter["dense1_out"]).astype(F64)
  h = {0: _np(inter["dense1_h"]), 1: _np(inter["dense2_h"])}
  xin = {0: np.swapaxes(x_bt.astype(F64) * m0, 0, 1), 1: s1 * m1}
  T = h[1].shape[0]
  g = np.repeat(np.asarray(gL, F64), group, axis=1)[None].repeat(T, 0) / (group * T)
  out = {}
  for i in (1, 0):
    tau = p["%s_%d" % (dyn, i)]["tau"]
    qw = qweight_of(oracle, p["QuantDense_%d" % i], 8, True)
    if kind == "plif":
      par = oracle.sigmoid_f32(tau[0])
      cur = oracle.quant_dense(xin[i].astype(F32), qw, "int")
      gI, _, gh, _ = nr.plif_backward_ref64(h[i], g.astype(F32), par, vth, name)
      # (the upstream enters the recurrence as float32, as the kernel receives it)
      Gp, _ = nr.param_sum(gh, nr.plif_difference(h[i], cur, vth, vr), False)
    else:
      par = oracle.sigmoid_f32(tau)
      gI, _, gh, _ = nr.lif_backward_ref64(h[i], g.astype(F32), par, vth, name)
      Gp, _ = nr.param_sum(gh, nr.carried_state(h[i], vth, vr), True)
    sg = 1.0 / (1.0 + np.exp(-tau.astype(F64)))
    out[(dyn + "_%d" % i, "tau")] = np.asarray(Gp).reshape(tau.shape) * sg * (1 - sg)
    gwq = np.einsum("tbk,tbn->kn", xin[i], gI)
    out[("QuantDense_%d" % i, "kernel")], ga, gc = tr.duq_vjp(gwq, p["QuantDense_%d" % i], 8, True)
    out[("QuantDense_%d" % i, "DuQ_0", "a")], out[("QuantDense_%d" % i, "DuQ_0", "c")] = ga, gc
    if i == 1:
      g = np.einsum("tbn,kn->tbk", gI, qw.w_fq.astype(F64)) * m1
  return out


def _close(got, ref, what):
  """tests/test_dense_train_gpu.py's rule for the leaves that exist today."""
  got, ref = np.asarray(got, F64).reshape(-1), np.asarray(ref, F64).reshape(-1)
  scale = np.abs(ref).max()
  if scale == 0:
    assert np.abs(got).max() == 0, what
    return
  rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
  assert rel <= 1e-5, "%s: relative L2 %.3g" % (what, rel)
  assert np.abs(got - ref).max() <= 1e-4 * scale, "%s: max abs %.3g of %.3g" % (what, np.abs(got - ref).max(), scale)


# largest |got - ref| / max |ref| of a `tau` leaf over the cases below, measured on MI355X (block 1 /
# block 0 per case, in GRAD_CASES' order): PLIF 4.0e-8 / 9.1e-8, 2.4e-8 / 7.1e-8, 7.9e-9 / 3.6e-8;
# LIF 1.3e-7 / 5.05e-7, 1.9e-7 / 1.3e-7, 7.3e-8 / 3.3e-7
TAU_ERR_MEASURED = {"plif": 9.06e-8, "lif": 5.05e-7}
GRAD_CASES = [("plif", "atan", 0.0), ("plif", "fast_sigmoid", 0.1), ("plif", "slayer", 0.0),
              ("lif", "atan", 0.0), ("lif", "piecewise_linear", 0.1), ("lif", "slayer", 0.0)]


@pytest.mark.parametrize("kind,name,vr", GRAD_CASES, ids=["-".join(map(str, c)) for c in GRAD_CASES])
def test_dense_gradients_match_float64_yardstick(dev, oracle, kind, name, vr):
  """Every leaf of DenseSNN against the float64 yardstick.  The kernels, a and c by the rule of
  test_dense_train_gpu.py::test_gradients_match_yardstick; the `tau` leaves within four times the
  largest error measured on MI355X over these cases (the inputs are fixed: the factor covers
  another compiler or machine).  Measured |got - ref| / max |ref|: at most 9.1e-8 for PLIF's
  scalars and 5.05e-7 for LIF's vectors (TAU_ERR_MEASURED lists every case); each neuron is allowed
  four times its own figure, 3.6e-7 and 2.02e-6."""
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _dense_setup(dev, kind, name, vr, dropout=0.8)
  B = x.shape[0]
  labels = (np.arange(B) * 7 % model.num_classes).astype(np.int64)
  params, logits, inter = _run_train(model, variables, x, rng=11, batch_stats=False)
  tu.mse_loss(logits, _t(labels, dev)).backward()
  torch.cuda.synchronize()
  got = _grad_tree(params)
  assert 0.01 < float(_np(inter["dense1_out"]).mean()) < 0.99
  lg = torch.from_numpy(_np(logits).astype(F64)).requires_grad_(True)
  tu.mse_loss(lg, torch.from_numpy(labels)).backward()
  ref = _dense_yardstick(oracle, v, kind, _np(x), inter, lg.grad.numpy(), 1.0, vr, name)
  for path, want in ref.items():
    if path[-1] == "tau":
      assert got[path] is not None and got[path].shape == v["params"][path[0]]["tau"].shape
      assert got[path].dtype == F32 and np.abs(want).max() > 0
      err = np.abs(got[path].astype(F64) - want).max() / np.abs(want).max()
      print("%s %s: tau error %.3g of the largest gradient" % (kind, path[0], err))
      assert err <= 4 * TAU_ERR_MEASURED[kind], (path, err)
    else:
      _close(got[path], want, "/".join(path))
  assert len([p for p in ref if p[-1] == "tau"]) == len(_tau_paths(params)) == 2


_conv_runs = {}


def _conv_run(dev, kind):
  """One training forward and backward of the PLIF / LIF ConvDenseSNN, shared by the checks."""
  if kind not in _conv_runs:
    from snnquantprune_amd import train_utils as tu
    model, v, variables, x = _conv_setup(dev, kind)
    params, logits, inter, stats = _run_train(model, variables, x, rng=11)
    labels = torch.arange(x.shape[0], device=dev) % 2
    tu.mse_loss(logits, labels).backward()
    torch.cuda.synchronize()
    _conv_runs[kind] = dict(v=v, x=x, logits=logits, inter=inter, labels=labels, grads=_grad_tree(params))
  return _conv_runs[kind]


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_conv_saved_state_bit_equal_oracle(dev, oracle, kind):
  """ConvDenseSNN at test_conv_train_gpu.py's shapes and its T = 3: conv*_h, conv*_out, dense_h,
  dense_out bit-equal to the oracle stepped with the block's PLIF / LIF neuron on the sown
  per-step statistics (the state is carried and reset over t, LIF's decays enter), the logits with
  them."""
  from tests import conv_train_reference as cr
  r = _conv_run(dev, kind)
  inter = r["inter"]
  stats = {i: (_np(inter["bn%d_mean" % i]), _np(inter["bn%d_var" % i])) for i in range(cr.NBLOCKS)}
  fwd = nr.conv_oracle_forward(kind, r["v"]["params"], _np(r["x"]), _np(inter["dropout_0"]), stats)
  for i in range(cr.NBLOCKS):
    rate = float(_np(inter["conv%d_out" % i]).mean())
    print("block", i, "rate", rate)
    assert 0.01 < rate < 0.99
    carried = _np(inter["conv%d_out" % i])[:-1]
    assert 0 < carried.mean() < 1                                      # resets and carries both occur
    np.testing.assert_array_equal(_np(inter["conv%d_h" % i]), fwd["h%d" % i])
    np.testing.assert_array_equal(_np(inter["conv%d_out" % i]), fwd["s%d" % i])
  assert 0.01 < float(_np(inter["dense_out"]).mean()) < 0.99
  np.testing.assert_array_equal(_np(inter["dense_h"]), fwd["hd"])
  np.testing.assert_array_equal(_np(inter["dense_out"]), fwd["sd"])
  np.testing.assert_allclose(_np(r["logits"]).astype(F64), fwd["logits"], rtol=1e-6)


# largest |got - ref| / max |ref| of a `tau` leaf of the conv model, measured on MI355X (conv0, conv1,
# read-out): PLIF 2.5e-7, 4.47e-7, 2.4e-8; LIF 3.37e-7, 1.0e-7, 4.0e-8
CONV_TAU_ERR_MEASURED = {"plif": 4.47e-7, "lif": 3.37e-7}


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_conv_gradients_match_float64_autograd(dev, kind):
  """Every leaf of the two-block ConvDenseSNN against torch.autograd on the float64 forward with
  the PLIF / LIF update and a `tau` leaf per block (nr.TorchConvDenseSNN64Neuron), fed the saved
  float32 spikes.  Kernels, a, c, BatchNorm's scale and bias by the rule of
  test_conv_train_gpu.py::test_gradients_match_float64_autograd (relative L2 1e-5; a conv layer's c,
  which cancels to nothing behind BatchNorm, by the gamma bound of its chain).  The `tau` leaves
  within four times the largest |got - ref| / max |ref| measured on MI355X for that neuron:
  measured 4.47e-7 (PLIF) and 3.37e-7 (LIF), allowed 1.79e-6 and 1.35e-6 (CONV_TAU_ERR_MEASURED
  lists every leaf).  The other leaves measured at most 9.0e-6 (conv0's a, PLIF), conv c 0.04 ..
  0.19 and inside its gamma bound."""
  from snnquantprune_amd import train_utils as tu
  from tests import conv_train_reference as cr
  r = _conv_run(dev, kind)
  inter = r["inter"]
  saved = {"hd": _np(inter["dense_h"]), "sd": _np(inter["dense_out"])}
  for i in range(cr.NBLOCKS):
    saved["h%d" % i], saved["s%d" % i] = _np(inter["conv%d_h" % i]), _np(inter["conv%d_out" % i])
  m = nr.TorchConvDenseSNN64Neuron(kind, r["v"]["params"])
  lg = m.forward(_np(r["x"]), _np(inter["dropout_0"]), saved)
  np.testing.assert_allclose(lg.detach().numpy(), _np(r["logits"]).astype(F64), rtol=1e-6, atol=1e-7)
  assert m.h_gap < 1e-4, m.h_gap
  tu.mse_loss(lg, _np(r["labels"])).backward()
  ref, got = m.grads(), r["grads"]
  seen_tau = 0
  for (layer, name), want in ref.items():
    if name == "tau":
      g = got[(layer, "tau")]
      seen_tau += 1
      assert g is not None and g.dtype == F32 and g.shape == want.shape and np.abs(want).max() > 0
      err = np.abs(g.astype(F64) - want).max() / np.abs(want).max()
      print("%s %s: tau error %.3g of the largest gradient" % (kind, layer, err))
      assert err <= 4 * CONV_TAU_ERR_MEASURED[kind], (layer, err)
      continue
    path = (layer, name) if layer.startswith("BatchNorm") else (
        (layer, "kernel") if name == "kernel" else (layer, "DuQ_0", name))
    g = got[path]
    assert g is not None and np.abs(g).max() > 0, path
    rel = np.linalg.norm(g.astype(F64) - want) / np.linalg.norm(want)
    print("%-28s relative L2 %.3g" % ("/".join(path), rel))
    if rel > 1e-5 and name == "c" and layer.startswith("QuantConv"):
      bound = m.c_gamma_bound(int(layer.split("_")[1]))
      err = float(np.abs(g.astype(F64) - want).max())
      assert err <= bound, "%s: |got - ref| %.3g over the gamma bound %.3g" % ("/".join(path), err, bound)
      continue
    assert rel <= 1e-5, "%s: relative L2 %.3g" % ("/".join(path), rel)
  assert seen_tau == cr.NBLOCKS + 1


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_conv_model_tau_leaves_receive_reproducible_gradients(dev, kind):
  """ConvDenseSNN: every `tau` leaf -- two conv blocks behind BatchNorm and the read-out -- gets a
  finite, non-zero gradient in its own shape, and a second backward gives the same bits for
  every leaf."""
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _conv_setup(dev, kind)
  runs = []
  for _ in range(2):
    params, logits, _, _ = _run_train(model, variables, x, rng=11)
    tu.mse_loss(logits, torch.arange(x.shape[0], device=dev) % 2).backward()
    runs.append(_grad_tree(params))
  taus = _tau_paths(params)
  assert len(taus) == 3
  for path in taus:
    g = runs[0][path]
    assert g is not None and g.shape == v["params"][path[0]]["tau"].shape
    assert np.isfinite(g).all() and np.abs(g).max() > 0, path
  for path, g in runs[0].items():
    if g is not None:
      np.testing.assert_array_equal(g, runs[1][path], err_msg="/".join(path))


def test_cextnet_step_plif(dev):
  """One CextNet training forward and backward at its smallest trainable frame (32 x 32), PLIF:
  every `tau` leaf (five conv blocks, two dense) receives a finite, non-zero gradient, and
  backward twice gives equal bits."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn, train_utils as tu
  from tests import cextnet_train_reference as xr
  v, x = xr.fixture(True, "uint8")
  C = xr.CHANNELS
  v["params"]["QuantDense_0"] = syn.quant_leaf((C, 4 * C), 8.0, 141, True, 0.9)
  v = _with_taus(v, "plif", (C,) * 5 + (4 * C, xr.CLASSES * 10))
  x = x[:, :, :32, :32].copy()
  cfg = syn.make_config(bits=xr.BITS, prune_percentage=0.9, channels=C, tau=xr.TAU, dropout=xr.KEEP,
                        gated_int=False, learn_neuron_params=True)
  cfg.neuron_dynamics = _dynamics("plif")[0]
  model = models.CextNet(num_classes=xr.CLASSES, config=cfg)
  variables, xt = nn.tree_from_numpy(v, dev), _t(x, dev)
  runs = []
  for _ in range(2):
    params, logits, _, _ = _run_train(model, variables, xt, rng=11)
    tu.mse_loss(logits, torch.arange(xt.shape[0], device=dev) % xr.CLASSES).backward()
    runs.append(_grad_tree(params))
  taus = _tau_paths(params)
  assert len(taus) == 7
  for path in taus:
    g = runs[0][path]
    assert g is not None and g.shape == (1,) and np.isfinite(g).all() and g[0] != 0, path
  for path, g in runs[0].items():
    if g is not None:
      np.testing.assert_array_equal(g, runs[1][path], err_msg="/".join(path))


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_train_step_moves_tau_and_eval_sees_it(dev, oracle, kind):
  """Two adam steps: the `tau` leaves change, and an eval apply on the tree the steps updated in
  place equals the oracle run with the updated parameters -- a decay or multiplier cached from
  before the steps would not."""
  from snnquantprune_amd import train_utils as tu
  model, v, variables, x = _dense_setup(dev, kind, dropout=0.9)
  cfg = model.config
  cfg.optimizer = "adam"
  labels = torch.arange(x.shape[0], device=dev) % model.num_classes
  (old, _) = model.apply(variables, x, train=False, rng=None)          # the caches hold the old values
  before = {p: t.detach().clone() for p, t in tu._flatten(variables["params"])}
  state = tu.create_train_state(variables, cfg, model)
  for step in range(2):
    state, _ = tu.train_step(state, {"dvs_matrix": x, "label": labels}, 21 + step, lambda s: 1e-2, 0.0, 0.0,
                             tu.mse_loss)
    (mid, _) = model.apply(variables, x, train=False, rng=None)        # and are refreshed between steps
  after = dict(tu._flatten(state.params["params"]))
  taus = [p for p in after if p[-1] == "tau"]
  assert len(taus) == 2
  for p in taus:
    assert not torch.equal(after[p], before[p]), p
    assert bool(torch.isfinite(after[p]).all())
  (got, _), mut = model.apply(variables, x, train=False, rng=None, mutable=["intermediates"])
  (plain, _) = model.apply(variables, x, train=False, rng=None)        # the prepared head's path
  host = tu._unflatten([(p, t.cpu().numpy()) for p, t in after.items()])
  dyn = _dynamics(kind)[1]
  xs = np.swapaxes(_np(x).astype(F32), 0, 1)
  for i in (0, 1):
    tau = host["%s_%d" % (dyn, i)]["tau"]
    ncfg = {"kind": "parametric_leaky_IF", "tau_param": tau} if kind == "plif" else {"kind": "LIF", "tau_vec": tau}
    _, xs = oracle.dense_block(xs, qweight_of(oracle, host["QuantDense_%d" % i], 8, True), ncfg, "int")
  want = oracle.vote(xs, 10)
  assert 0.01 < xs.mean() < 0.99
  np.testing.assert_array_equal(_np(_dense(mut["intermediates"]["dense2_out"][0])).astype(F32), xs)
  np.testing.assert_allclose(_np(got).astype(F64), np.asarray(want, F64), rtol=1e-6)
  assert torch.equal(plain, got) and torch.equal(mid, got)
  assert not torch.equal(got, old)


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_conv_eval_after_train_steps_equals_oracle(dev, oracle, kind):
  """ConvDenseSNN, two adam steps, eval before and between them so that every eval-side cache
  (the decays, the channel-liveness plan of SpikingBlock) holds values from before: the eval apply
  on the updated tree and running statistics equals the oracle run with them."""
  from snnquantprune_amd import train_utils as tu
  from tests import conv_train_reference as cr
  model, v, variables, x = _conv_setup(dev, kind)
  cfg = model.config
  cfg.optimizer = "adam"
  labels = torch.arange(x.shape[0], device=dev) % cr.CLASSES
  state = tu.create_train_state(variables, cfg, model)
  (old, _) = model.apply({"params": state.params["params"], "batch_stats": state.batch_stats}, x, train=False,
                         rng=None)
  for step in range(2):
    state, _ = tu.train_step(state, {"dvs_matrix": x, "label": labels}, 21 + step, lambda s: 5e-2, 0.0, 0.0,
                             tu.mse_loss)
    model.apply({"params": state.params["params"], "batch_stats": state.batch_stats}, x, train=False, rng=None)
  (got, _), mut = model.apply({"params": state.params["params"], "batch_stats": state.batch_stats}, x,
                              train=False, rng=None, mutable=["intermediates"])
  (plain, _) = model.apply({"params": state.params["params"], "batch_stats": state.batch_stats}, x, train=False,
                           rng=None)
  host = tu._unflatten([(p, t.cpu().numpy()) for p, t in tu._flatten(state.params["params"])])
  T = x.shape[1]
  stats = {i: tuple(np.broadcast_to(_np(state.batch_stats["BatchNorm_%d" % i][n]), (T, cr.CHANNELS))
                    for n in ("mean", "var")) for i in range(cr.NBLOCKS)}
  K = (cr.HW >> cr.NBLOCKS) ** 2 * cr.CHANNELS
  fwd = nr.conv_oracle_forward(kind, host, _np(x), np.ones((T, x.shape[0], K), F32), stats)
  for name in nr.neuron_leaf_names(kind, cr.NBLOCKS):
    assert not np.array_equal(host[name]["tau"], v["params"][name]["tau"]), name
  assert 0.01 < fwd["sd"].mean() < 0.99
  np.testing.assert_array_equal(_np(_dense(mut["intermediates"]["dense_out"][0])).astype(F32), fwd["sd"])
  np.testing.assert_allclose(_np(got).astype(F64), fwd["logits"], rtol=1e-6)
  assert torch.equal(plain, got)
  assert not torch.equal(got, old)


@pytest.mark.parametrize("kind", ["plif", "lif"])
def test_interrupted_run_resumes_bit_for_bit_with_tau(dev, tmp_path, kind):
  """train_and_evaluate on tests/train_loop_cases.py's fixture with PLIF or LIF neurons, from
  model.init (LIF's `tau` vectors are drawn there): stopped after 5 of 8 steps and continued, it
  ends at the checkpoint of the uninterrupted run, `tau` and its optimiser moments included, and
  `tau` moves between the two epochs' checkpoints."""
  from snnquantprune_amd import checkpoint, train
  from snnquantprune_amd import train_utils as tu
  from tests import train_loop_cases as lc
  src, test = lc.sources()

  def run(name, stages):
    for stage in stages:
      cfg = lc.make_config(learn_neuron_params=True, learning_rate=0.05, **stage)
      cfg.neuron_dynamics = _dynamics(kind)[0]
      train.train_and_evaluate(cfg, str(tmp_path / name), source=src, eval_source=test, device=dev)
    return ckpt(name, 8)

  def ckpt(name, step):
    with open(os.path.join(str(tmp_path / name), "checkpoint_%d" % step), "rb") as f:
      return {"/".join(p): t for p, t in tu._flatten(checkpoint.msgpack_restore(f.read()))}

  whole = run("whole", [{}])
  resumed = run("resumed", [dict(num_train_steps=5), dict(num_train_steps=-1)])
  assert set(whole) == set(resumed)
  taus = [k for k in whole if k.startswith("params/") and k.endswith("/tau")]
  assert len(taus) == 3 and any(k.startswith("opt_state/0/nu/") and k.endswith("/tau") for k in whole)
  for k, t in whole.items():
    np.testing.assert_array_equal(resumed[k], t, err_msg=k)
  half = ckpt("whole", 4)
  widths = sorted(np.asarray(whole[k]).size for k in taus)
  assert widths == ([1, 1, 1] if kind == "plif" else [16, 16, 20])
  for k in taus:
    assert not np.array_equal(np.asarray(whole[k]), np.asarray(half[k])), k
