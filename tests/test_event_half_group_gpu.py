"""GPU suite: the half group of the event layer (conv3x3_u8c2.hip, template
parameter HALF) -- the block through ops.conv_lif_forward bit for bit against the oracle with the
path on and off, the threshold itself, the launches that must stay on the full path, the refusals,
and the model."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import cases, tie_cases as tc
from tests.helpers import packbits_lastaxis, qweight_of

pytestmark = pytest.mark.gpu

F32 = np.float32
MSL = {"kind": "multi_step_LIF", "tau": 2.0}


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()
  return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _switches_restored():
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  before = ops.fallback_counts()
  yield
  nn.set_event_half_group(True)
  nn.set_channel_compaction(True)
  after = ops.fallback_counts()
  assert (after["conv_blocks"], after["dense_blocks"]) == (before["conv_blocks"], before["dense_blocks"]), after
  assert ops.device_status() == 0


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(s):
  return s.bits.cpu().numpy().view(np.uint32)


def _rng(seed):
  return np.random.Generator(np.random.PCG64(seed))


# ---- the block ------------------------------------------------------------------------------------

def _silence(leaf, bn, lo, hi):
  """Channels lo .. hi - 1 can never fire: no positive code, a positive multiplier, zero mean and
  bias -- every current is <= 0.  (They keep their negative codes: their own tables are not trivial,
  which the switched-off launch reads.)"""
  leaf["kernel"][..., lo:hi] = -np.abs(leaf["kernel"][..., lo:hi])
  bn["scale"][lo:hi] = np.abs(bn["scale"][lo:hi]) + F32(0.1)
  bn["mean"][lo:hi] = 0
  bn["bias"][lo:hi] = 0


@functools.lru_cache(maxsize=None)
def _block_case(cout, fire, H, W, B, bn_kind, live=None, T=20):
  """Weights, BatchNorm, binary frames and the oracle's raster (T steps, not pooled); shared by the
  cases that read it, which leave it unchanged.  The raster of the first t steps is that of a run of
  t steps: the block starts from zero state."""
  from oracle import snn_oracle as o
  from snnquantprune_amd import synthetic as syn
  r = _rng(1000 * cout + 10 * H + W + B + (7 if bn_kind == "fresh" else 0))
  w = (r.standard_normal((3, 3, 2, cout)) * 0.8).astype(F32)
  ac = syn.gaussian_ac(w)
  leaf = {"kernel": w, "DuQ_0": {"a": np.array([ac], F32), "c": np.array([ac], F32)},
          "prune_0": {"mask": syn.magnitude_mask(w, 0.6)}}
  if bn_kind == "fresh":
    bn = {"mean": np.zeros(cout, F32), "var": np.ones(cout, F32), "scale": np.ones(cout, F32),
          "bias": np.zeros(cout, F32)}
  else:
    bn = {"mean": (0.1 * r.standard_normal(cout)).astype(F32), "var": (1 + 0.3 * r.random(cout)).astype(F32),
          "scale": (1 + 0.5 * r.standard_normal(cout)).astype(F32), "bias": (0.2 * r.standard_normal(cout)).astype(F32)}
    bn["scale"][fire - 16 + 3] = F32(-1.25)                 # a negative multiplier inside the half group
  _silence(leaf, bn, fire if live is None else live, cout)
  x = (r.random((T, B, H, W, 2)) < 0.3).astype(np.uint8)
  _, s = o.conv_block(x.astype(F32), qweight_of(o, leaf, 4), bn, MSL)
  assert not s[..., (fire if live is None else live):].any()
  return leaf, bn, x, s.astype(np.uint8)


def _weight(leaf, fire, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  pk = packing.PackedKernel(_t(leaf["kernel"], dev), QuantDesc(L.Q_DUQ, 4, a, c, 7.0, c),
                            _t(leaf["prune_0"]["mask"], dev))
  cout = leaf["kernel"].shape[-1]
  w = pk.sliced(None, np.arange(cout), fire).int_weight()
  assert w.cout_fire == fire and w.ch_slots is not None and 0 < w.code_max <= 7
  return w, pk


def _bn(bn, dev):
  from snnquantprune_amd import ops
  mul = (F32(1) / np.sqrt(bn["var"] + F32(1e-5))) * bn["scale"]
  return ops.BnCoeffs(_t(bn["mean"], dev), _t(mul.astype(F32), dev), _t(bn["bias"], dev))


def _nrn():
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  return ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)


def _pooled(o, s, pool):
  return o.max_pool_2x2(s) if pool == 2 else s


def _run_both(x_in, geom, w, bnc, T, pool, expect_half, ref, what, **kw):
  """The three assertions of a case: the predicate names the path, the raster is the oracle's, and
  the switch off gives the same bits."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  nrn = _nrn()
  out = []
  for on in (True, False):
    nn.set_event_half_group(on)
    assert nn.event_half_group() == on
    took = ops.conv_event_half_group(L.EV1, T, geom, w, nrn, state=False, pool=pool, x_max=1)
    assert took == (on and expect_half), (what, on, took)
    _, s = ops.conv_lif_forward(x_in, geom, w, nrn, bn=bnc, want_u=False, packed_out=True, pool=pool,
                                impl=L.IMPL_MFMA, x_max=1, **kw)
    out.append(_bits(s))
  np.testing.assert_array_equal(out[0], ref, err_msg=what + " (half group on)")
  np.testing.assert_array_equal(out[1], out[0], err_msg=what + " (switch off)")


GROUPS = [(32, 16), (64, 48), (96, 80), (128, 112)]         # the half wave is wave 0 .. 3 in turn
IMAGES = [(8, 8), (16, 24), (13, 10), (9, 17)]              # one patch; several; clipped, odd pool; unaligned rows


@pytest.mark.parametrize("H,W", IMAGES, ids=["%dx%d" % i for i in IMAGES])
@pytest.mark.parametrize("cout,fire", GROUPS, ids=["%d_%d" % g for g in GROUPS])
def test_block_against_the_oracle(dev, oracle, cout, fire, H, W):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  geom = ops.ConvGeom(H, W, 2, cout, 3, 3, (1, 1), ((1, 1), (1, 1)))
  for B in (1, 3):
    for bn_kind in ("random", "fresh"):
      leaf, bn, x, s = _block_case(cout, fire, H, W, B, bn_kind)
      rate = s[..., fire - 16:fire].mean()
      assert 0.03 <= rate <= 0.5, (rate, cout, H, W, B, bn_kind)
      w, _ = _weight(leaf, fire, dev)
      bnc = _bn(bn, dev)
      for T in (1, 5, 20):
        xin = ops.pack_frames(_t(x[:T], dev), L.EV1)
        for pool in (1, 2):
          ref = packbits_lastaxis(_pooled(oracle, s[:T], pool))
          _run_both(xin, geom, w, bnc, T, pool, True, ref,
                    "%d/%d %dx%d B %d T %d pool %d %s" % (cout, fire, H, W, B, T, pool, bn_kind))


@pytest.mark.parametrize("pool", [1, 2])
def test_fewer_than_sixteen_firing_channels(dev, oracle, pool):
  """70 of 80: the last ten channels of the computed half are silent too."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, s = _block_case(96, 80, 16, 24, 3, "random", live=70)
  assert s[..., 64:70].any()
  w, _ = _weight(leaf, 80, dev)
  geom = ops.ConvGeom(16, 24, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  _run_both(ops.pack_frames(_t(x, dev), L.EV1), geom, w, _bn(bn, dev), 20, pool, True,
            packbits_lastaxis(_pooled(oracle, s, pool)), "70 of 80, pool %d" % pool)


@functools.lru_cache(maxsize=None)
def _tie_case():
  """u8c2_binary of tests/tie_cases.py at 96 channels with the last sixteen silent: dyadic codes,
  BatchNorm and threshold, so that membrane potentials of the half group land ON the threshold."""
  import oracle.snn_oracle as o
  c = tc.case("u8c2_binary")
  s0 = 1000 * c["seed"]
  T, B, H, W, cout = 4, 2, 16, 16, 96
  leaf = tc.dyadic_leaf((3, 3, 2, cout), c["bits"], c["k"], s0 + 1, c["prune"])
  bn = tc.dyadic_bn(cout, "per_channel", s0 + 6)
  _silence(leaf, bn, 80, cout)
  bn["var"][80:] = F32(1) - F32(1e-5)
  x = tc.spikes((T, B, H, W, 2), c["density"], s0 + 2)
  b = {"case": dict(c, cout=cout), "leaf": leaf, "x": x, "bn": bn, "strides": None, "padding": ((1, 1), (1, 1))}
  cfg = tc.neuron_cfg("mul0", cout)
  cur = tc.block_currents(o, b)
  half = tc.census_of_currents(o, cur[..., 64:80], cfg, pooled=True)
  return leaf, bn, x, tc.census_of_currents(o, cur, cfg, pooled=True), half


@pytest.mark.parametrize("pool", [1, 2])
def test_half_group_at_exact_ties(dev, oracle, pool):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, r, half = _tie_case()
  # the half group's own channels meet the threshold exactly, and a strict compare would change bits
  assert half["ties"] >= 20 and half["strict_flips"] >= 20, (half["ties"], half["strict_flips"])
  assert half["tie_only_windows"] >= 1
  assert not r["s"][..., 80:].any()
  w, _ = _weight(leaf, 80, dev)
  geom = ops.ConvGeom(16, 16, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  mean, mul, bias = oracle.bn_coeffs(bn["mean"], bn["var"], bn["scale"], bn["bias"], 1e-5)
  bnc = ops.BnCoeffs(_t(mean, dev), _t(mul, dev), _t(bias, dev))
  _run_both(ops.pack_frames(_t(x, dev), L.EV1), geom, w, bnc, x.shape[0], pool, True,
            packbits_lastaxis(r["pooled"] if pool == 2 else r["s"]), "ties, pool %d" % pool)


@pytest.mark.parametrize("pool", [1, 2])
def test_byte_frames_binary_first_and_counts(dev, oracle, pool):
  """uint8 binary frames: the packed launch of binary_first takes the half path.  Count frames: the
  predicated launch behind it redoes the block on the full path with the same weight -- the oracle's
  raster, the bits from cout_fire on zero."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, s = _block_case(96, 80, 16, 24, 3, "random")
  w, _ = _weight(leaf, 80, dev)
  bnc = _bn(bn, dev)
  geom = ops.ConvGeom(16, 24, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  T = 5
  _run_both(_t(x[:T], dev), geom, w, bnc, T, pool, True, packbits_lastaxis(_pooled(oracle, s[:T], pool)),
            "uint8 binary, pool %d" % pool, binary_first=True)
  xc = x[:T].copy()
  xc[1, 0, 3:9, 5:11, :] = 3
  xc[3, 2, 12:, :4, 1] = 3
  _, sc = oracle.conv_block(xc.astype(F32), qweight_of(oracle, leaf, 4), bn, MSL)
  assert not sc[..., 80:].any() and (sc != s[:T]).any()
  for on in (True, False):
    from snnquantprune_amd import linen as nn
    nn.set_event_half_group(on)
    # (the byte launch is never the half path, whatever the switch says)
    assert not ops.conv_event_half_group(L.U8, T, geom, w, _nrn(), state=False, pool=pool, x_max=3)
    _, got = ops.conv_lif_forward(_t(xc, dev), geom, w, _nrn(), bn=bnc, want_u=False, packed_out=True, pool=pool,
                                  impl=L.IMPL_MFMA, x_max=1, binary_first=True)
    g = _bits(got)
    np.testing.assert_array_equal(g, packbits_lastaxis(_pooled(oracle, sc, pool)), err_msg="counts, on %s" % on)
    assert not (g[..., 2] >> 16).any()


def test_carried_state_and_long_runs_stay_on_the_full_path(dev, oracle):
  """u0 given, u_T wanted and T above the staging chunk are the variant that carries its potentials:
  the predicate says so and the results are what they were."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, s = _block_case(96, 80, 13, 10, 1, "random", T=40)
  w, _ = _weight(leaf, 80, dev)
  bnc, nrn = _bn(bn, dev), _nrn()
  geom = ops.ConvGeom(13, 10, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  u_ref, s_ref = oracle.conv_block(x.astype(F32), qweight_of(oracle, leaf, 4), bn, MSL)
  xin = ops.pack_frames(_t(x, dev), L.EV1)
  assert ops.conv_event_half_group(L.EV1, 20, geom, w, nrn, state=False)
  assert not ops.conv_event_half_group(L.EV1, 20, geom, w, nrn, state=True)
  assert not ops.conv_event_half_group(L.EV1, 40, geom, w, nrn, state=False)
  # T = 40 > the chunk of 32
  _, s40 = ops.conv_lif_forward(xin, geom, w, nrn, bn=bnc, want_u=False, packed_out=True, impl=L.IMPL_MFMA, x_max=1)
  np.testing.assert_array_equal(_bits(s40), packbits_lastaxis(s_ref))
  # the state out of the first half and into the second
  u1, s1 = ops.conv_lif_forward(ops.pack_frames(_t(x[:20], dev), L.EV1), geom, w, nrn, bn=bnc, want_u=True,
                                packed_out=True, impl=L.IMPL_MFMA, x_max=1)
  u2, s2 = ops.conv_lif_forward(ops.pack_frames(_t(x[20:], dev), L.EV1), geom, w, nrn, bn=bnc, u0=u1, want_u=True,
                                packed_out=True, impl=L.IMPL_MFMA, x_max=1)
  np.testing.assert_array_equal(np.concatenate([_bits(s1), _bits(s2)]), packbits_lastaxis(s_ref))
  np.testing.assert_array_equal(u2.cpu().numpy()[..., :80], u_ref[..., :80])


@pytest.mark.parametrize("bad", [8, 24, 112])
def test_malformed_cout_fire_is_refused_before_any_launch(dev, bad):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, s = _block_case(96, 80, 8, 8, 1, "fresh")
  w, _ = _weight(leaf, 80, dev)
  wb = dataclasses.replace(w, cout_fire=bad)                 # 112 = Cout + 16
  geom = ops.ConvGeom(8, 8, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  for xin in (ops.pack_frames(_t(x[:3], dev), L.EV1), _t(x[:3], dev)):
    with pytest.raises(L.SnnqpError) as e:
      ops.conv_lif_forward(xin, geom, wb, _nrn(), bn=_bn(bn, dev), want_u=False, packed_out=True,
                           impl=L.IMPL_MFMA, x_max=1)
    assert e.value.code == L.EINVAL and "cout_fire" in str(e.value)
  with pytest.raises(L.SnnqpError):
    ops.conv_event_half_group(L.EV1, 3, geom, wb, _nrn())
  torch.cuda.synchronize()
  assert ops.device_status() == 0


# ---- the model ------------------------------------------------------------------------------------

C0_TAG = "conv3x3[16x16x2->128]"


@functools.lru_cache(maxsize=None)
def _model_case():
  """ConvDenseSNN at 16x16 whose conv0 keeps exactly 70 live channels on binary input."""
  import oracle.snn_oracle as o
  from snnquantprune_amd import prune_utils as pu, synthetic as syn
  c = cases.conv_net_case(T=5, B=2, hw=16, p=0.9, random_bn=True)
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  v = c["vars"]
  live = pu.conv_net_liveness(v, cfg, 1)[0]
  assert live.sum() >= 70
  drop = np.flatnonzero(live)[70:]
  v["params"]["QuantConv_0"]["prune_0"]["mask"][..., drop] = 0
  v["params"]["BatchNorm_0"]["bias"][drop] = F32(-0.25)      # (an all-pruned channel still sees its bias)
  assert int(pu.conv_net_liveness(v, cfg, 1)[0].sum()) == 70
  return c, cfg, cases.conv_net_expected(o, c)


def test_model_with_seventy_live_channels(dev, oracle):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops
  c, cfg, e = _model_case()
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(c["vars"], dev)
  x = ops.pack_frames(_t(c["x"], dev), L.EV1)
  for compact in (True, False):
    for half in (True, False):
      nn.set_channel_compaction(compact)
      nn.set_event_half_group(half)
      ops.profile_start()
      (logits, _), mut = model.apply(variables, x, trgt=None, train=False, rng=None, mutable=["intermediates"])
      ops.profile_stop()
      what = "compaction %s half group %s" % (compact, half)
      np.testing.assert_array_equal(logits.cpu().numpy(), e["logits"], err_msg=what)
      for i in range(3):
        got = _bits(mut["intermediates"]["pool%d" % i][0])
        assert got.shape[-1] == 4                              # sown at 128 channels
        np.testing.assert_array_equal(got, e["pool%d_bits" % i], err_msg="%s pool%d" % (what, i))
      ch = ops.PROFILE_NOTES.get(C0_TAG, {}).get("channels")
      if compact:
        assert ch is not None and (ch["live_out"], ch["cout"]) == (70, 96), ch
        assert ch.get("half_group") is half, ch
      else:
        assert ch is None, ch
  nn.set_channel_compaction(True)
  nn.set_event_half_group(True)
  step = nn.capture(model, variables, x, trgt=None, train=False, rng=None)
  logits, _ = step(x)
  np.testing.assert_array_equal(logits.cpu().numpy(), e["logits"])
