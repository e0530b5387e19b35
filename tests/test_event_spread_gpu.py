"""GPU suite: the wave spread of the event layer (conv3x3_u8c2.hip, template parameter
SPREAD) -- the 64-channel launch and the 96-channel half-group launch through ops.conv_lif_forward
bit for bit against the oracle with the switch on and off, the threshold itself, byte frames, the
launches that must stay on the old path, and the model."""
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
  nn.set_event_wave_spread(True)
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
  bias -- every current is <= 0.  (They keep their negative codes: their tables are not trivial.)"""
  leaf["kernel"][..., lo:hi] = -np.abs(leaf["kernel"][..., lo:hi])
  bn["scale"][lo:hi] = np.abs(bn["scale"][lo:hi]) + F32(0.1)
  bn["mean"][lo:hi] = 0
  bn["bias"][lo:hi] = 0


# Seeds: the cases whose first draw leaves a unit of the ORACLE's raster outside the rates asserted
# below (one or six live channels of the half group on a small image) take the first later draw that
# does not -- chosen on the reference alone.
SALT = {(96, 70, 9, 17, 1, "random"): 1, (96, 65, 8, 8, 1, "random"): 1, (96, 65, 16, 24, 1, "fresh"): 2,
        (96, 65, 13, 10, 3, "random"): 2, (96, 65, 13, 10, 3, "fresh"): 2, (96, 65, 9, 17, 1, "random"): 2,
        (96, 65, 9, 17, 3, "random"): 1}


@functools.lru_cache(maxsize=None)
def _block_case(cout, live, H, W, B, bn_kind, T=20):
  """Weights, BatchNorm, binary frames and the oracle's raster (T steps, not pooled); shared by the
  cases that read it, which leave it unchanged.  The raster of the first t steps is that of a run of
  t steps: the block starts from zero state.  Channels from `live` on are silent."""
  from oracle import snn_oracle as o
  from snnquantprune_amd import synthetic as syn
  salt = SALT.get((cout, live, H, W, B, bn_kind), 0) if T == 20 else 0
  r = _rng(77000 + 1000 * cout + 10 * H + W + B + (7 if bn_kind == "fresh" else 0) + 100000 * salt)
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
    # a negative multiplier inside the half group (96) / inside the second group (64), on a live channel
    bn["scale"][{96: 64, 64: 35}.get(cout, cout // 2 + 3)] = F32(-1.25)
  _silence(leaf, bn, live, cout)
  x = (r.random((T, B, H, W, 2)) < 0.3).astype(np.uint8)
  _, s = o.conv_block(x.astype(F32), qweight_of(o, leaf, 4), bn, MSL)
  return leaf, bn, x, s.astype(np.uint8)


def _unit_rates(s, cout, live):
  """Firing rate of the live channels of every unit a wave computes: the four (group, tile) units and,
  at 96 channels, the four quarters of the half group (rows 4 g ..+3, columns 4 q ..+3 of a patch)."""
  H, W = s.shape[2], s.shape[3]
  yy, xx = np.meshgrid(np.arange(H) % 8, np.arange(W) % 8, indexing="ij")
  out = {}
  for w in range(4):
    g, q = w >> 1, w & 1
    rows = (yy >> 2) == q
    out["unit %d" % w] = s[:, :, rows][..., 32 * g:min(32 * g + 32, live)].mean()
    if cout == 96:
      sel = ((yy >> 2) == g) & ((xx >> 2) == q)
      out["quarter %d" % w] = s[:, :, sel][..., 64:live].mean()
  return out


def _check_reference(s, cout, live, what):
  """The conditions on the oracle's raster: every unit of every wave is exercised, silence is silence."""
  for k, rate in _unit_rates(s, cout, live).items():
    assert 0.03 <= rate <= 0.5, (what, k, rate)
  assert not s[..., live:].any(), what


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


def _run_both(x_in, geom, w, bnc, T, pool, expect_spread, ref, what, **kw):
  """The three assertions of a case: the predicate names the path, the raster is the oracle's, and
  the switch off gives the same bits."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  nrn = _nrn()
  out = []
  for on in (True, False):
    nn.set_event_wave_spread(on)
    assert nn.event_wave_spread() == on
    took = ops.conv_event_wave_spread(L.EV1, T, geom, w, nrn, state=False, pool=pool, x_max=1)
    assert took == (on and expect_spread), (what, on, took)
    _, s = ops.conv_lif_forward(x_in, geom, w, nrn, bn=bnc, want_u=False, packed_out=True, pool=pool,
                                impl=L.IMPL_MFMA, x_max=1, **kw)
    out.append(_bits(s))
  np.testing.assert_array_equal(out[0], ref, err_msg=what + " (spread on)")
  np.testing.assert_array_equal(out[1], out[0], err_msg=what + " (switch off)")


# (computed, cout_fire, live): the 64-channel launch, full and with silent channels; the half-group launch
SHAPES = [(64, 0, 64), (64, 0, 54), (96, 80, 80), (96, 80, 70), (96, 80, 65)]
IMAGES = [(8, 8), (16, 24), (13, 10), (9, 17)]              # one patch; several; clipped, odd pool; unaligned rows


@pytest.mark.parametrize("H,W", IMAGES, ids=["%dx%d" % i for i in IMAGES])
@pytest.mark.parametrize("cout,fire,live", SHAPES, ids=["%d_%d_live%d" % g for g in SHAPES])
def test_block_against_the_oracle(dev, oracle, cout, fire, live, H, W):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  geom = ops.ConvGeom(H, W, 2, cout, 3, 3, (1, 1), ((1, 1), (1, 1)))
  for B in (1, 3):
    for bn_kind in ("random", "fresh"):
      leaf, bn, x, s = _block_case(cout, live, H, W, B, bn_kind)
      _check_reference(s, cout, live, (cout, live, H, W, B, bn_kind))
      w, _ = _weight(leaf, fire, dev)
      bnc = _bn(bn, dev)
      for T in (1, 5, 20):
        xin = ops.pack_frames(_t(x[:T], dev), L.EV1)
        for pool in (1, 2):
          ref = packbits_lastaxis(_pooled(oracle, s[:T], pool))
          _run_both(xin, geom, w, bnc, T, pool, True, ref,
                    "%d/%d live %d %dx%d B %d T %d pool %d %s" % (cout, fire, live, H, W, B, T, pool, bn_kind))


@functools.lru_cache(maxsize=None)
def _tie_case():
  """u8c2_binary of tests/tie_cases.py at 96 channels with the last sixteen silent: dyadic codes,
  BatchNorm and threshold, so that membrane potentials land ON the threshold -- in the units of channels
  0..63 and in the half group."""
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
  own = tc.census_of_currents(o, cur[..., :64], cfg, pooled=True)
  return leaf, bn, x, tc.census_of_currents(o, cur, cfg, pooled=True), half, own


@pytest.mark.parametrize("pool", [1, 2])
def test_spread_at_exact_ties(dev, oracle, pool):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, r, half, own = _tie_case()
  # both kinds of unit meet the threshold exactly, and a strict compare would change bits
  for census in (half, own):
    assert census["ties"] >= 20 and census["strict_flips"] >= 20, (census["ties"], census["strict_flips"])
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
  """uint8 binary frames: the packed launch of binary_first takes the spread path.  Count frames: the
  predicated launch behind it redoes the block on the old path with the same weight -- the oracle's
  raster, the bits from cout_fire on zero."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
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
    nn.set_event_wave_spread(on)
    # (the byte launch is never the spread path, whatever the switch says)
    assert not ops.conv_event_wave_spread(L.U8, T, geom, w, _nrn(), state=False, pool=pool, x_max=3)
    _, got = ops.conv_lif_forward(_t(xc, dev), geom, w, _nrn(), bn=bnc, want_u=False, packed_out=True, pool=pool,
                                  impl=L.IMPL_MFMA, x_max=1, binary_first=True)
    g = _bits(got)
    np.testing.assert_array_equal(g, packbits_lastaxis(_pooled(oracle, sc, pool)), err_msg="counts, on %s" % on)
    assert not (g[..., 2] >> 16).any()


# (computed, cout_fire): wave w computes channel group w, as before
OLD_PATH = [(32, 0), (48, 0), (96, 96), (96, 0), (128, 0)]


@pytest.mark.parametrize("cout,fire", OLD_PATH, ids=["%d_%d" % g for g in OLD_PATH])
def test_other_channel_counts_stay_on_the_old_path(dev, oracle, cout, fire):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, s = _block_case(cout, cout, 13, 10, 3, "random", T=5)
  assert s.any(axis=(0, 1, 2, 3)).sum() >= cout // 2
  w, _ = _weight(leaf, fire, dev)
  geom = ops.ConvGeom(13, 10, 2, cout, 3, 3, (1, 1), ((1, 1), (1, 1)))
  xin = ops.pack_frames(_t(x, dev), L.EV1)
  for pool in (1, 2):
    _run_both(xin, geom, w, _bn(bn, dev), 5, pool, False, packbits_lastaxis(_pooled(oracle, s, pool)),
              "%d/%d pool %d" % (cout, fire, pool))


@pytest.mark.parametrize("cout,fire", [(64, 0), (96, 80)])
def test_carried_state_and_long_runs_stay_on_the_old_path(dev, oracle, cout, fire):
  """u0 given, u_T wanted and T above the staging chunk are the variant that carries its potentials:
  the predicate says so and the results are what they were."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  live = fire or cout
  leaf, bn, x, s_ref = _block_case(cout, live, 13, 10, 1, "random", T=40)
  w, _ = _weight(leaf, fire, dev)
  bnc, nrn = _bn(bn, dev), _nrn()
  geom = ops.ConvGeom(13, 10, 2, cout, 3, 3, (1, 1), ((1, 1), (1, 1)))
  u_ref, _ = oracle.conv_block(x.astype(F32), qweight_of(oracle, leaf, 4), bn, MSL)
  xin = ops.pack_frames(_t(x, dev), L.EV1)
  assert ops.conv_event_wave_spread(L.EV1, 20, geom, w, nrn, state=False)
  assert not ops.conv_event_wave_spread(L.EV1, 20, geom, w, nrn, state=True)
  assert not ops.conv_event_wave_spread(L.EV1, 40, geom, w, nrn, state=False)
  # T = 40 > the chunk of 32
  _, s40 = ops.conv_lif_forward(xin, geom, w, nrn, bn=bnc, want_u=False, packed_out=True, impl=L.IMPL_MFMA, x_max=1)
  np.testing.assert_array_equal(_bits(s40), packbits_lastaxis(s_ref))
  # the state out of the first half and into the second
  u1, s1 = ops.conv_lif_forward(ops.pack_frames(_t(x[:20], dev), L.EV1), geom, w, nrn, bn=bnc, want_u=True,
                                packed_out=True, impl=L.IMPL_MFMA, x_max=1)
  u2, s2 = ops.conv_lif_forward(ops.pack_frames(_t(x[20:], dev), L.EV1), geom, w, nrn, bn=bnc, u0=u1, want_u=True,
                                packed_out=True, impl=L.IMPL_MFMA, x_max=1)
  np.testing.assert_array_equal(np.concatenate([_bits(s1), _bits(s2)]), packbits_lastaxis(s_ref))
  np.testing.assert_array_equal(u2.cpu().numpy()[..., :live], u_ref[..., :live])


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
      for spread in (True, False):
        nn.set_channel_compaction(compact)
        nn.set_event_half_group(half)
        nn.set_event_wave_spread(spread)
        ops.profile_start()
        (logits, _), mut = model.apply(variables, x, trgt=None, train=False, rng=None, mutable=["intermediates"])
        ops.profile_stop()
        what = "compaction %s half group %s spread %s" % (compact, half, spread)
        np.testing.assert_array_equal(logits.cpu().numpy(), e["logits"], err_msg=what)
        for i in range(3):
          got = _bits(mut["intermediates"]["pool%d" % i][0])
          assert got.shape[-1] == 4                              # sown at 128 channels
          np.testing.assert_array_equal(got, e["pool%d_bits" % i], err_msg="%s pool%d" % (what, i))
        ch = ops.PROFILE_NOTES.get(C0_TAG, {}).get("channels")
        if compact:
          assert ch is not None and (ch["live_out"], ch["cout"]) == (70, 96), ch
          assert ch.get("half_group") is half, ch
          assert ch.get("wave_spread") is (half and spread), ch
        else:
          assert ch is None, ch
  nn.set_channel_compaction(True)
  nn.set_event_half_group(True)
  nn.set_event_wave_spread(True)
  step = nn.capture(model, variables, x, trgt=None, train=False, rng=None)
  logits, _ = step(x)
  np.testing.assert_array_equal(logits.cpu().numpy(), e["logits"])
