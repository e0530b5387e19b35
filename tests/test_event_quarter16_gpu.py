"""GPU suite: the quarter of the half group on a 16x16x64 matrix instruction (DESIGN.md 4.2;
conv3x3_u8c2.hip, template parameter Q16) -- the 96 / 80 spread launch through ops.conv_lif_forward bit
for bit against the oracle with the switch on and off, the threshold itself, byte frames, the launches
that are not this path, and the model.  The cases are the ones tests/test_event_spread_gpu.py draws
(their oracle rasters keep every quarter's firing rate in 0.03 .. 0.5)."""
import numpy as np
import pytest
import torch

from tests import test_event_spread_gpu as sp
from tests.helpers import packbits_lastaxis, qweight_of

pytestmark = pytest.mark.gpu

F32 = np.float32


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
  nn.set_event_quarter16(True)
  nn.set_event_wave_spread(True)
  nn.set_event_half_group(True)
  nn.set_channel_compaction(True)
  after = ops.fallback_counts()
  assert (after["conv_blocks"], after["dense_blocks"]) == (before["conv_blocks"], before["dense_blocks"]), after
  assert ops.device_status() == 0


def _run_both(x_in, geom, w, bnc, T, pool, expect, ref, what, **kw):
  """The three assertions of a case: the predicate names the path, the raster is the oracle's, and
  the switch off gives the same bits."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  nrn = sp._nrn()
  out = []
  for on in (True, False):
    nn.set_event_quarter16(on)
    assert nn.event_quarter16() == on
    took = ops.conv_event_quarter16(L.EV1, T, geom, w, nrn, state=False, pool=pool, x_max=1)
    assert took == (on and expect), (what, on, took)
    _, s = ops.conv_lif_forward(x_in, geom, w, nrn, bn=bnc, want_u=False, packed_out=True, pool=pool,
                                impl=L.IMPL_MFMA, x_max=1, **kw)
    out.append(sp._bits(s))
  np.testing.assert_array_equal(out[0], ref, err_msg=what + " (quarter16 on)")
  np.testing.assert_array_equal(out[1], out[0], err_msg=what + " (switch off)")


SHAPES = [g for g in sp.SHAPES if g[0] == 96]               # (96, 80) with 80 / 70 / 65 live channels
assert [g[2] for g in SHAPES] == [80, 70, 65]


@pytest.mark.parametrize("H,W", sp.IMAGES, ids=["%dx%d" % i for i in sp.IMAGES])
@pytest.mark.parametrize("cout,fire,live", SHAPES, ids=["%d_%d_live%d" % g for g in SHAPES])
def test_block_against_the_oracle(dev, oracle, cout, fire, live, H, W):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  geom = ops.ConvGeom(H, W, 2, cout, 3, 3, (1, 1), ((1, 1), (1, 1)))
  for B in (1, 3):
    for bn_kind in ("random", "fresh"):
      leaf, bn, x, s = sp._block_case(cout, live, H, W, B, bn_kind)
      sp._check_reference(s, cout, live, (cout, live, H, W, B, bn_kind))
      w, _ = sp._weight(leaf, fire, dev)
      bnc = sp._bn(bn, dev)
      for T in (1, 5, 20):
        xin = ops.pack_frames(sp._t(x[:T], dev), L.EV1)
        for pool in (1, 2):
          ref = packbits_lastaxis(sp._pooled(oracle, s[:T], pool))
          _run_both(xin, geom, w, bnc, T, pool, True, ref,
                    "%d/%d live %d %dx%d B %d T %d pool %d %s" % (cout, fire, live, H, W, B, T, pool, bn_kind))


@pytest.mark.parametrize("pool", [1, 2])
def test_quarter16_at_exact_ties(dev, oracle, pool):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x, r, half, own = sp._tie_case()
  assert half["ties"] >= 20 and half["strict_flips"] >= 20 and half["tie_only_windows"] >= 1
  w, _ = sp._weight(leaf, 80, dev)
  geom = ops.ConvGeom(16, 16, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  mean, mul, bias = oracle.bn_coeffs(bn["mean"], bn["var"], bn["scale"], bn["bias"], 1e-5)
  bnc = ops.BnCoeffs(sp._t(mean, dev), sp._t(mul, dev), sp._t(bias, dev))
  _run_both(ops.pack_frames(sp._t(x, dev), L.EV1), geom, w, bnc, x.shape[0], pool, True,
            packbits_lastaxis(r["pooled"] if pool == 2 else r["s"]), "ties, pool %d" % pool)


@pytest.mark.parametrize("pool", [1, 2])
def test_byte_frames_binary_first_and_counts(dev, oracle, pool):
  """uint8 binary frames: the packed launch of binary_first takes the path.  Count frames: the predicated
  launch behind it is not this path and gives the oracle's raster with the switch either way."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  leaf, bn, x, s = sp._block_case(96, 80, 16, 24, 3, "random")
  w, _ = sp._weight(leaf, 80, dev)
  bnc = sp._bn(bn, dev)
  geom = ops.ConvGeom(16, 24, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  T = 5
  _run_both(sp._t(x[:T], dev), geom, w, bnc, T, pool, True, packbits_lastaxis(sp._pooled(oracle, s[:T], pool)),
            "uint8 binary, pool %d" % pool, binary_first=True)
  xc = x[:T].copy()
  xc[1, 0, 3:9, 5:11, :] = 3
  xc[3, 2, 12:, :4, 1] = 3
  _, sc = oracle.conv_block(xc.astype(F32), qweight_of(oracle, leaf, 4), bn, sp.MSL)
  assert not sc[..., 80:].any() and (sc != s[:T]).any()
  for on in (True, False):
    nn.set_event_quarter16(on)
    assert not ops.conv_event_quarter16(L.U8, T, geom, w, sp._nrn(), state=False, pool=pool, x_max=3)
    _, got = ops.conv_lif_forward(sp._t(xc, dev), geom, w, sp._nrn(), bn=bnc, want_u=False, packed_out=True,
                                  pool=pool, impl=L.IMPL_MFMA, x_max=1, binary_first=True)
    g = sp._bits(got)
    np.testing.assert_array_equal(g, packbits_lastaxis(sp._pooled(oracle, sc, pool)), err_msg="counts, on %s" % on)
    assert not (g[..., 2] >> 16).any()


@pytest.mark.parametrize("live", [64, 54])
def test_the_64_channel_launch_is_not_this_path(dev, oracle, live):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  H, W, B = 13, 10, 3
  leaf, bn, x, s = sp._block_case(64, live, H, W, B, "random")
  w, _ = sp._weight(leaf, 0, dev)
  geom = ops.ConvGeom(H, W, 2, 64, 3, 3, (1, 1), ((1, 1), (1, 1)))
  assert ops.conv_event_wave_spread(L.EV1, 5, geom, w, sp._nrn(), state=False)
  xin = ops.pack_frames(sp._t(x[:5], dev), L.EV1)
  for pool in (1, 2):
    _run_both(xin, geom, w, sp._bn(bn, dev), 5, pool, False, packbits_lastaxis(sp._pooled(oracle, s[:5], pool)),
              "64 live %d pool %d" % (live, pool))


def test_carried_state_and_long_runs_are_not_this_path(dev, oracle):
  """u0 given, u_T wanted and T above the staging chunk are the variant that carries its potentials."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  leaf, bn, x, s_ref = sp._block_case(96, 80, 13, 10, 1, "random", T=40)
  w, _ = sp._weight(leaf, 80, dev)
  bnc, nrn = sp._bn(bn, dev), sp._nrn()
  geom = ops.ConvGeom(13, 10, 2, 96, 3, 3, (1, 1), ((1, 1), (1, 1)))
  u_ref, _ = oracle.conv_block(x.astype(F32), qweight_of(oracle, leaf, 4), bn, sp.MSL)
  xin = ops.pack_frames(sp._t(x, dev), L.EV1)
  for on in (True, False):
    nn.set_event_quarter16(on)
    assert ops.conv_event_quarter16(L.EV1, 20, geom, w, nrn, state=False) == on
    assert not ops.conv_event_quarter16(L.EV1, 20, geom, w, nrn, state=True)
    assert not ops.conv_event_quarter16(L.EV1, 40, geom, w, nrn, state=False)
    # T = 40 > the chunk of 32
    _, s40 = ops.conv_lif_forward(xin, geom, w, nrn, bn=bnc, want_u=False, packed_out=True, impl=L.IMPL_MFMA, x_max=1)
    np.testing.assert_array_equal(sp._bits(s40), packbits_lastaxis(s_ref))
    # the state out of the first half and into the second
    u1, s1 = ops.conv_lif_forward(ops.pack_frames(sp._t(x[:20], dev), L.EV1), geom, w, nrn, bn=bnc, want_u=True,
                                  packed_out=True, impl=L.IMPL_MFMA, x_max=1)
    u2, s2 = ops.conv_lif_forward(ops.pack_frames(sp._t(x[20:], dev), L.EV1), geom, w, nrn, bn=bnc, u0=u1,
                                  want_u=True, packed_out=True, impl=L.IMPL_MFMA, x_max=1)
    np.testing.assert_array_equal(np.concatenate([sp._bits(s1), sp._bits(s2)]), packbits_lastaxis(s_ref))
    np.testing.assert_array_equal(u2.cpu().numpy()[..., :80], u_ref[..., :80])


# ---- the model ------------------------------------------------------------------------------------

def test_model_with_seventy_live_channels(dev, oracle):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops
  c, cfg, e = sp._model_case()
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(c["vars"], dev)
  x = ops.pack_frames(sp._t(c["x"], dev), L.EV1)
  for compact in (True, False):
    for half in (True, False):
      for spread in (True, False):
        for q16 in (True, False):
          nn.set_channel_compaction(compact)
          nn.set_event_half_group(half)
          nn.set_event_wave_spread(spread)
          nn.set_event_quarter16(q16)
          ops.profile_start()
          (logits, _), mut = model.apply(variables, x, trgt=None, train=False, rng=None, mutable=["intermediates"])
          ops.profile_stop()
          what = "compaction %s half group %s spread %s quarter16 %s" % (compact, half, spread, q16)
          np.testing.assert_array_equal(logits.cpu().numpy(), e["logits"], err_msg=what)
          for i in range(3):
            got = sp._bits(mut["intermediates"]["pool%d" % i][0])
            np.testing.assert_array_equal(got, e["pool%d_bits" % i], err_msg="%s pool%d" % (what, i))
          ch = ops.PROFILE_NOTES.get(sp.C0_TAG, {}).get("channels")
          if compact:
            assert ch is not None and (ch["live_out"], ch["cout"]) == (70, 96), ch
            assert ch.get("wave_spread") is (half and spread), ch
            assert ch.get("quarter16") is (half and spread and q16), ch
          else:
            assert ch is None, ch
  nn.set_channel_compaction(True)
  nn.set_event_half_group(True)
  nn.set_event_wave_spread(True)
  nn.set_event_quarter16(True)
  step = nn.capture(model, variables, x, trgt=None, train=False, rng=None)
  logits, _ = step(x)
  np.testing.assert_array_equal(logits.cpu().numpy(), e["logits"])
