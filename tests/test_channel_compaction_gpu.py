"""GPU suite: channel compaction -- the event layer at 32 / 64 / 96 / 128 output
channels against the oracle, the scatter kernel, and the models with compaction on against the
oracle and against the same run with compaction off (bit-equal)."""
import numpy as np
import pytest
import torch

from tests import cases
from tests.helpers import packbits_lastaxis, qweight_of

pytestmark = pytest.mark.gpu

F32 = np.float32
C0_TAG = "conv3x3[128x128x2->128]"


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()
  return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _compaction_default():
  from snnquantprune_amd import linen as nn
  yield
  nn.set_channel_compaction(True)


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(x):
  return x.bits.cpu().numpy().view(np.uint32)


def _rng(seed):
  return np.random.Generator(np.random.PCG64(seed))


# ---- the scatter kernel ---------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout", [(96, 128), (54, 128), (32, 40), (64, 64)])
def test_scatter_spike_channels(dev, cin, cout):
  from snnquantprune_amd import ops
  r = _rng(cin * 1000 + cout)
  s = (r.random((3, 5, 7, cin)) < 0.3).astype(np.uint8)
  m = r.permutation(cout)[:cin].astype(np.int32)
  m[0] = cout + 3                                  # out of range: dropped
  ps = ops.pack_bits(_t(s, dev).to(torch.float32))
  out = ops.scatter_spike_channels(ps, _t(m, dev), cout)
  ref = np.zeros((3, 5, 7, cout), np.uint8)
  for c in range(1, cin):
    ref[..., m[c]] = s[..., c]
  np.testing.assert_array_equal(_bits(out), packbits_lastaxis(ref))


# ---- the event layer at reduced channel counts ------------------------------------------------

def _event_case(cout, seed, fmt):
  r = _rng(seed)
  w = (r.standard_normal((3, 3, 2, cout)) * 0.8).astype(F32)
  from snnquantprune_amd import synthetic as syn
  leaf = {"kernel": w, "DuQ_0": {"a": np.array([syn.gaussian_ac(w)], F32),
                                  "c": np.array([syn.gaussian_ac(w)], F32)},
          "prune_0": {"mask": syn.magnitude_mask(w, 0.6)}}
  bn = {"mean": (0.1 * r.standard_normal(cout)).astype(F32), "var": (1 + 0.3 * r.random(cout)).astype(F32),
        "scale": (1 + 0.5 * r.standard_normal(cout)).astype(F32), "bias": (0.2 * r.standard_normal(cout)).astype(F32)}
  T, B, H, W = 6, 2, 16, 24
  if fmt == "ev1":
    x = (r.random((T, B, H, W, 2)) < 0.3).astype(np.uint8)
  elif fmt == "ev4":
    x = np.minimum(r.poisson(1.0, (T, B, H, W, 2)), 15).astype(np.uint8)
  else:
    x = (r.random((T, B, H, W, 2)) < 0.3).astype(np.uint8)
    x[2, 1, 5, 7, 0] = 200                         # a hot pixel: its chunk takes the general path
  return leaf, bn, x


def _weights(leaf, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  desc = QuantDesc(L.Q_DUQ, 4, a, c, 7.0, c)
  pk = packing.PackedKernel(_t(leaf["kernel"], dev), desc, _t(leaf["prune_0"]["mask"], dev))
  return pk.int_weight(), pk.float_weight()


@pytest.mark.parametrize("pool", [1, 2])
@pytest.mark.parametrize("fmt", ["u8", "ev1", "ev4", "f32", "pred"])
@pytest.mark.parametrize("cout", [32, 64, 96, 128])
def test_event_layer_reduced_cout(dev, oracle, cout, fmt, pool):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  leaf, bn, x = _event_case(cout, 77 + cout, fmt)
  w, fw = _weights(leaf, dev)
  mul = (F32(1) / np.sqrt(bn["var"] + F32(1e-5))) * bn["scale"]
  bnc = ops.BnCoeffs(_t(bn["mean"], dev), _t(mul.astype(F32), dev), _t(bn["bias"], dev))
  nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  T, B, H, W, _ = x.shape
  geom = ops.ConvGeom(H, W, 2, cout, 3, 3, (1, 1), ((1, 1), (1, 1)))
  xu = _t(x, dev)
  kw = dict(bn=bnc, packed_out=True, pool=pool)
  if fmt == "ev1":
    xin, kw["x_max"] = ops.pack_frames(xu, L.EV1), 1
  elif fmt == "ev4":
    xin, kw["x_max"] = ops.pack_frames(xu, L.EV4), 15
  elif fmt == "f32":
    xin, kw["x_max"], kw["fallback"] = xu.to(torch.float32), 1, ops.FloatFallback(fw)
  elif fmt == "pred":
    xin, kw["x_max"], kw["binary_first"] = xu, 1, True
  else:
    xin, kw["x_max"] = xu, 1
  _, s = ops.conv_lif_forward(xin, geom, w, nrn, want_u=False, **kw)
  qw = qweight_of(oracle, leaf, 4)
  u_ref, s_ref = oracle.conv_block(x.astype(F32), qw, bn, {"kind": "multi_step_LIF", "tau": 2.0})
  if pool == 2:
    s_ref = oracle.max_pool_2x2(s_ref)
  assert s.channels == cout
  np.testing.assert_array_equal(_bits(s), packbits_lastaxis(s_ref))
  if fmt == "u8" and pool == 1:
    # the potentials carried out and back in: two halves of T give the same raster and state
    u1, s1 = ops.conv_lif_forward(xin[:3], geom, w, nrn, bn=bnc, packed_out=True, x_max=1)
    u2, s2 = ops.conv_lif_forward(xin[3:], geom, w, nrn, bn=bnc, u0=u1, packed_out=True, x_max=1)
    np.testing.assert_array_equal(np.concatenate([_bits(s1), _bits(s2)]), packbits_lastaxis(s_ref))
    np.testing.assert_array_equal(u2.cpu().numpy(), u_ref)


# ---- the models ---------------------------------------------------------------------------

def _apply(model, variables, x, compact):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import ops
  nn.set_channel_compaction(compact)
  ops.profile_start()
  (logits, _), mut = model.apply(variables, x, trgt=None, train=False, rng=None,
                                 mutable=["intermediates"])
  ops.profile_stop()
  notes = dict(ops.PROFILE_NOTES)
  pools = [_bits(mut["intermediates"]["pool%d" % i][0]) for i in range(3)]
  return logits.cpu().numpy(), pools, notes


def _inputs(x, dev):
  """EV1 frames, uint8 frames, float32 frames of the same model input [B, T, H, W, 2]."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  xu = _t(x, dev)
  out = {"u8": xu, "f32": xu.to(torch.float32)}
  if x.max() <= 1:
    out["ev1"] = ops.pack_frames(xu, L.EV1)
  return out


def _check_model(model, variables, x, dev, expected=None, compacted=None):
  """Compaction on == off == oracle (logits and the sown pool0..2 at 128 channels)."""
  from snnquantprune_amd import ops
  ops.fallback_counts(reset=True)
  for kind, xin in _inputs(x, dev).items():
    lo_on, pools_on, notes = _apply(model, variables, xin, True)
    lo_off, pools_off, _ = _apply(model, variables, xin, False)
    np.testing.assert_array_equal(lo_on, lo_off, err_msg=kind)
    for i in range(3):
      np.testing.assert_array_equal(pools_on[i], pools_off[i], err_msg="%s pool%d" % (kind, i))
      if expected is not None:
        np.testing.assert_array_equal(pools_on[i], expected["pool%d_bits" % i], err_msg="%s pool%d" % (kind, i))
    if expected is not None:
      np.testing.assert_array_equal(lo_on, expected["logits"], err_msg=kind)
    if compacted is not None:
      ch = notes.get(C0_TAG, {}).get("channels")
      if kind == "f32":
        assert ch is None, ch          # float32 frames hold no bound: nothing compacts
      else:
        assert ch is not None and (ch["live_out"], ch["cout"]) == compacted, (kind, ch)
  assert ops.fallback_counts()["conv_blocks"] == 0
  assert ops.fallback_counts()["dense_blocks"] == 0


@pytest.mark.parametrize("config", ["c3", "c5"])
def test_models_full_geometry(dev, oracle, config):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  lb = [4, 4, 4, 4] if config == "c3" else [2, 4, 2, 4]
  p = 0.9 if config == "c3" else 0.95
  c = cases.conv_net_case(T=6, B=1, hw=128, p=p, layer_bits=lb, out=100, random_bn=False,
                          gains=(4.0, 5.0, 4.0, 4.0))
  e = cases.conv_net_expected(oracle, c)
  cfg = syn.make_config(bits=4, prune_percentage=p)
  cfg.quant.layer_bits = lb
  model = models.ConvDenseSNN(num_classes=10, config=cfg)
  variables = nn.tree_from_numpy(c["vars"], dev)
  _check_model(model, variables, c["x"], dev, e, compacted=(79, 96) if config == "c3" else (54, 64))
  # count frames: counts above 1 -> the predicated launch behind the packed-first one
  xc = syn.poisson_counts((1, 6, 128, 128, 2), 0.4, seed=5)
  assert xc.max() > 1
  c2 = dict(c, x=xc)
  _check_model(model, variables, xc, dev, cases.conv_net_expected(oracle, c2),
               compacted=(79, 96) if config == "c3" else (54, 64))


def _tiny(oracle, seed=3):
  from snnquantprune_amd import synthetic as syn
  c = cases.conv_net_case(T=5, B=2, hw=16, p=0.9, random_bn=True, counts=True)
  return c


def test_liveness_follows_the_input_bound(dev, oracle):
  """Channel 0 of conv0 is silent on binary input but fires on counts: computed for uint8 frames."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  c = _tiny(oracle)
  v = c["vars"]
  k = v["params"]["QuantConv_0"]["kernel"]
  m = v["params"]["QuantConv_0"]["prune_0"]["mask"]
  m[..., 0] = 0
  m[1, 1, 0, 0] = 1
  k[1, 1, 0, 0] = abs(k[1, 1, 0, 0]) + 0.5 * float(v["params"]["QuantConv_0"]["DuQ_0"]["a"][0])
  bnp, bns = v["params"]["BatchNorm_0"], v["batch_stats"]["BatchNorm_0"]
  bnp["bias"][0], bns["mean"][0], bns["var"][0], bnp["scale"][0] = 0.0, 0.0, 1.0, 1.0
  # code of the one tap: q in 1..7; current q / 7 * c per unit of input: silent at 1, not at 255
  from oracle import snn_oracle as o
  qw = qweight_of(o, v["params"]["QuantConv_0"], 4)
  q = float(qw.q[1, 1, 0, 0])
  assert q >= 1
  bnp["scale"][0] = F32(0.9 / (q / 7 * float(qw.m)) / 2)       # x_hi(1) ~ 0.45, x_hi(255) >> 1
  x = np.minimum(c["x"], 30).astype(np.uint8)
  x[:, :, :, :, 0] = np.maximum(x[:, :, :, :, 0], 4)
  c = dict(c, x=x)
  e = cases.conv_net_expected(o, c)
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(v, dev)
  _check_model(model, variables, x, dev, e)
  pool0 = e["pool0_bits"]
  assert (pool0[..., 0] & 1).any(), "channel 0 must fire on counts"


def test_all_pruned_channel_fires_through_bias(dev, oracle):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  c = _tiny(oracle)
  v = c["vars"]
  v["params"]["QuantConv_0"]["prune_0"]["mask"][..., 5] = 0
  v["params"]["BatchNorm_0"]["bias"][5] = 1.5
  x = np.minimum(c["x"], 1).astype(np.uint8)
  c = dict(c, x=x)
  e = cases.conv_net_expected(oracle, c)
  assert ((e["pool0_bits"][..., 0] >> 5) & 1).any()
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  _check_model(model, nn.tree_from_numpy(v, dev), x, dev, e)


def test_cextnet_random_bn(dev, oracle):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  c = cases.cextnet_case(T=4, B=2, hw=64)
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  model = models.CextNet(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(c["vars"], dev)
  _check_model(model, variables, c["x"], dev)


def test_captured_c3_replays(dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, synthetic as syn
  c = cases.conv_net_case(T=6, B=2, hw=128, p=0.9, random_bn=False, gains=(4.0, 5.0, 4.0, 4.0))
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(c["vars"], dev)
  x = ops.pack_frames(_t(c["x"], dev), L.EV1)
  nn.set_channel_compaction(False)
  ref = model.apply(variables, x, trgt=None, train=False, rng=None)[0].cpu().numpy()
  nn.set_channel_compaction(True)
  eager = model.apply(variables, x, trgt=None, train=False, rng=None)[0].cpu().numpy()
  step = nn.capture(model, variables, x, trgt=None, train=False, rng=None)
  for _ in range(2):
    logits, _ = step(x)
    np.testing.assert_array_equal(logits.cpu().numpy(), eager)
  np.testing.assert_array_equal(eager, ref)
  assert ops.fallback_counts()["conv_blocks"] == 0
