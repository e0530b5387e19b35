"""The rate encoder without a device: the hash and key of tests/encode_cases.py, ops.RateTable
against an independent builder, that the reference is a sound generator at the seeds the tests use,
and the host side of the image pipeline (load_source, ImagePlan, the refusals)."""
import ctypes
import math

import numpy as np
import pytest

from tests import encode_cases as ec

TOP = 2 ** 32


# ---- hash and key -----------------------------------------------------------------------------------

def test_fmix32_matches_scalar_implementation():
  rng = np.random.default_rng(3)
  words = np.concatenate([np.array([0, 1, TOP - 1], np.uint64), rng.integers(0, TOP, 1000, dtype=np.uint64)])
  got = ec.fmix32(words)
  assert got.dtype == np.uint32
  assert [int(g) for g in got] == [ec.fmix32_scalar(int(w)) for w in words]
  assert ec.fmix32_scalar(0) == 0 and ec.fmix32_scalar(1) == 0x514E28B7        # murmur3's published value


def test_key_depends_on_every_argument():
  base = dict(seed=7, draw=0, sample_id=[5], T=4, K=6)
  u0 = ec.hashes(**base)
  assert u0.shape == (1, 4, 6) and len(np.unique(u0)) == 24                     # t and k: all distinct
  for key, value in (("seed", 8), ("draw", 1), ("sample_id", [6])):
    u1 = ec.hashes(**dict(base, **{key: value}))
    assert (u1 != u0).all(), key
  # the scalar chain, written out
  c = ec.fmix32_scalar(ec.fmix32_scalar(7 ^ ec.fmix32_scalar(0)) ^ 5)
  assert int(u0[0, 2, 3]) == ec.fmix32_scalar(c ^ (2 * 6 + 3))
  # seed and draw are taken modulo 2^32
  assert np.array_equal(ec.hashes(7 + TOP, TOP, [5], 4, 6), u0)


# ---- table ------------------------------------------------------------------------------------------

PARAMS = [dict(), dict(gain=6.0), dict(gain=0.5, mean=0.1307, std=0.3081), dict(gain=0.0), dict(gain=20.0)]


@pytest.mark.parametrize("kind", ["bernoulli", "poisson"])
@pytest.mark.parametrize("kw", PARAMS, ids=lambda d: "-".join("%s%s" % kv for kv in d.items()) or "default")
def test_rate_table_matches_independent_builder(kind, kw):
  from snnquantprune_amd import ops
  t = ops.RateTable(kind, **kw)
  got, want = t.entries.astype(np.int64), ec.table_reference(kind, **kw).astype(np.int64)
  assert t.entries.shape == (256, 16) and t.entries.dtype == np.uint32
  # two float64 accumulations may round differently: nothing tighter is asserted
  assert np.abs(got - want).max() <= 2
  assert (got[:, 15] == 0).all()
  np.testing.assert_allclose(t.rates, ec.rates(**kw), rtol=1e-15, atol=0)
  if kind == "poisson":
    assert (np.diff(got[:, :15], axis=1) >= 0).all()                            # rows non-decreasing in j
  else:
    assert (got[:, 1:] == 0).all()


def test_rate_table_exact_ends():
  from snnquantprune_amd import ops
  zero = ops.RateTable("poisson", gain=0.0).entries
  assert (zero[:, :15] == TOP - 1).all() and (zero[:, 15] == 0).all()           # r = 0: never a count
  assert (ops.RateTable("bernoulli", gain=0.0).entries == 0).all()              # r = 0: never a spike
  b = ops.RateTable("bernoulli", gain=2.0).entries
  r = np.array(ec.rates(gain=2.0))
  assert (b[r >= 1.0, 0] == TOP - 1).all() and (r >= 1.0).sum() == 128          # r >= 1: always
  assert b[0, 0] == 0 and 0 < b[1, 0] < TOP - 1
  neg = ops.RateTable("poisson", mean=0.5)                                      # negative rates encode as 0
  assert (neg.entries[:128, :15] == TOP - 1).all() and (neg.rates[:128] == 0).all() and neg.rates[255] == 0.5


@pytest.mark.parametrize("gain", [0.0, 1.0, 6.0, 20.0])
def test_truncated_mass(gain):
  from snnquantprune_amd import ops
  t = ops.RateTable("poisson", gain=gain)
  want = max(ec.truncated_mass_reference(r) for r in ec.rates(gain=gain))
  # the table forms 1 - P(X <= 15) from a float64 sum of 16 terms: a few ulps of 1
  assert abs(t.truncated_mass - want) <= 1e-14
  assert ops.RateTable("bernoulli", gain=gain).truncated_mass == 0.0
  if gain == 20.0:
    assert 0.8 < t.truncated_mass < 0.9                                         # P(X > 15; 20) = 0.843...


def test_rate_table_refusals():
  from snnquantprune_amd import ops
  with pytest.raises(ValueError, match="kind"):
    ops.RateTable("gauss")
  for kw in (dict(std=0.0), dict(std=-1.0)):
    with pytest.raises(ValueError, match="std"):
      ops.RateTable("poisson", **kw)
  for kw in (dict(gain=math.inf), dict(mean=math.nan), dict(std=math.inf)):
    with pytest.raises(ValueError, match="finite"):
      ops.RateTable("poisson", **kw)


def test_image_set_and_rate_encode_argument_errors():
  import torch
  from snnquantprune_amd import ops
  s = ops.ImageSet(np.zeros((3, 2, 4), np.uint8))
  assert (s.num_samples, s.K, s.item_shape) == (3, 8, (2, 4)) and s.data.shape == (3, 8)
  e = ops.ImageSet(torch.zeros((0, 5), dtype=torch.uint8))
  assert (e.num_samples, e.K, e.item_shape) == (0, 5, (5,))
  for bad in (np.zeros((3, 4), np.float32), np.zeros((3, 4), np.int8), torch.zeros((3, 4))):
    with pytest.raises(ValueError, match="uint8"):
      ops.ImageSet(bad)
  table = ops.RateTable("bernoulli")
  for rows in ([3], [-1], [0, 1, 7]):
    with pytest.raises(ValueError, match="sample"):                             # before any launch
      ops.rate_encode(s, rows, 2, table, seed=0)
  with pytest.raises(ValueError, match="sample_id"):
    ops.rate_encode(s, [0, 1], 2, table, seed=0, sample_id=[4])
  with pytest.raises(ValueError, match="bernoulli"):
    ops.rate_encode(s, [0], 2, ops.RateTable("poisson"), seed=0, fmt="bits")
  with pytest.raises(ValueError, match="fmt"):
    ops.rate_encode(s, [0], 2, table, seed=0, fmt="ev4")


def test_entry_refusals_without_a_gpu():
  """snnqp_rate_encode's host checks: nothing is launched, so they answer without a device."""
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  p = ctypes.c_void_p(16)

  def call(B=2, T=3, K=5, kind=L.ENCODE_BERNOULLI, out_type=L.U8, ptr=p):
    return lib.snnqp_rate_encode(ptr, 4, ptr, ptr, B, T, K, 1, 0, ptr, kind, ptr, out_type, T * K, K, None)

  assert call(T=2 ** 16, K=2 ** 16, ptr=None) == L.EINVAL and b"T * K" in lib.snnqp_last_error()
  assert call(K=0) == L.EINVAL
  assert call(B=-1) == L.EINVAL
  assert call(kind=2) == L.EINVAL and b"kind" in lib.snnqp_last_error()
  assert call(out_type=L.EV4) == L.EINVAL and b"out_type" in lib.snnqp_last_error()
  assert call(kind=L.ENCODE_POISSON, out_type=L.BITS) == L.EINVAL and b"Poisson" in lib.snnqp_last_error()
  assert call(ptr=None) == L.EINVAL and b"null" in lib.snnqp_last_error()
  assert call(B=0, ptr=None) == L.OK and call(T=0, ptr=None) == L.OK            # nothing to write


# ---- the reference is a sound generator at the seeds the tests use -----------------------------------

S_GEN, T_GEN, K_GEN = 64, 32, 784
LIMIT = 5.0                                                                     # standard errors


def _spikes(p, seed=7, draw=0, ids=None):
  ids = np.arange(S_GEN) if ids is None else ids
  u = ec.hashes(seed, draw, ids, T_GEN, K_GEN)
  return (u.astype(np.float64) < math.floor(p * TOP)).astype(np.float64)


def _corr_z(a, b):
  """The sample correlation of two 0 / 1 arrays in standard errors (1 / sqrt(n) under independence)."""
  a, b = a.reshape(-1), b.reshape(-1)
  return float(np.corrcoef(a, b)[0, 1] * math.sqrt(a.size))


@pytest.mark.parametrize("p", [0.1 / 255, 0.1, 0.5, 0.9])
def test_reference_is_a_sound_generator(p):
  """A condition on the inputs, not a measurement of the kernel: at seed 7, 64 samples, T = 32,
  K = 784 the overall rate and the lag-1 correlations along k, along t, across consecutive
  sample ids, across draw 0 / 1 and across seed 7 / 8 all lie inside 5 standard errors (seen: within
  1.9).  Per-column rates are not asserted where n * p < 50: the normal approximation fails there."""
  s = _spikes(p)
  n = s.size
  q = math.floor(p * TOP) / TOP
  z = {"rate": (s.mean() - q) / math.sqrt(q * (1 - q) / n),
       "k": _corr_z(s[:, :, :-1], s[:, :, 1:]),
       "t": _corr_z(s[:, :-1], s[:, 1:]),
       "sample_id": _corr_z(s[:-1], s[1:]),
       "draw": _corr_z(s, _spikes(p, draw=1)),
       "seed": _corr_z(s, _spikes(p, seed=8))}
  print("p = %g:" % p, {k: round(v, 2) for k, v in z.items()})
  for k, v in z.items():
    assert abs(v) < LIMIT, (k, v)
  if S_GEN * T_GEN * p >= 50:                                                   # per-column rates
    col = s.mean((0, 1))
    zc = (col - q) / math.sqrt(q * (1 - q) / (S_GEN * T_GEN))
    print("  per-column rate: largest |z| %.2f of %d" % (np.abs(zc).max(), K_GEN))
    assert np.abs(zc).max() < LIMIT


def test_reference_poisson_mean_and_variance():
  table = np.tile(ec.table_reference("poisson", gain=0.7)[255], (256, 1))       # rate 0.7 for every pixel
  x = ec.rate_encode_reference(np.zeros((S_GEN, K_GEN), np.uint8), np.arange(S_GEN), np.arange(S_GEN), T_GEN,
                               table, "poisson", 7, 0).astype(np.float64)
  n = x.size
  z_mean = (x.mean() - 0.7) / math.sqrt(0.7 / n)
  # Var of the sample variance of a Poisson: (mu4 - sigma^4) / n with mu4 = r + 3 r^2
  z_var = (x.var() - 0.7) / math.sqrt((0.7 + 2 * 0.49) / n)
  print("poisson 0.7: mean %.5f (z %.2f), variance %.5f (z %.2f)" % (x.mean(), z_mean, x.var(), z_var))
  assert abs(z_mean) < LIMIT and abs(z_var) < LIMIT


def test_reference_packing():
  rng = np.random.default_rng(1)
  x = rng.integers(0, 2, (3, 2, 45)).astype(np.uint8)
  w = ec.pack_bits_reference(x)
  assert w.shape == (3, 2, 2) and w.dtype == np.int32
  for k in range(45):
    assert np.array_equal((w[..., k >> 5].view(np.uint32) >> np.uint32(k & 31)) & 1, x[..., k])
  assert (w[..., 1].view(np.uint32) >> np.uint32(13) == 0).all()                # the tail bits are zero


# ---- pipeline without a device -------------------------------------------------------------------------

def _cfg(**kw):
  return ec.make_config(**kw)


def test_load_source_image_dict_and_npz(tmp_path):
  from snnquantprune_amd import input_pipeline as ip
  src = ec.make_images(1, 6)
  src["label"] = src["label"].astype(np.int64)
  assert ip.is_image_source(src) and not ip.is_event_source(src)
  got = ip.load_source(src)
  assert set(got) == {"image", "label"} and got["label"].dtype == np.int8
  assert np.array_equal(got["image"], src["image"]) and np.array_equal(got["label"], src["label"])
  path = str(tmp_path / "images.npz")
  np.savez(path, **src)
  again = ip.load_source(path)
  assert np.array_equal(again["image"], src["image"]) and again["label"].dtype == np.int8
  # idempotent: the loop loads what it was handed
  assert ip.is_image_source(got) and np.array_equal(ip.load_source(got)["image"], src["image"])


def test_load_source_image_refusals():
  from snnquantprune_amd import input_pipeline as ip
  img = np.zeros((4, 8, 8), np.uint8)
  with pytest.raises(ValueError, match="uint8"):
    ip.load_source({"image": img.astype(np.float32), "label": np.zeros(4)})
  with pytest.raises(ValueError, match="one label per image"):
    ip.load_source({"image": img, "label": np.zeros(3)})
  with pytest.raises(ValueError, match="one label per image"):
    ip.load_source({"image": np.uint8(3), "label": np.zeros(1)})


def test_frame_source_still_raises_what_it_raised():
  from snnquantprune_amd import input_pipeline as ip
  from snnquantprune_amd import train
  frames = {"dvs_matrix": np.zeros((4, 3, 8, 8, 2), np.uint8), "label": np.zeros(4, np.int8)}
  assert not ip.is_image_source(frames)
  assert not ip.is_image_source(dict(frames, image=np.zeros((4, 8), np.uint8)))   # a dvs_matrix decides
  assert set(ip.load_source(frames)) == {"dvs_matrix", "label"}
  with pytest.raises(ValueError, match=r"dvs_matrix must be \[N, T, H, W, 2\]"):
    ip.load_source({"dvs_matrix": np.zeros((4, 8, 8, 2), np.uint8), "label": np.zeros(4)})
  with pytest.raises(NotImplementedError, match="the training split"):
    ip.create_split(frames, _cfg(), train=True, cache=False)
  with pytest.raises(NotImplementedError, match="the training split needs an event source"):
    train.train_and_evaluate(_cfg(), "/nonexistent", source=frames, device="cpu")


def test_image_plan_eval_repeats_itself():
  from snnquantprune_amd import input_pipeline as ip
  plan = ip.ImagePlan(_cfg(eval_batch_size=5), (8, 8), 32, train=False)
  assert (plan.per, plan.nb, plan.T, plan.K, plan.batch_shape) == (5, 6, 8, 64, (5, 8, 64))
  it = plan.batches()
  first = [next(it) for _ in range(6)]
  second = [next(it) for _ in range(6)]
  assert np.array_equal(np.concatenate([b[0] for b in first]), np.arange(30))    # in order, remainder dropped
  for (i0, s0, d0), (i1, s1, d1) in zip(first, second):
    assert np.array_equal(i0, i1) and np.array_equal(s0, s1) and d0 == d1 == 0
  # skip: modulo the pass
  it = plan.batches(skip=6 + 2)
  assert np.array_equal(next(it)[0], first[2][0])


def test_image_plan_train_permutes_and_skips():
  from snnquantprune_amd import input_pipeline as ip
  mk = lambda: ip.ImagePlan(_cfg(batch_size=6), (8, 8), 32, train=True)          # noqa: E731
  it = mk().batches()
  got = [next(it) for _ in range(15)]                                            # 5 batches an epoch
  epochs = [np.concatenate([b[0] for b in got[e * 5:(e + 1) * 5]]) for e in range(3)]
  for e, idx in enumerate(epochs):
    assert len(np.unique(idx)) == 30 and idx.min() >= 0 and idx.max() < 32       # once each, 2 dropped
    assert [b[2] for b in got[e * 5:(e + 1) * 5]] == [1 + e] * 5                 # draw = 1 + epoch
  assert not np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[1], epochs[2])
  for skip in (1, 5, 7):
    it = mk().batches(skip=skip)
    for want in got[skip:skip + 6]:
      idx, ids, draw = next(it)
      assert np.array_equal(idx, want[0]) and np.array_equal(ids, want[1]) and draw == want[2]
  # another seed, another order; the same seed, the same order
  other = next(ip.ImagePlan(_cfg(batch_size=6, seed=6), (8, 8), 32, train=True).batches())
  assert not np.array_equal(other[0], got[0][0])
  assert np.array_equal(next(mk().batches())[0], got[0][0])


@pytest.mark.parametrize("train", [False, True])
def test_image_plan_ids_are_global(train):
  from snnquantprune_amd import input_pipeline as ip
  cfg = _cfg(batch_size=8, eval_batch_size=8)
  for rank in (0, 1):
    plan = ip.ImagePlan(cfg, (8, 8), 20, train, rank, 2)
    assert plan.per == 4 and plan.lo == 20 * rank
    idx, ids, _ = next(plan.batches())
    assert np.array_equal(ids, 20 * rank + idx) and idx.max() < 20
  a = next(ip.ImagePlan(cfg, (8, 8), 20, True, 0, 2).batches())[0]
  b = next(ip.ImagePlan(cfg, (8, 8), 20, True, 1, 2).batches())[0]
  assert not np.array_equal(a, b)                                                # seeded seed + rank


def test_image_plan_refusals():
  from snnquantprune_amd import input_pipeline as ip
  from snnquantprune_amd import linen as nn
  plan = lambda train=False, shape=(8, 8), **kw: ip.ImagePlan(_cfg(**kw), shape, 32, train)   # noqa: E731
  with pytest.raises(ValueError, match="feed_format must be one of"):
    plan(feed_format="ev4")
  with pytest.raises(ValueError, match="feed_format 'bits' holds spikes: the training split needs feed_format 'u8'"):
    plan(True, feed_format="bits")
  with pytest.raises(ValueError, match="feed_format 'bits' holds spikes: encoding kind 'poisson' needs feed_format 'u8'"):
    plan(feed_format="bits")                                                     # (the fixture encodes Poisson counts)
  assert plan(feed_format="bits", encoding=nn.ConfigDict(kind="bernoulli")).fmt == "bits"
  with pytest.raises(ValueError, match="image_layout must be one of"):
    plan(image_layout="nchw")
  with pytest.raises(ValueError, match=r"image_layout 'frames' needs images of \[N, H, W, 2\]"):
    plan(image_layout="frames")
  assert plan(shape=(4, 4, 2), image_layout="frames").batch_shape == (16, 8, 4, 4, 2)
  for train in (False, True):
    with pytest.raises(ValueError, match="augment is for event sources"):
      plan(train, augment=nn.ConfigDict(flip_x=0.5))
  with pytest.raises(ValueError, match="encoding has unknown keys"):
    plan(encoding=nn.ConfigDict(kind="poisson", rate=2.0))
  with pytest.raises(ValueError, match="std"):
    plan(encoding=nn.ConfigDict(std=0.0))
  with pytest.raises(ValueError, match="needs at least 33 samples"):
    plan(eval_batch_size=33)
  # the default encoder is the reference's: Poisson counts at the pixel's own intensity
  cfg = _cfg()
  del cfg["encoding"]
  t = ip.ImagePlan(cfg, (8, 8), 32, False).table
  assert (t.kind, t.gain, t.mean, t.std) == ("poisson", 1.0, 0.0, 1.0)


def test_image_input_shape():
  from snnquantprune_amd import input_pipeline as ip
  flat = {"image": np.zeros((4, 8, 8), np.uint8), "label": np.zeros(4)}
  assert ip.image_input_shape(flat, _cfg()) == (1, 8, 64)
  frames = {"image": np.zeros((4, 6, 5, 2), np.uint8), "label": np.zeros(4)}
  assert ip.image_input_shape(frames, _cfg(image_layout="frames")) == (1, 8, 6, 5, 2)
  assert ip.image_input_shape(frames, _cfg()) == (1, 8, 60)


def test_fixture_can_be_learnt():
  """The float64 model on the plan's own batches, from lecun-normal weights: the epoch-mean loss
  falls.  (The GPU test replays the loop's own initial weights the same way.)"""
  import torch
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import train_utils as tu
  cfg = _cfg()
  src, _ = ec.sources()
  steps = ec.N_TRAIN // ec.BATCH
  key = torch.Generator()
  key.manual_seed(5)
  init = nn.lecun_normal()
  params = {}
  for i, shape in enumerate([(ec.SIDE * ec.SIDE, ec.HIDDEN), (ec.HIDDEN, ec.CLASSES * 10)]):
    params["QuantDense_%d" % i] = {"kernel": init(key, shape).cpu().numpy(), "DuQ_0": {"a": np.array([-1.0]), "c": np.array([-1.0])}}
  batches = [(x, y) for x, y, _, _ in ec.plan_batches(src, cfg, steps * cfg.num_epochs, train=True)]
  losses = ec.reference_losses(params, batches, tu.create_learning_rate_fn(cfg, cfg.learning_rate, steps))
  first, last = np.mean(losses[:steps]), np.mean(losses[-steps:])
  print("reference losses", [round(l, 4) for l in losses], "first epoch", first, "last epoch", last)
  assert np.isfinite(losses).all() and last < first
