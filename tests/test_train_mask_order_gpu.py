"""Which random numbers a seed gives the dropout masks of the three training forwards: the sown
masks against masks drawn here from dense_train.generator_of / dense_train.dropout_mask in the
documented order and shapes.  Every other check reads the masks back from the sown values, so a
forward that drew them in another order or shape would pass those and change every seeded run."""
import pytest
import torch

from tests import cextnet_train_reference as xr
from tests import conv_train_reference as cr
from tests.test_cextnet_train_gpu import _setup as _cext_setup
from tests.test_conv_train_gpu import _setup as _conv_setup
from tests.test_dense_train_gpu import _setup as _dense_setup
from tests.train_helpers import _run_train

pytestmark = pytest.mark.gpu

SEED = 1234
B, T, K, HIDDEN = 2, 3, 64, 32


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _dense(dev):
  """-> (model, variables, x, batch_stats, keep, mask shapes in drawing order)."""
  model, _, variables, x = _dense_setup(dev, True, T=T, B=B, K=K, hidden=HIDDEN, dropout=0.8)
  return model, variables, x, False, 0.8, [(B, T, K), (T, B, HIDDEN)]


def _conv(dev):
  model, _, variables, x = _conv_setup(dev, True)
  flat = cr.CHANNELS * (cr.HW >> cr.NBLOCKS) ** 2                # the raster behind the pools
  return model, variables, x, True, cr.KEEP, [(cr.T_STEPS, cr.BATCH, flat)]


def _cext(dev):
  model, _, variables, x = _cext_setup(dev, True)
  flat = xr.CHANNELS * (xr.HW >> xr.NCONV) ** 2
  return model, variables, x, True, xr.KEEP, [(xr.T_STEPS, xr.BATCH, flat),
                                              (xr.T_STEPS, xr.BATCH, xr.CHANNELS * 2 * 2)]


MODELS = {"dense": _dense, "conv": _conv, "cext": _cext}


def _sown_masks(model, variables, x, rng, batch_stats, n):
  inter = _run_train(model, variables, x, rng=rng, batch_stats=batch_stats)[2]
  assert sum(k.startswith("dropout_") for k in inter) == n
  return [inter["dropout_%d" % i] for i in range(n)]


def _drawn(gen, shapes, keep, dev):
  from snnquantprune_amd import dense_train as dt
  return [dt.dropout_mask(s, keep, gen, dev) for s in shapes]


@pytest.mark.parametrize("name", list(MODELS))
def test_seed_gives_the_documented_masks(dev, name):
  from snnquantprune_amd import dense_train as dt
  model, variables, x, batch_stats, keep, shapes = MODELS[name](dev)
  got = _sown_masks(model, variables, x, SEED, batch_stats, len(shapes))
  want = _drawn(dt.generator_of(SEED, dev), shapes, keep, dev)
  for i, (g, w) in enumerate(zip(got, want)):
    assert tuple(g.shape) == tuple(w.shape), i
    assert 0.0 < float(w.mean()) < 1.0, i                        # a mask that says something
    assert torch.equal(g, w), "dropout_%d" % i


@pytest.mark.parametrize("name", list(MODELS))
def test_generator_is_advanced(dev, name):
  from snnquantprune_amd import dense_train as dt
  model, variables, x, batch_stats, keep, shapes = MODELS[name](dev)
  gen = dt.generator_of(SEED, dev)
  first = _sown_masks(model, variables, x, gen, batch_stats, len(shapes))
  second = _sown_masks(model, variables, x, gen, batch_stats, len(shapes))
  ref = dt.generator_of(SEED, dev)
  want = _drawn(ref, shapes, keep, dev) + _drawn(ref, shapes, keep, dev)
  for i, (g, w) in enumerate(zip(first + second, want)):
    assert torch.equal(g, w), "call %d, dropout_%d" % divmod(i, len(shapes))
  for i, (a, b) in enumerate(zip(first, second)):
    assert not torch.equal(a, b), "dropout_%d" % i
