"""ops.rate_encode (snnqp_rate_encode, csrc/encode.hip) on the GPU, bit for bit against the numpy
reference of tests/encode_cases.py: shapes at the unit and word edges, both kinds, both formats,
both orders and strided rows inside a sentinel frame, the tables' ends, independence of the batch,
the entry's refusals, and DenseSNN on the bits batch."""
import numpy as np
import pytest
import torch

from tests import encode_cases as ec

pytestmark = pytest.mark.gpu

SEED, DRAW = 7, 3
BYTE, WORD = 0xA5, 0x5A5A5A5A


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _images(S, K, seed=1):
  """Every byte value occurs: row 0 counts 0, 1, 2, ... and the rest is random."""
  rng = np.random.default_rng(seed)
  x = rng.integers(0, 256, (S, K)).astype(np.uint8)
  x[0] = np.arange(K) % 256
  x[-1] = 255 - np.arange(K) % 256
  return x


def _rows(S, B):
  """Repeats, descending order and the set's last row."""
  return np.array([S - 1 - (i * 3) % S if i % 4 else S - 1 for i in range(B)], np.int64)


_tables = {}


def _table(kind, **kw):
  from snnquantprune_amd import ops
  key = (kind, tuple(sorted(kw.items())))
  if key not in _tables:
    _tables[key] = ops.RateTable(kind, **kw)
  return _tables[key]


def _raw(dev, images, rows, ids, T, table, kind, bits, time_major, gap, seed=SEED, draw=DRAW):
  """The entry point on rows `gap` units apart inside a frame of sentinels -> (the [B, T, unit] rows
  as numpy, batch-major whatever the order written; whether every sentinel is untouched)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  S, K = images.shape
  B = len(rows)
  unit = (K + 31) // 32 if bits else K
  pitch = unit + gap
  pad = 64 + (1 if gap and not bits else 0)            # uint8 rows apart: the first one at an odd address
  n = B * T * pitch
  whole = torch.full((n + 2 * pad,), WORD if bits else BYTE, dtype=torch.int32 if bits else torch.uint8, device=dev)
  os_t, os_b = (B * pitch, pitch) if time_major else (pitch, T * pitch)
  img = torch.from_numpy(images).to(dev)
  r = torch.from_numpy(np.asarray(rows, np.int32)).to(dev)
  i = torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32)).to(dev)
  out = whole[pad:]
  L.check(L.lib().snnqp_rate_encode(
      ops._ptr(img), S, ops._ptr(r), ops._ptr(i), B, T, K, seed, draw, ops._ptr(table.on(dev)),
      L.ENCODE_POISSON if kind == "poisson" else L.ENCODE_BERNOULLI, ops._ptr(out),
      L.BITS if bits else L.U8, os_b, os_t, ops._stream()))
  torch.cuda.synchronize()
  w = whole.cpu().numpy()
  body = w[pad:pad + n].reshape((T, B, pitch) if time_major else (B, T, pitch))
  got = body[..., :unit]
  if time_major:
    got = np.swapaxes(got, 0, 1)
  sentinel = np.int32(WORD) if bits else np.uint8(BYTE)
  clean = (w[:pad] == sentinel).all() and (w[pad + n:] == sentinel).all() and (body[..., unit:] == sentinel).all()
  return np.ascontiguousarray(got), bool(clean)


def _check_all_forms(dev, S, B, T, K, gaps=(0, 3)):
  images, rows = _images(S, K), _rows(S, B)
  ids = rows + 1000
  for kind, kw in (("poisson", dict(gain=2.0)), ("bernoulli", dict(gain=0.9))):
    table = _table(kind, **kw)
    want = ec.rate_encode_reference(images, rows, ids, T, table.entries, kind, SEED, DRAW)
    for time_major in (False, True):
      for gap in gaps:
        got, clean = _raw(dev, images, rows, ids, T, table, kind, False, time_major, gap)
        np.testing.assert_array_equal(got, want, err_msg="%s u8 tm=%s gap=%d" % (kind, time_major, gap))
        assert clean, "%s u8 tm=%s gap=%d wrote outside its rows" % (kind, time_major, gap)
        if kind == "bernoulli":
          got, clean = _raw(dev, images, rows, ids, T, table, kind, True, time_major, min(gap, 1))
          np.testing.assert_array_equal(got, ec.pack_bits_reference(want),
                                        err_msg="bits tm=%s gap=%d" % (time_major, gap))
          assert clean, "bits tm=%s gap=%d wrote outside its rows" % (time_major, gap)


# ---- 1. shapes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 3, 31, 32, 33, 63, 64, 65, 127, 784, 2049])
def test_row_lengths(dev, K):
  _check_all_forms(dev, S=5, B=3, T=2, K=K)


@pytest.mark.parametrize("T", [0, 1, 2, 33])
@pytest.mark.parametrize("B", [0, 1, 3, 70])
def test_steps_and_rows(dev, T, B):
  _check_all_forms(dev, S=7, B=B, T=T, K=65, gaps=(0, 1))


def test_many_units_many_steps(dev):
  """More than 256 units a row and more steps than a chunk: the unit loop and the chunk edge."""
  _check_all_forms(dev, S=3, B=2, T=33, K=2049, gaps=(1,))
  _check_all_forms(dev, S=4, B=70, T=33, K=127, gaps=(0,))


# ---- 2. ops.rate_encode: formats and orders ------------------------------------------------------------

@pytest.mark.parametrize("K", [33, 784])
def test_ops_forms(dev, K):
  from snnquantprune_amd import ops
  S, B, T = 6, 5, 3
  images, rows = _images(S, K), _rows(S, B)
  s = ops.ImageSet(images.reshape(S, K, 1), device=dev)
  assert s.item_shape == (K, 1) and s.K == K
  for kind in ("poisson", "bernoulli"):
    table = _table(kind, gain=0.8)
    want = ec.rate_encode_reference(images, rows, rows, T, table.entries, kind, SEED, DRAW)
    got = ops.rate_encode(s, rows, T, table, seed=SEED + 2 ** 32, draw=DRAW - 2 ** 32)   # modulo 2^32
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, T, K)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    tm = ops.rate_encode(s, torch.from_numpy(rows), T, table, seed=SEED, draw=DRAW, time_major=True)
    np.testing.assert_array_equal(tm.cpu().numpy(), np.swapaxes(want, 0, 1))
    if kind == "bernoulli":
      assert set(np.unique(want)) == {0, 1}
      for time_major in (False, True):
        bits = ops.rate_encode(s, rows, T, table, seed=SEED, draw=DRAW, fmt="bits", time_major=time_major)
        u8 = tm if time_major else got
        assert isinstance(bits, ops.PackedSpikes) and bits.shape == tuple(u8.shape)
        # word for word ops.pack_bits of the u8 result, the tail bits of the last word zero
        assert torch.equal(bits.bits, ops.pack_bits(u8).bits)
        np.testing.assert_array_equal(bits.bits.cpu().numpy(), ec.pack_bits_reference(u8.cpu().numpy()))
        assert torch.equal(bits.to_dense().to(torch.uint8), u8)
  # nothing to encode
  assert tuple(ops.rate_encode(s, [], T, table, seed=1).shape) == (0, T, K)
  assert tuple(ops.rate_encode(s, rows, 0, table, seed=1, fmt="bits").bits.shape) == (B, 0, (K + 31) // 32)
  assert ops.device_status() == 0


# ---- 3. tables -----------------------------------------------------------------------------------------

def test_table_ends(dev):
  from snnquantprune_amd import ops
  S, T = 4, 5
  images = _images(S, 300)
  images[1] = 255                                            # white
  s = ops.ImageSet(images, device=dev)
  rows = np.arange(S)
  for kind in ("poisson", "bernoulli"):
    assert int(ops.rate_encode(s, rows, T, _table(kind, gain=0.0), seed=SEED).max()) == 0      # gain 0: all zero
  ones = ops.rate_encode(s, rows, T, _table("bernoulli", gain=1.5), seed=SEED)
  assert int(ones[1].min()) == 1                             # gain >= 1 on white pixels: all one
  np.testing.assert_array_equal(
      ones.cpu().numpy(), ec.rate_encode_reference(images, rows, rows, T, _table("bernoulli", gain=1.5).entries,
                                                   "bernoulli", SEED, 0))
  bits = ops.rate_encode(s, rows, T, _table("bernoulli", gain=1.5), seed=SEED, fmt="bits")
  assert (bits.bits[1, :, :-1] == -1).all() and (bits.bits[1, :, -1] == (1 << (300 - 288)) - 1).all()
  # a rate of 6 on white pixels: the cap at 15 and every count below it are reached
  six = _table("poisson", gain=6.0)
  big = ops.ImageSet(np.full((2, 50000), 255, np.uint8), device=dev)
  got = ops.rate_encode(big, [0, 1], 4, six, seed=SEED).cpu().numpy()
  np.testing.assert_array_equal(
      got, ec.rate_encode_reference(np.full((2, 50000), 255, np.uint8), [0, 1], [0, 1], 4, six.entries, "poisson", SEED, 0))
  assert set(np.unique(got)) == set(range(16))
  assert 0 < six.truncated_mass < 1e-3


def test_hand_made_thresholds(dev):
  """Tables nobody's rates produce: 2^32 - 1 stands for 2^32 in both kinds, thresholds need not grow."""
  from snnquantprune_amd import ops
  rng = np.random.default_rng(5)
  entries = rng.integers(0, 2 ** 32, (256, 16), dtype=np.uint64)
  entries[:, 15] = 0
  entries[::3, 0] = 2 ** 32 - 1
  entries[1::5, 7] = 2 ** 32 - 1
  entries[2::7, 3] = 0
  images, rows = _images(3, 513), np.array([2, 0, 1])
  s = ops.ImageSet(images, device=dev)
  for kind in ("poisson", "bernoulli"):
    table = ops.RateTable(kind)
    table.entries = entries.astype(np.uint32)
    want = ec.rate_encode_reference(images, rows, rows, 6, table.entries, kind, SEED, DRAW)
    np.testing.assert_array_equal(ops.rate_encode(s, rows, 6, table, seed=SEED, draw=DRAW).cpu().numpy(), want)


# ---- 4. independence -------------------------------------------------------------------------------------

def test_value_depends_on_id_step_and_element_alone(dev):
  from snnquantprune_amd import ops
  S, K, T = 80, 130, 9
  images = _images(S, K, seed=2)
  s = ops.ImageSet(images, device=dev)
  table = _table("poisson", gain=1.5)
  enc = lambda rows, **kw: ops.rate_encode(s, rows, T, table, **dict(dict(seed=SEED, draw=DRAW), **kw)).cpu().numpy()   # noqa: E731
  alone = enc([41])[0]
  rng = np.random.default_rng(0)
  order = rng.permutation(S)[:70]
  order[13] = 41
  batch = enc(order)
  np.testing.assert_array_equal(batch[13], alone)                              # in a batch of 70
  again = enc(order[::-1].copy())
  np.testing.assert_array_equal(again[70 - 1 - 13], alone)                     # at another position
  np.testing.assert_array_equal(again[::-1], batch)                            # another order, the same rows
  first = enc(np.concatenate([[41], order[:5]]))
  np.testing.assert_array_equal(first[0], alone)
  # draw and seed change the result
  assert (enc([41], draw=DRAW + 1)[0] != alone).mean() > 0.2
  assert (enc([41], seed=SEED + 1)[0] != alone).mean() > 0.2
  # sample_id overrides sample in the key only: row 41's pixels under id 7 ...
  moved = enc([41], sample_id=[7])[0]
  np.testing.assert_array_equal(
      moved, ec.rate_encode_reference(images, [41], [7], T, table.entries, "poisson", SEED, DRAW)[0])
  assert (moved != alone).mean() > 0.2
  # ... and a slice of the set under the ids of the whole set is the whole set's rows
  part = ops.ImageSet(images[40:], device=dev)
  got = ops.rate_encode(part, [1, 0], T, table, seed=SEED, draw=DRAW, sample_id=[41, 40]).cpu().numpy()
  np.testing.assert_array_equal(got[0], alone)
  np.testing.assert_array_equal(got[1], enc([40])[0])
  # ids modulo 2^32
  np.testing.assert_array_equal(enc([41], sample_id=[41 + 2 ** 32])[0], alone)


def test_out_of_range_row_is_an_image_of_zeros(dev):
  """The host refuses such a row (ops.rate_encode); the kernel's own guard reads nothing for it."""
  images = np.full((2, 40), 255, np.uint8)
  table = _table("bernoulli", gain=1.5)
  got, clean = _raw(dev, images, [0, 2, -1, 1], [0, 1, 2, 3], 3, table, "bernoulli", False, False, 0)
  assert clean and got[0].min() == 1 and got[3].min() == 1 and got[1].max() == 0 and got[2].max() == 0


# ---- 5. the entry's refusals ---------------------------------------------------------------------------

def test_entry_refusals(dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  lib = L.lib()
  buf = torch.zeros(4096, dtype=torch.int32, device=dev)
  p = ops._ptr(buf)

  def call(B=2, T=3, K=5, kind=L.ENCODE_BERNOULLI, out_type=L.U8, ptr=p):
    return lib.snnqp_rate_encode(ptr, 4, ptr, ptr, B, T, K, 1, 0, ptr, kind, ptr, out_type, T * K, K, ops._stream())

  assert call(T=2 ** 16, K=2 ** 16, ptr=None) == L.EINVAL                      # by arguments alone
  assert call(T=2 ** 31 - 1, K=3, ptr=None) == L.EINVAL
  assert call(kind=L.ENCODE_POISSON, out_type=L.BITS) == L.EINVAL
  assert call(kind=7) == L.EINVAL
  assert call(out_type=L.F32) == L.EINVAL
  assert call(K=0) == L.EINVAL
  assert call(ptr=None) == L.EINVAL
  assert call(B=0, ptr=None) == L.OK and call(T=0, ptr=None) == L.OK
  torch.cuda.synchronize()
  assert int(buf.abs().max()) == 0                                             # nothing was launched
  assert ops.device_status() == 0


# ---- 6. the model sees the same thing ------------------------------------------------------------------

def test_dense_snn_on_bits_equals_u8(dev):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, synthetic as syn
  B, T, K, hidden = 6, 5, 200, 160
  v = nn.tree_from_numpy(syn.dense_net_variables(K, hidden, 110, True, 0.5), dev)
  model = models.DenseSNN(num_classes=11, config=syn.make_config(bits=8, prune_percentage=0.5, hidden=hidden))
  s = ops.ImageSet(_images(8, K, seed=3), device=dev)
  table = _table("bernoulli", gain=0.6)
  rows = _rows(8, B)
  u8 = ops.rate_encode(s, rows, T, table, seed=SEED)
  bits = ops.rate_encode(s, rows, T, table, seed=SEED, fmt="bits")
  (a, _) = model.apply(v, u8, trgt=None, train=False, rng=None)
  (b, _) = model.apply(v, bits, trgt=None, train=False, rng=None)
  torch.cuda.synchronize()
  print("input rate %.3f, largest logit %.4f" % (float(u8.float().mean()), float(a.abs().max())))
  assert tuple(a.shape) == (B, 11) and 0.1 < float(u8.float().mean()) < 0.5
  assert torch.equal(a, b)
  assert ops.device_status() == 0
