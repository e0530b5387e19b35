"""CPU suite: the half group of the event layer -- a numpy model of the operands
the wave of the last channel group hands to v_mfma_i32_32x32x32_i8 on the half path
(conv3x3_u8c2.hip, template parameter HALF), the assembly of its spike words, and the host plan
that decides `snnqp_weight_t.cout_fire`."""
import numpy as np
import pytest

from snnquantprune_amd import packing, prune_utils as pu, synthetic as syn

HALO = 10


# ---- the operands, as the kernel places them ------------------------------------------------
# k = 16 h + j is the k index lane half h holds in its 16 operand bytes (A: row m, B: column n).

def a_source(m, k):
  """A operand of row m: (halo row, halo column, cin) of the byte at k.  The 32 rows are the
  patch's even image rows Y = 2 ty x 8 columns; halo row r is image row r - 1."""
  ty = ((m >> 2) & 1) | ((m >> 4) << 1)
  tx = (m & 3) | (((m >> 3) & 1) << 2)
  b = k & 7                                   # the 8 bytes that start at pixel tx of a halo row
  return 2 * ty + (k >> 3), tx + (b >> 1), b & 1


def b_source(n, k):
  """B operand of column n: (channel of the half group, dy, dx, cin) of the code at k, or None for
  a zero.  Columns n >= 16 hold the channel of column n - 16 with its taps one halo row lower."""
  kk = k - 8 if n >= 16 else k
  if not 0 <= kk < 24 or (kk & 7) >= 6:
    return None
  return n & 15, kk >> 3, (kk & 7) >> 1, kk & 1


def d_row(i, h):
  """Row m of the product that register i holds in lane half h."""
  return (i & 3) + 4 * h + 8 * (i >> 2)


def pixel_of(i, n, h):
  """(image row, column) within the 8x8 patch of register i in lane (n, h)."""
  m = d_row(i, h)
  y, _, _ = a_source(m, 0)
  tx = (m & 3) | (((m >> 3) & 1) << 2)
  return y + (n >> 4), tx


def test_every_pixel_and_channel_meets_its_18_taps_once():
  seen = set()
  for i in range(16):
    for h in range(2):
      for n in range(32):
        Y, X = pixel_of(i, n, h)
        assert (i & 7) == X
        seen.add((Y, X, n & 15))
        m = d_row(i, h)
        met, zeros = [], 0
        for k in range(32):
          src, code = a_source(m, k), b_source(n, k)
          assert src[0] <= HALO - 1                        # the last halo row used is 9
          if code is None:
            zeros += 1
            continue
          ch, dy, dx, cin = code
          assert ch == n & 15
          # the tap (dy, dx, cin) of the pixel (Y, X) reads halo pixel (Y + dy, X + dx)
          assert src == (Y + dy, X + dx, cin), (i, n, h, k)
          met.append((dy, dx, cin))
        assert sorted(met) == sorted((dy, dx, c) for dy in range(3) for dx in range(3) for c in range(2))
        assert zeros == 14                                # 8 unused k rows + 3 x 2 neighbour-pixel bytes
  assert len(seen) == 64 * 16                             # every pixel of the patch x every channel, once


def test_product_is_the_convolution_at_both_pixels():
  r = np.random.Generator(np.random.PCG64(5))
  codes = r.integers(-7, 8, size=(3, 3, 2, 16))
  halo = r.integers(0, 2, size=(HALO, HALO + 2, 2)) * 16  # (a 24-byte LDS row holds 12 pixels)
  base = r.integers(1000, 5000, size=32)                   # the C operand: one table address per lane
  for i in range(16):
    for h in range(2):
      m = d_row(i, h)
      a = np.array([halo[a_source(m, k)] for k in range(32)])
      for n in range(32):
        b = np.array([0 if b_source(n, k) is None else 8 * codes[b_source(n, k)[1:] + (n & 15,)]
                      for k in range(32)])
        Y, X = pixel_of(i, n, h)
        acc = int((halo[Y:Y + 3, X:X + 3] // 16 * codes[..., n & 15]).sum())
        assert base[n] + int(a @ b) == base[n] + 128 * acc     # 128 B of table per unit of accumulator


def _masks(s):
  """The 64-bit compare mask of every register from spikes s[8, 8, 16] (row, column, channel)."""
  out = []
  for i in range(16):
    v = 0
    for h in range(2):
      for n in range(32):
        Y, X = pixel_of(i, n, h)
        v |= int(s[Y, X, n & 15]) << (32 * h + n)
    out.append(v)
  return out


def test_spike_words_against_a_direct_or():
  r = np.random.Generator(np.random.PCG64(9))
  s = r.random((8, 8, 16)) < 0.3
  word = lambda px: sum(int(b) << c for c, b in enumerate(px))
  m = _masks(s)
  # without pool: field r of register i = pixel (4 g + r, i & 7), stored by lane row * 8 + column
  lanes = {}
  for i in range(16):
    g = i >> 3
    for f in range(4):
      lanes[(4 * g + f) * 8 + (i & 7)] = (m[i] >> (16 * f)) & 0xFFFF
  assert sorted(lanes) == list(range(64))
  for lane, w in lanes.items():
    assert w == word(s[lane >> 3, lane & 7]) and w >> 16 == 0
  # with pool: a register pair's columns and a lane half's row pair are one 2x2 window
  pooled = {}
  for i in range(0, 16, 2):
    g, j = i >> 3, (i >> 1) & 3
    o = m[i] | m[i + 1]
    lo, hi = o & 0xFFFFFFFF, o >> 32
    pooled[8 * g + j] = (lo | lo >> 16) & 0xFFFF
    pooled[8 * g + 4 + j] = (hi | hi >> 16) & 0xFFFF
  assert sorted(pooled) == list(range(16))
  for lane, w in pooled.items():
    py, px = lane >> 2, lane & 3
    ref = s[2 * py:2 * py + 2, 2 * px:2 * px + 2].reshape(4, 16).any(0)
    assert w == word(ref)


# ---- the host plan ----------------------------------------------------------------------------

@pytest.mark.parametrize("live,fire", [(1, 16), (15, 16), (16, 16), (17, 0), (32, 0), (33, 48), (48, 48),
                                       (79, 80), (80, 80), (81, 0), (112, 112), (113, 0), (128, 0)])
def test_cout_fire_of_a_live_count(live, fire):
  lv = np.zeros(128, bool)
  lv[np.random.Generator(np.random.PCG64(live)).permutation(128)[:live]] = True
  idx = pu.computed_channels(lv)
  assert lv[idx[:live]].all() and not lv[idx[live:]].any()       # live first: what cout_fire rests on
  got = pu.half_group_fire(live, idx.size)
  assert got == fire
  assert (got != 0) == (1 <= live % 32 <= 16)
  if got:
    assert got % 16 == 0 and got + 16 == idx.size and idx.size % 32 == 0 and live <= got


def test_slot_ranges_take_the_larger_of_padding_channel_and_twin():
  r = np.random.Generator(np.random.PCG64(2))
  own = r.integers(0, 40, size=96)
  got = packing.half_group_ranges(own, 80)
  np.testing.assert_array_equal(got[:80], own[:80])
  np.testing.assert_array_equal(got[80:], np.maximum(own[80:], own[64:80]))
  # nothing changes without the half group: no cout_fire, or padding that is not the last 16
  np.testing.assert_array_equal(packing.half_group_ranges(own, 0), own)
  np.testing.assert_array_equal(packing.half_group_ranges(own, 64), own)
  np.testing.assert_array_equal(packing.half_group_ranges(own, 96), own)
  # one slot table for both paths: every slot at least as tall as either table it may hold
  slots, stack = packing.table_slots(got)
  col = np.zeros(32, np.int64)
  np.add.at(col, slots[:96] >> 2, got)
  assert stack == col.max() and len(set(slots[:96].tolist())) == 96


def _event_layer(p, bits, layer_bits=None):
  cfg = syn.make_config(bits=bits, prune_percentage=p)
  if layer_bits is not None:
    cfg.quant.layer_bits = list(layer_bits)
  v = syn.conv_net_variables(prune_p=p, random_bn=False)
  live = pu.conv_net_liveness(v, cfg, 1)[0]
  b0 = bits if layer_bits is None else layer_bits[0]
  codes = pu._host_codes(v["params"]["QuantConv_0"], b0)[0]
  idx = pu.computed_channels(live)
  return int(live.sum()), idx, np.abs(codes[..., idx]).reshape(-1, idx.size).sum(0)


def test_c3_takes_the_half_group_at_the_same_table_height():
  live, idx, ranges = _event_layer(0.9, 4)
  assert (live, idx.size) == (79, 96)
  fire = pu.half_group_fire(live, idx.size)
  assert fire == 80
  _, before = packing.table_slots(ranges)
  _, stack = packing.table_slots(packing.half_group_ranges(ranges, fire))
  assert before == 47 and stack == 47                     # 51 rows, 6.4 KB: the sixth workgroup stays


def test_c5_and_8bit_do_not():
  live, idx, _ = _event_layer(0.95, 4, (2, 4, 2, 4))
  assert (live, idx.size) == (54, 64) and pu.half_group_fire(live, idx.size) == 0
  live, idx, _ = _event_layer(0.3, 8)
  assert (live, idx.size) == (128, 128) and pu.half_group_fire(live, idx.size) == 0
