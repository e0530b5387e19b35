"""CPU suite: the quarter of the half group on a 16x16x64 matrix instruction (DESIGN.md 4.2;
conv3x3_u8c2.hip, template parameter Q16) -- a numpy model of the operand placement as the kernel makes
it: which (channel, pixel) every (wave, lane, register) updates, the pool blocks, the LDS banks of the
table gathers, the lanes that store word 2 of a (pooled) pixel, the bytes of A and B that meet, and the
truth table of the predicate snnqp_conv_event_quarter16."""
import ctypes
import itertools

import numpy as np
import pytest

HALO, HROW2 = 10, 24
HCOPY2 = HALO * HROW2
HIMG2 = 496


# ---- the placement, as the kernel makes it ---------------------------------------------------
# v_mfma_i32_16x16x64_i8: lane l of A holds row l & 15, of B column l & 15, both the 16 k bytes of
# lane group l >> 4; lane l of D holds column l & 15, register i = row 4 (l >> 4) + i.

def quarter_pixel(w, r):
  """(image row, column) inside the 8x8 patch of A row r of wave w (conv3x3_u8c2.hip: py, px)."""
  g, q = w >> 1, w & 1
  return 4 * g + 2 * (r >> 3) + ((r >> 1) & 1), 4 * q + 2 * ((r >> 2) & 1) + (r & 1)


def updates(w, lane, i):
  """(channel, image row, column) that register i of `lane` of wave w updates."""
  y, x = quarter_pixel(w, 4 * (lane >> 4) + i)
  return 64 + (lane & 15), y, x


def test_every_channel_and_pixel_of_the_half_group_has_exactly_one_updater():
  got = [updates(w, lane, i) for w in range(4) for lane in range(64) for i in range(4)]
  want = set(itertools.product(range(64, 80), range(8), range(8)))
  assert len(got) == len(want) == 16 * 64
  assert set(got) == want
  for w in range(4):                                        # a wave's quarter: rows 4 g ..+3, columns 4 q ..+3
    g, q = w >> 1, w & 1
    px = {updates(w, lane, i)[1:] for lane in range(64) for i in range(4)}
    assert px == set(itertools.product(range(4 * g, 4 * g + 4), range(4 * q, 4 * q + 4)))


def test_the_four_registers_of_a_lane_are_one_pool_block():
  for w in range(4):
    for lane in range(64):
      px = [updates(w, lane, i)[1:] for i in range(4)]
      y0, x0 = px[0]
      assert y0 % 2 == 0 and x0 % 2 == 0
      assert px == [(y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)]
      assert len({updates(w, lane, i)[0] for i in range(4)}) == 1


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_gather_touches_thirty_two_banks_per_thirty_two_lanes(seed):
  """Lane groups 0 and 2 read the channel's own table column, 1 and 3 the twin slot sixteen channels up
  (tab0 of lane n = lane & 31: the entry of channel 64 + n), with the host's slots and with the default."""
  from snnquantprune_amd import packing
  r = np.random.Generator(np.random.PCG64(4100 + seed))
  ranges = r.integers(1, 60, 96)
  ranges[80:] = r.integers(0, 3, 16)
  host, _ = packing.table_slots(packing.half_group_ranges(ranges, 80))
  default = np.array([4 * (c & 31) + (c >> 5) for c in range(128)])
  for slots in (host, default):
    for half in range(2):
      cols = []
      for lane in range(32 * half, 32 * half + 32):
        chan = 64 + (lane & 15) + 16 * ((lane >> 4) & 1)      # own, or the twin's slot
        cols.append(int(slots[chan]) >> 2)
      assert len(set(cols)) == 32


# ---- who stores word 2 ------------------------------------------------------------------------

def place_words(pool, m):
  """place_words_quarter16 (conv_tile.h): lane -> 16-bit word, from the four 64-bit compare masks."""
  lanes = {}
  if pool:
    o = m[0] | m[1] | m[2] | m[3]
    for gq in range(4):
      lanes[4 * (gq >> 1) + (gq & 1)] = (o >> (16 * gq)) & 0xFFFF
  else:
    for i in range(4):
      for gq in range(4):
        lanes[4 * (2 * (gq >> 1) + (i >> 1)) + 2 * (gq & 1) + (i & 1)] = (m[i] >> (16 * gq)) & 0xFFFF
  return lanes


def store_plan(pool, w):
  """[(lane, ring word index)] of a wave's stores of word 2 (conv3x3_u8c2.hip: ob1, quarter_lane)."""
  g, q = w >> 1, w & 1
  out = []
  for lane in range(64):
    if (lane < 8 and (lane & 2) == 0) if pool else lane < 16:
      pix = ((2 * g + ((lane >> 2) & 1)) * 4 + 2 * q + (lane & 1) if pool
             else (4 * g + ((lane >> 2) & 3)) * 8 + 4 * q + (lane & 3))
      out.append((lane, pix * 4 + 2))
  return out


@pytest.mark.parametrize("pool", [False, True])
def test_every_stored_word_has_one_writer_and_is_the_raster(pool):
  r = np.random.Generator(np.random.PCG64(12))
  s = r.random((8, 8, 80)) < 0.3
  ring = {}
  for w in range(4):
    m = []
    for i in range(4):
      v = 0
      for lane in range(64):
        c, y, x = updates(w, lane, i)
        v |= int(s[y, x, c]) << lane
      m.append(v)
    lanes = place_words(pool, m)
    plan = store_plan(pool, w)
    assert sorted(lanes) == sorted(l for l, _ in plan)      # every written lane is stored, and no other
    for lane, o in plan:
      assert o not in ring
      ring[o] = lanes[lane]
  npix = 16 if pool else 64
  assert sorted(ring) == [p * 4 + 2 for p in range(npix)]
  word = lambda bits: sum(int(b) << c for c, b in enumerate(bits))
  for pix in range(npix):
    if pool:
      py, px = pix >> 2, pix & 3
      bits = s[2 * py:2 * py + 2, 2 * px:2 * px + 2].reshape(4, 80).any(0)
    else:
      bits = s[pix >> 3, pix & 7]
    assert ring[pix * 4 + 2] == word(bits[64:80])


# ---- the bytes of A and B that meet -------------------------------------------------------------

def tap_row(kk):
  """tap_row (conv3x3_u8c2.hip): the HWIO weight row of k row kk, or None."""
  return 6 * (kk >> 3) + (kk & 7) if 0 <= kk < 24 and (kk & 7) < 6 else None


def b_bytes(codes, c, kb):
  """The 16 bytes of B lane (c, kb): codes [18, 16] of channels 64..79, x 8."""
  out = np.zeros(16, np.int64)
  for j in range(16):
    row = tap_row(16 * kb + j)
    if row is not None:
      out[j] = 8 * codes[row, c]
  return out


def a_offset(w, lane):
  """offA[1] relative to the timestep image, and the pixel it belongs to."""
  y, x = quarter_pixel(w, lane & 15)
  kb = lane >> 4
  cq = x & 1
  return cq * HCOPY2 + 2 * x + 2 * cq + (y + 2 * (kb & 1)) * HROW2, y, x


def test_a_and_b_agree_on_every_tap_and_every_other_b_byte_is_zero():
  # B: the 18 taps once each over lane groups 0 and 1, zeros elsewhere
  codes = np.arange(1, 18 * 16 + 1).reshape(18, 16)           # every (row, channel) its own value
  for c in range(16):
    seen = {}
    for kb in range(4):
      for j, v in enumerate(b_bytes(codes, c, kb)):
        if v:
          seen[(kb, j)] = v // 8
    assert sorted(seen.values()) == sorted(codes[:, c])
    assert all(kb < 2 for kb, _ in seen) and len(seen) == 18
  # A: byte j of lane group kb is halo pixel (dy, dx), polarity cin of the lane's pixel -- read out of
  # the LDS image as the staging writes it (copy c: pixel hx at byte 2 hx + 2 c of a 24-byte row) --
  # wherever B holds a tap, and the weight row is that tap's
  r = np.random.Generator(np.random.PCG64(13))
  halo = r.integers(0, 2, (2, HALO, HALO, 2)) * 16             # two timesteps: reads may run into the next image
  lds = r.integers(0, 256, 2 * HIMG2 + 64)                     # what no tap may meet: noise
  for t in range(2):
    for cp in range(2):
      for hy in range(HALO):
        for hx in range(HALO):
          at = t * HIMG2 + cp * HCOPY2 + hy * HROW2 + 2 * hx + 2 * cp
          lds[at:at + 2] = halo[t, hy, hx]
  for w in range(4):
    for lane in range(64):
      off, y, x = a_offset(w, lane)
      assert off % 4 == 0                                      # a 4-byte-aligned ds_read2_b32
      kb = lane >> 4
      a = np.concatenate([lds[off:off + 8], lds[off + HROW2:off + HROW2 + 8]])
      assert a.size == 16 and off + HROW2 + 8 <= HIMG2 + 32     # inside this image or the next bytes
      for j in range(16):
        row = tap_row(16 * kb + j)
        if row is None:
          continue
        dy, dx, cin = row // 6, (row % 6) // 2, row % 2
        assert a[j] == halo[0, y + dy, x + dx, cin], (w, lane, j)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_product_is_the_convolution(seed):
  """D = C + A B over the instruction's 64 k bytes (lane group, byte: the same pairing in A and B,
  whatever the instruction's k order), against the 3x3 convolution of the patch."""
  r = np.random.Generator(np.random.PCG64(14 + seed))
  halo = r.integers(0, 2, (HALO, HALO, 2))
  codes = r.integers(-7, 8, (18, 16))
  lds = r.integers(0, 128, HIMG2 + 64)
  for cp in range(2):
    for hy in range(HALO):
      for hx in range(HALO):
        at = cp * HCOPY2 + hy * HROW2 + 2 * hx + 2 * cp
        lds[at:at + 2] = 16 * halo[hy, hx]
  want = np.zeros((8, 8, 16), np.int64)
  for y in range(8):
    for x in range(8):
      want[y, x] = halo[y:y + 3, x:x + 3].reshape(18) @ codes
  for w in range(4):
    for lane in range(64):                                      # a lane of D: channel lane & 15, four pixels
      c = lane & 15
      for i in range(4):
        rrow = 4 * (lane >> 4) + i
        acc = 0
        for kb in range(4):
          off, y, x = a_offset(w, 16 * kb + rrow)
          a = np.concatenate([lds[off:off + 8], lds[off + HROW2:off + HROW2 + 8]])
          acc += int(a @ b_bytes(codes, c, kb))
        _, y, x = updates(w, lane, i)
        assert acc == 128 * want[y, x, c]                       # table rows of 128 bytes: 16 x input, 8 x code


# ---- the predicate ------------------------------------------------------------------------------

def _ask(L, what, cout=96, fire=80, in_type=None, T=20, state=0, pool=2, x_max=1, nrn=None):
  g = L.ConvGeomT(H=16, W=24, Cin=2, Cout=cout, KH=3, KW=3, stride_h=1, stride_w=1, pad_h_lo=1, pad_h_hi=1,
                  pad_w_lo=1, pad_w_hi=1, in_dil_h=1, in_dil_w=1, k_dil_h=1, k_dil_w=1, groups=1)
  w = L.WeightT(L.W_I8, 8, 7.0, 1.0, 40, 7)
  w.ch_stack_max, w.cout_fire = 47, fire
  n = L.NeuronT(*(nrn or (L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)))
  f = getattr(L.lib(), "snnqp_conv_event_" + what)
  return f(L.EV1 if in_type is None else in_type, T, ctypes.byref(g), ctypes.byref(w), ctypes.byref(n), state,
           pool, x_max)


@pytest.fixture
def switches():
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  yield L, lib
  lib.snnqp_set_event_quarter16(1)
  lib.snnqp_set_event_wave_spread(1)
  lib.snnqp_set_event_half_group(1)


TABLE = [
    ("96 / 80: the headline", dict(), 1),
    ("96 / 80 without pool", dict(pool=1), 1),
    ("64: spread, no quarter", dict(cout=64, fire=0), 0),
    ("64 / 48: the half group's own launch", dict(cout=64, fire=48), 0),
    ("96 / 96", dict(cout=96, fire=96), 0),
    ("128 / 112", dict(cout=128, fire=112), 0),
    ("state carried", dict(state=1), 0),
    ("T = 40: two staging chunks", dict(T=40), 0),
    ("byte frames", dict(in_type=1), 0),
    ("v_reset != 0", dict(nrn=(1, 2.0, 1.0, 0.5)), 0),
]


@pytest.mark.parametrize("what,kw,want", TABLE, ids=[t[0] for t in TABLE])
def test_predicate_truth_table(switches, what, kw, want):
  L, lib = switches
  if "nrn" in kw:
    kw = dict(kw, nrn=(L.NEURON_MULTI_STEP_LIF,) + kw["nrn"][1:])
  if "in_type" in kw:
    kw = dict(kw, in_type=L.U8)
  assert lib.snnqp_set_event_quarter16(-1) == 1
  assert _ask(L, "quarter16", **kw) == want, what
  # it is the spread launch with the half group, and nothing else
  assert want == (_ask(L, "wave_spread", **kw) and _ask(L, "half_group", **kw))
  # the switch off: never; and it returns what it replaced, and leaves the other two paths alone
  spread = _ask(L, "wave_spread", **kw)
  assert lib.snnqp_set_event_quarter16(0) == 1
  assert lib.snnqp_set_event_quarter16(-1) == 0
  assert _ask(L, "quarter16", **kw) == 0, what
  assert _ask(L, "wave_spread", **kw) == spread
  assert lib.snnqp_set_event_quarter16(1) == 0
  # either of the other switches off: no quarter to take
  for other in (lib.snnqp_set_event_wave_spread, lib.snnqp_set_event_half_group):
    other(0)
    assert _ask(L, "quarter16", **kw) == 0, what
    other(1)


def test_predicate_refuses_what_the_half_group_predicate_refuses(switches):
  L, lib = switches
  assert _ask(L, "quarter16", fire=24) == L.EINVAL and b"conv_event_quarter16" in lib.snnqp_last_error()
  assert _ask(L, "quarter16", pool=3) == L.EINVAL
  assert _ask(L, "quarter16", T=-1) == L.EINVAL
  assert lib.snnqp_conv_event_quarter16(L.EV1, 20, None, None, None, 0, 1, 1) == L.EINVAL
