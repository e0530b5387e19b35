"""CPU suite: the wave spread of the event layer (conv3x3_u8c2.hip, template parameter
SPREAD) -- a numpy model of which (channel, pixel) every (wave, register, lane) of the spread launches
updates, of the lanes that store the three words of a (pooled) pixel, and the truth table of the
predicate snnqp_conv_event_wave_spread."""
import ctypes
import itertools

import numpy as np
import pytest


# ---- the placement, as the kernel makes it ---------------------------------------------------
# Lane (n, h) of the MFMA's D: column n (the channel), register i = row d_row(i, h) of the product.

def d_row(i, h):
  return (i & 3) + 4 * h + 8 * (i >> 2)


def row_pixel(m):
  """(ty, tx) of the 4x8 tile that A row m reads (conv3x3_u8c2.hip: ty, tx of lane n = m)."""
  return ((m >> 2) & 1) | ((m >> 4) << 1), (m & 3) | (((m >> 3) & 1) << 2)


def own_unit(w, i, n, h):
  """(channel, image row, column) that register i of lane (n, h) of wave w updates in its own unit:
  tile w & 1 of channel group w >> 1."""
  ty, tx = row_pixel(d_row(i, h))
  return 32 * (w >> 1) + n, 4 * (w & 1) + ty, tx


def half_group_pixel(i, n, h, perm=0):
  """The half group's product (test_event_half_group_cpu.py): A row m reads the even image row 2 ty
  of the pixel of row m ^ perm; lanes n >= 16 hold the channel of lane n - 16 one image row lower."""
  ty, tx = row_pixel(d_row(i, h) ^ perm)
  return 2 * ty + (n >> 4), tx


def quarter(w, i, n, h):
  """(channel, image row, column) that register i < 4 of wave w updates in the shared unit: the wave
  permutes its A rows by 8 w."""
  y, x = half_group_pixel(i, n, h, perm=8 * w)
  return 64 + (n & 15), y, x


LANES = [(n, h) for h in range(2) for n in range(32)]


def _updates(half):
  out = []
  for w in range(4):
    for i in range(16):
      out += [own_unit(w, i, n, h) for n, h in LANES]
    if half:
      for i in range(4):
        out += [quarter(w, i, n, h) for n, h in LANES]
  return out


@pytest.mark.parametrize("channels,half", [(64, False), (80, True)])
def test_every_channel_and_pixel_has_exactly_one_updater(channels, half):
  got = _updates(half)
  want = set(itertools.product(range(channels), range(8), range(8)))
  assert len(got) == len(want) == channels * 64        # nothing twice ...
  assert set(got) == want                              # ... nothing missing, nothing else
  # and the same number of potentials in every wave: 16, or 16 + 4
  assert len(got) == 4 * 64 * (20 if half else 16)


def test_the_quarters_tile_the_sixteen_registers_of_the_half_group():
  seen = []
  for w in range(4):
    g, q = w >> 1, w & 1
    for i in range(4):
      full = 4 * w + i                                  # the register of the unpermuted product
      seen.append(full)
      for n, h in LANES:
        assert half_group_pixel(i, n, h, perm=8 * w) == half_group_pixel(full, n, h)
        _, y, x = quarter(w, i, n, h)
        assert x == 4 * q + i and 4 * g <= y < 4 * g + 4
      # (a register pair = two neighbouring columns, a lane half = two neighbouring rows: whole 2x2 windows)
  assert sorted(seen) == list(range(16))


# ---- who stores which word ---------------------------------------------------------------------

def out_pix(pool, tl, lane):
  if pool:
    return (tl * 2 + ((lane >> 2) & 1)) * 4 + (lane & 3)
  ty = ((lane >> 2) & 1) | (((lane >> 4) & 1) << 1)
  tx = (lane & 3) | (((lane >> 3) & 1) << 2)
  return (tl * 4 + ty) * 8 + tx


def store_plan(pool, half):
  """[(wave, lane, ring word index)] of the stores of one timestep (conv3x3_u8c2.hip: ob0 / store_lane,
  ob1 / quarter_lane)."""
  out = []
  for w in range(4):
    g, q = w >> 1, w & 1
    for lane in range(64):
      if lane < (8 if pool else 32):
        out.append((w, lane, out_pix(pool, q, lane) * 4 + g))
      if half and (lane < 8 and (lane & 2) == 0 if pool else lane < 16):
        pix = ((2 * g + ((lane >> 2) & 1)) * 4 + 2 * q + (lane & 1) if pool
               else (4 * g + ((lane >> 2) & 3)) * 8 + 4 * q + (lane & 3))
        out.append((w, lane, pix * 4 + 2))
  return out


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("half", [False, True])
def test_every_word_of_every_pixel_has_exactly_one_writer(pool, half):
  words = [o for _, _, o in store_plan(pool, half)]
  npix = 16 if pool else 64
  want = sorted(p * 4 + k for p in range(npix) for k in range(3 if half else 2))
  assert sorted(words) == want


def _mask(spikes, where):
  """64-bit compare mask of one register: bit 32 h + n = the spike of where(n, h) = (channel, y, x)."""
  v = 0
  for n, h in LANES:
    c, y, x = where(n, h)
    v |= int(spikes[y, x, c]) << (32 * h + n)
  return v


@pytest.mark.parametrize("pool", [False, True])
def test_stored_words_are_the_spikes_of_their_pixels(pool):
  """The words as place_words (conv_tile.h) drops them into lanes -- EP_TILE for the own unit, EP_QUARTER
  for the shared unit -- stored by the plan above, against the raster read directly."""
  r = np.random.Generator(np.random.PCG64(11))
  s = r.random((8, 8, 80)) < 0.3
  ring = {}
  for w in range(4):
    g, q = w >> 1, w & 1
    lanes_own, lanes_q = {}, {}
    m = [_mask(s, lambda n, h, i=i: own_unit(w, i, n, h)) for i in range(16)]
    mq = [_mask(s, lambda n, h, i=i: quarter(w, i, n, h)) for i in range(4)]
    if pool:
      for i in range(0, 16, 2):
        o = m[i] | m[i + 1]
        lanes_own[i >> 1] = (o | o >> 32) & 0xFFFFFFFF
      for j in range(2):
        o = mq[2 * j] | mq[2 * j + 1]
        lo, hi = o & 0xFFFFFFFF, o >> 32
        lanes_q[j] = (lo | lo >> 16) & 0xFFFF
        lanes_q[4 + j] = (hi | hi >> 16) & 0xFFFF
    else:
      for i in range(0, 16, 2):
        r0 = (i & 3) + 8 * (i >> 2)
        lanes_own[r0], lanes_own[r0 + 4] = m[i] & 0xFFFFFFFF, m[i] >> 32
        lanes_own[r0 + 1], lanes_own[r0 + 5] = m[i + 1] & 0xFFFFFFFF, m[i + 1] >> 32
      for i in range(4):
        for f in range(4):
          lanes_q[4 * f + i] = (mq[i] >> (16 * f)) & 0xFFFF
    for ww, lane, o in store_plan(pool, True):
      if ww != w:
        continue
      src = lanes_q if o & 3 == 2 else lanes_own
      assert o not in ring
      ring[o] = src[lane]                                 # (a lane the epilogue did not write: KeyError)
  word = lambda bits: sum(int(b) << c for c, b in enumerate(bits))
  for pix in range(16 if pool else 64):
    if pool:
      py, px = pix >> 2, pix & 3
      px_s = s[2 * py:2 * py + 2, 2 * px:2 * px + 2].reshape(4, 80).any(0)
    else:
      px_s = s[pix >> 3, pix & 7]
    assert ring[pix * 4] == word(px_s[:32])
    assert ring[pix * 4 + 1] == word(px_s[32:64])
    assert ring[pix * 4 + 2] == word(px_s[64:80])


# ---- the predicate ------------------------------------------------------------------------------

def _lib():
  from snnquantprune_amd import _lib as L
  return L


def _ask(L, what, cout=96, fire=80, in_type=None, T=20, state=0, pool=2, x_max=1, nrn=None, code_max=7,
         stack=47, abs_sum=40):
  g = L.ConvGeomT(H=16, W=24, Cin=2, Cout=cout, KH=3, KW=3, stride_h=1, stride_w=1, pad_h_lo=1, pad_h_hi=1,
                  pad_w_lo=1, pad_w_hi=1, in_dil_h=1, in_dil_w=1, k_dil_h=1, k_dil_w=1, groups=1)
  w = L.WeightT(L.W_I8, 8, 7.0, 1.0, abs_sum, code_max)
  w.ch_stack_max, w.cout_fire = stack, fire
  n = L.NeuronT(*(nrn or (L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)))
  f = getattr(L.lib(), "snnqp_conv_event_" + what)
  return f(L.EV1 if in_type is None else in_type, T, ctypes.byref(g), ctypes.byref(w), ctypes.byref(n), state,
           pool, x_max)


@pytest.fixture
def switches():
  L = _lib()
  lib = L.lib()
  yield lib
  lib.snnqp_set_event_wave_spread(1)
  lib.snnqp_set_event_half_group(1)


# (what, keyword changes, spread with both switches on)
TABLE = [
    ("96 / 80: the headline", dict(), 1),
    ("96 / 80 without pool", dict(pool=1), 1),
    ("64, every channel may fire", dict(cout=64, fire=0), 1),
    ("64 / 64", dict(cout=64, fire=64), 1),
    ("64 / 48: the half group's own launch", dict(cout=64, fire=48), 0),
    ("32", dict(cout=32, fire=0), 0),
    ("32 / 16", dict(cout=32, fire=16), 0),
    ("48", dict(cout=48, fire=0), 0),
    ("96 / 96", dict(cout=96, fire=96), 0),
    ("96, nothing known", dict(cout=96, fire=0), 0),
    ("128", dict(cout=128, fire=0), 0),
    ("128 / 112", dict(cout=128, fire=112), 0),
    ("state carried", dict(state=1), 0),
    ("T = 40: two staging chunks", dict(T=40), 0),
    ("T = 0", dict(T=0), 0),
    ("byte frames", dict(in_type=1, x_max=1), 0),
    ("v_reset != 0", dict(nrn=(1, 2.0, 1.0, 0.5)), 0),
    ("tau = 3: divided", dict(nrn=(1, 3.0, 1.0, 0.0)), 0),
    ("8-bit codes: the shared table", dict(code_max=127, abs_sum=900, stack=0), 0),
]


@pytest.mark.parametrize("what,kw,want", TABLE, ids=[t[0] for t in TABLE])
def test_predicate_truth_table(switches, what, kw, want):
  L = _lib()
  if "nrn" in kw:
    kw = dict(kw, nrn=(L.NEURON_MULTI_STEP_LIF,) + kw["nrn"][1:])
  if "in_type" in kw:
    kw = dict(kw, in_type=L.U8)
  lib = switches
  assert lib.snnqp_set_event_wave_spread(-1) == 1 and lib.snnqp_set_event_half_group(-1) == 1
  assert _ask(L, "wave_spread", **kw) == want, what
  # the switch off: never; and it returns what it replaced
  assert lib.snnqp_set_event_wave_spread(0) == 1
  assert lib.snnqp_set_event_wave_spread(-1) == 0
  assert _ask(L, "wave_spread", **kw) == 0, what
  assert lib.snnqp_set_event_wave_spread(1) == 0
  # the half-group switch off: 96 / 80 is then a whole 96-channel launch (old path), 64 / 48 a
  # 64-channel launch off the half path (spread), everything else as before
  lib.snnqp_set_event_half_group(0)
  cout = kw.get("cout", 96)
  plain = {k: v for k, v in kw.items() if k not in ("cout", "fire")}
  family = _ask(L, "wave_spread", cout=64, fire=0, **plain)     # is it the family at all?
  assert _ask(L, "half_group", **kw) == 0
  assert _ask(L, "wave_spread", **kw) == (1 if cout == 64 and family else 0), what


def test_predicate_refuses_what_the_half_group_predicate_refuses(switches):
  L = _lib()
  assert _ask(L, "wave_spread", fire=24) == L.EINVAL and b"conv_event_wave_spread" in L.lib().snnqp_last_error()
  assert _ask(L, "wave_spread", pool=3) == L.EINVAL
  assert _ask(L, "wave_spread", T=-1) == L.EINVAL
  assert L.lib().snnqp_conv_event_wave_spread(L.EV1, 20, None, None, None, 0, 1, 1) == L.EINVAL
