"""CPU checks of the K packing of the bit-input 3x3 conv kernels (bits_tile.h):
the Cin padding rule of the packed codes, and -- on a model of the kernel's LDS halo image and
lane addressing -- that the k-steps it walks pair every A fragment with the int8 tile of the same
(tap, 32-channel group), each exactly once."""
import pytest

from snnquantprune_amd import packing

# bits_tile.h (BitsTile: the layout conv3x3_bits.hip and conv3x3_currents.hip share); HALO: conv_tile.h
F6_PITCH, F6_ROWS, HALO = 12, 6, 10
F6_PLANE = F6_ROWS * F6_PITCH * 32


def pair_tap(p, h):
  return p + 3 * h if p < 3 else 2 * p + h


def test_cin_pad_rule():
  for cin in range(1, 129):
    assert packing.conv_cin_pad(cin) == 32 * ((cin + 31) // 32)
    assert packing.conv_cin_pad(cin, False) == (64 if cin <= 64 else 128)
  for bad in (0, 129):
    with pytest.raises(ValueError):
      packing.conv_cin_pad(bad)


def _staged(G, i8):
  """LDS byte address -> (halo row, halo column, spike word) of the halo image as staged."""
  img = {}
  for hy in range(F6_ROWS):
    for hx in range(HALO):
      for wi in range(G):
        plane = wi if i8 else wi >> 1
        base = plane * F6_PLANE + (hy * F6_PITCH + hx) * 32
        if i8:                                   # both 16-byte halves of the word's plane
          for half in range(2):
            img[base + ((half ^ (hy & 1)) * 16)] = (hy, hx, wi, half)
        else:
          img[base + (((wi & 1) ^ (hy & 1)) * 16)] = (hy, hx, wi, 0)
  return img


def _walk(G, i8):
  """The kernel's k-steps: per (k-step, lane half) the B tile index (None: zero codes) and,
  per lane n, the LDS byte address of its A fragment."""
  NP = G if i8 else (G + 1) // 2
  NPL = G if i8 else G // 2
  PAIRS = 0 if i8 or G % 2 == 0 else 5
  KS = 9 * NPL + PAIRS
  steps = []
  for ks in range(KS):
    for h in range(2):
      addrs = []
      for n in range(32):
        ty = ((n >> 2) & 1) | ((n >> 4) << 1)
        tx = (n & 3) | (((n >> 3) & 1) << 2)
        pixb = (ty * F6_PITCH + tx) * 32
        if ks < 9 * NPL:
          tap = ks // NPL
          base = pixb + ((h ^ (ty & 1) ^ ((tap // 3) & 1)) * 16)
          off = (ks % NPL) * F6_PLANE + ((tap // 3) * F6_PITCH + tap % 3) * 32
        else:
          p = ks - 9 * NPL
          if p < 3:
            base = pixb + h * F6_PITCH * 32 + ((ty ^ h) & 1) * 16
          else:
            base = pixb + h * 32 + (ty & 1) * 16
          off = NPL * F6_PLANE + (p if p < 3 else 2 * F6_PITCH + 2 * (p - 3)) * 32
        addrs.append((ty, tx, base + off))
      if i8:
        tile = ks
      elif ks < 9 * NPL:
        tile = (ks // NPL) * G + (ks % NPL) * 2 + h
      else:
        t = pair_tap(ks - 9 * NPL, h)
        tile = t * G + G - 1 if t < 9 else None
      steps.append((ks, h, tile, addrs))
  return KS, NP, steps


@pytest.mark.parametrize("i8", [False, True], ids=["fp6", "int8"])
@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_k_walk_pairs_fragments_with_their_tiles(G, i8):
  KS, NP, steps = _walk(G, i8)
  assert KS == (9 * G if i8 else (9 * G + 1) // 2)
  img = _staged(G, i8)
  seen = []
  for ks, h, tile, addrs in steps:
    for ty, tx, addr in addrs:
      assert 0 <= addr and addr + 16 <= NP * F6_PLANE, (ks, h)   # every read inside the image
      if tile is None:
        continue                                  # zero codes: any spikes will do
      # packed codes: row tap * Cpad + cin, tile f = rows 32 f .. 32 f + 31 = (tap, group)
      tap, group = divmod(tile, G)
      assert img.get(addr) is not None, (ks, h, ty, tx)
      hy, hx, wi, half = img[addr]
      assert (hy - ty, hx - tx) == divmod(tap, 3) and wi == group, (ks, h, ty, tx)
      if i8:
        assert half == h                          # int8: lane half h holds channels 16 h + j
    if tile is not None:
      seen.append(tile)
  per_tile = 2 if i8 else 1                       # (int8: both lane halves of a k-step)
  assert sorted(seen) == sorted(list(range(9 * G)) * per_tile)
