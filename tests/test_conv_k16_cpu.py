"""CPU checks of the 16-channel K walk of the bit-input 3x3 conv kernel (conv3x3_bits.hip on the
layout of bits_tile.h): the address model of test_conv_kpack_cpu.py extended to a last channel group of
which only the lower 16 channels are walked (CIN = 16, 48, 80, 112).  On a model of the LDS halo
image as the kernel stages it and of its lane addressing: every A piece meets the code rows of its
own (tap, 16-channel) unit, every (tap, channel) is covered exactly once, empty units meet zero
codes, the k-step counts are the ones DESIGN.md lists, the A ring never overwrites a fragment that
is still waiting for its MFMA, and the lanes of one LDS read group hit distinct banks."""
import pytest

# bits_tile.h (BitsTile: the layout conv3x3_bits.hip and conv3x3_currents.hip share); HALO: conv_tile.h
F6_PITCH, F6_ROWS, HALO = 12, 6, 10
F6_PLANE = F6_ROWS * F6_PITCH * 32
KS_TABLE = {("fp6", 16): 3, ("fp6", 48): 8, ("fp6", 80): 12, ("fp6", 112): 17,
            ("int8", 16): 5, ("int8", 48): 14, ("int8", 80): 23, ("int8", 112): 32}


def pair_tap(p, h):
  return p + 3 * h if p < 3 else 2 * p + h


def k16_tap(q, h, i):
  return q + 3 * h if i == 0 else (6 + q if h == 0 else 9)


def _shape(cin, i8):
  WPP, GW = (cin + 31) // 32, cin // 32
  NP = WPP if i8 else (WPP + 1) // 2
  NPL = GW if i8 else GW // 2
  PAIRS = 5 if (cin % 32 if i8 else GW % 2 == 1) else 0
  K16 = 3 if not i8 and cin % 32 else 0
  return WPP, GW, NP, NPL, PAIRS, K16


def _staged(cin, i8):
  """LDS byte address -> (halo row, halo column, first channel) for every 8-byte piece (fp4: 16
  channels) or 16-byte piece (bytes: 16 channels) of the halo image as the kernel stages it."""
  WPP, GW, NP, NPL, PAIRS, K16 = _shape(cin, i8)
  img = {}
  for hy in range(F6_ROWS):
    for hx in range(HALO):
      for wi in range(WPP):
        plane = wi if i8 else wi >> 1
        base = plane * F6_PLANE + (hy * F6_PITCH + hx) * 32
        if i8:                                   # channels 0..15 and 16..31 of the word
          for half in range(2):
            img[base + ((half ^ (hy & 1)) * 16)] = (hy, hx, 32 * wi + 16 * half)
        else:
          slot = base + (((wi & 1) ^ (hy & 1)) * 16)
          img[slot] = (hy, hx, 32 * wi)
          # the 16-channel last group: its lower 16 channels again in place of the upper 16
          img[slot + 8] = (hy, hx, 32 * wi + (0 if K16 and wi == GW else 16))
  return img


def _lane(n):
  return ((n >> 2) & 1) | ((n >> 4) << 1), (n & 3) | (((n >> 3) & 1) << 2)


def _walk(cin, i8):
  """Per k-step a list of reads; a read is (bytes per lane, [per lane half h: per lane n the LDS
  byte address], [per lane half: the units (tap, first channel) its pieces of 16 channels carry,
  None for zero codes])."""
  WPP, GW, NP, NPL, PAIRS, K16 = _shape(cin, i8)
  steps = []
  for ks in range(9 * NPL + PAIRS + K16):
    reads = []
    if ks < 9 * NPL:                              # a whole plane at one tap
      tap, kk = divmod(ks, NPL)
      addrs, units = [], []
      for h in range(2):
        a = []
        for n in range(32):
          ty, tx = _lane(n)
          base = (ty * F6_PITCH + tx) * 32 + ((h ^ (ty & 1) ^ ((tap // 3) & 1)) * 16)
          a.append(base + kk * F6_PLANE + ((tap // 3) * F6_PITCH + tap % 3) * 32)
        addrs.append(a)
        grp = kk if i8 else 2 * kk + h
        units.append([(tap, 32 * grp + 16 * h)] if i8 else [(tap, 32 * grp), (tap, 32 * grp + 16)])
      reads.append((16, addrs, units))
    elif ks < 9 * NPL + PAIRS:                    # pair walk: first half of plane NPL
      p = ks - 9 * NPL
      grp = GW if i8 else GW - 1
      addrs, units = [], []
      for h in range(2):
        a = []
        for n in range(32):
          ty, tx = _lane(n)
          pixb = (ty * F6_PITCH + tx) * 32
          if p < 3:
            base = pixb + h * F6_PITCH * 32 + ((ty ^ h) & 1) * 16
          else:
            base = pixb + h * 32 + (ty & 1) * 16
          a.append(base + NPL * F6_PLANE + (p if p < 3 else 2 * F6_PITCH + 2 * (p - 3)) * 32)
        addrs.append(a)
        t = pair_tap(p, h)
        if t >= 9:
          units.append([None] if i8 else [None, None])
        else:
          units.append([(t, 32 * grp)] if i8 else [(t, 32 * grp), (t, 32 * grp + 16)])
      reads.append((16, addrs, units))
    else:                                         # k16: two 8-byte pieces per lane
      q = ks - 9 * NPL - PAIRS
      off = (GW >> 1) * F6_PLANE + q * 32
      for i in range(2):
        addrs, units = [], []
        for h in range(2):
          a = []
          for n in range(32):
            ty, tx = _lane(n)
            pixb = (ty * F6_PITCH + tx) * 32
            if i == 0:
              base = pixb + h * F6_PITCH * 32 + ((GW ^ ty ^ h) & 1) * 16 + (((ty + h) >> 1) & 1) * 8
              a.append(base + off)
            else:
              base = pixb + ((GW ^ ty) & 1) * 16 + (((ty >> 1) & 1) ^ 1) * 8
              a.append(base + off + 2 * F6_PITCH * 32)
          addrs.append(a)
          t = k16_tap(q, h, i)
          units.append([(t, 32 * GW) if t < 9 else None])
        reads.append((8, addrs, units))
    steps.append(reads)
  return steps


CASES = [(cin, i8) for i8 in (False, True) for cin in (16, 48, 80, 112)]
IDS = ["%s-%d" % ("int8" if i8 else "fp6", cin) for cin, i8 in CASES]


@pytest.mark.parametrize("cin,i8", CASES, ids=IDS)
def test_k16_walk_pairs_pieces_with_their_code_rows(cin, i8):
  WPP, GW, NP, NPL, PAIRS, K16 = _shape(cin, i8)
  steps = _walk(cin, i8)
  assert len(steps) == KS_TABLE["int8" if i8 else "fp6", cin]
  img = _staged(cin, i8)
  piece = 16 if i8 else 8                         # bytes of 16 channels
  seen = []
  for ks, reads in enumerate(steps):
    kbytes = 0
    for nbytes, addrs, units in reads:
      kbytes += nbytes
      for h in range(2):
        for n, addr in enumerate(addrs[h]):
          ty, tx = _lane(n)
          assert 0 <= addr and addr + nbytes <= NP * F6_PLANE, (ks, h)   # inside the image
          for j, unit in enumerate(units[h]):
            if unit is None:
              continue                            # zero codes: any spikes will do
            tap, ch = unit
            got = img.get(addr + j * piece)
            assert got is not None, (ks, h, n)    # a staged piece, not a gap of the image
            hy, hx, c0 = got
            assert (hy - ty, hx - tx) == divmod(tap, 3) and c0 == ch, (ks, h, n, unit, got)
        seen += [u for u in units[h] if u is not None]
    assert kbytes == 16                           # one A fragment: K = 64 fp4 / 32 bytes per lane pair
  # every (tap, 16-channel unit) below CIN exactly once; the upper half of the last group never
  want = [(tap, c) for tap in range(9) for c in range(0, cin, 16)]
  assert sorted(seen) == sorted(want)


@pytest.mark.parametrize("cin,i8", CASES, ids=IDS)
def test_k16_reads_are_bank_conflict_free(cin, i8):
  """ds_read_b64: the two 32-lane halves are the groups, bank (a / 4) % 64; ds_read_b128: four
  16-lane groups, the same banks.  Every lane of a group on banks of its own: 0 conflicts."""
  b128_groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
                 [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
  for reads in _walk(cin, i8):
    for nbytes, addrs, _ in reads:
      for h in range(2):
        groups = [list(range(32))] if nbytes == 8 else b128_groups
        for grp in groups:
          banks = [(addrs[h][n] // 4 + d) % 64 for n in grp for d in range(nbytes // 4)]
          assert len(set(banks)) == len(banks)
          assert all(addrs[h][n] % nbytes == 0 for n in grp)   # aligned: no replay


def _ring(ks, table, i8):
  """RING, PF of conv3x3_bits_kernel."""
  def ok(ring, pf):
    if pf >= ring or pf >= ks:
      return False
    return all((k + pf) % ks % ring != (k + j) % ks % ring for k in range(ks) for j in range(1, pf))
  div = 6 if ks % 6 == 0 and not table else 3 if ks % 3 == 0 else 7 if ks % 7 == 0 else ks
  ring = div if div < ks or ks <= 5 else 3 if table else 6 if ok(6, 4) else 8
  pf = 1 if ks == 3 else 4 if ring in (6, 8) or (ring == 7 and not table) else 2
  return ring, pf, ok(ring, pf)


@pytest.mark.parametrize("cin,i8", CASES, ids=IDS)
def test_k16_fragment_ring_and_halo_slots(cin, i8):
  ks = KS_TABLE["int8" if i8 else "fp6", cin]
  for table in ([False] if i8 else [False, True]):
    ring, pf, ok = _ring(ks, table, i8)
    assert ok and ring <= 8
    # simulate three timesteps: entry k % ring holds the fragment of k-step k when its MFMA runs
    held = {k % ring: (0, k) for k in range(pf)}
    for t in range(3):
      for k in range(ks):
        assert held[k % ring] == (t, k)
        nt, nk = (t, k + pf) if k + pf < ks else (t + 1, k + pf - ks)
        held[nk % ring] = (nt, nk)
    # the halo of timestep t + 2 is written before the barrier, the next fragments read after it
    late = table or i8
    bar_late = ks * 5 // 6 if ks * 5 // 6 < ks - pf else ks - pf - 1
    wr_late = ks * 5 // 9 if ks * 5 // 9 < bar_late else bar_late - 1
    wr = wr_late if late else 2 if 2 < ks - pf - 2 else 1 if ks - pf > 2 else 0
    bar = bar_late if late else 4 if 4 < ks - pf else wr + 1
    assert 0 <= wr < bar < ks - pf
