"""The gated ('gint') connections one launch at a time: csrc/conv_gated.hip and dense_gated.hip in
every launch form and on every code value.  The case tables, their data and the references; no GPU
here -- tests/test_gated_forms_cpu.py and test_gated_forms_gpu.py use it.

The contract (include/snnqp.h):
    I[c][o] = sum over the taps / positions of channel c of code * spike      (exact integer)
    acc[o]  = fmaf(gate[c], I[c][o], acc[o])   for c = 0 .. C - 1, from +0
    y[o]    = fl(fl(acc / L) * m)
The reference is oracle.gated_conv / oracle.gated_dense on a stand-in weight made from RAW codes
(they read only q, L, m and quantised): I as an exact integer, the chain with the C library's
fmaf.  The chain is not emulated in float64: g x I has up to 35 significant bits, so a float64
product rounded to float32 may round twice.

Forms.  conv: snnqp_conv_gated_plan -> (full_groups, rest_tiles, wide): a launch of
conv_gated_kernel<4, wide> on full_groups workgroup rows, then conv_gated_kernel<rest_tiles, wide>
on the last tiles.  dense: snnqp_dense_gated_plan -> (grid_y, wide); inside the launch wave w of
workgroup row y holds live = clamp(OT - 4 (4 y + w), 0, 4) output tiles (none: it leaves after the
barrier)."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import snn_oracle as oracle
from tests.train_helpers import mixed

F32 = np.float32
F64 = np.float64


class RawWeight:
  """What oracle.gated_conv / gated_dense read of a QWeight, made from raw integer codes."""
  quantised = True

  def __init__(self, codes, L, m):
    self.q = np.asarray(codes, F32)
    self.L, self.m = F32(L), F32(m)


# kind "conv": NB images of H x W x C, 3x3 to N outputs; kind "dense": NB images of HW positions
# (H = HW, W = 1) x C channels to N outputs.  code_max: what the weight declares (it picks the
# layout); code_lim: the largest |code| the data holds.  codes: "rand" / "plus" / "minus" / "alt";
# raster: "rand" / "ones"; gates: "sigmoid" / "edges" / "inf" / "nan"; form: what the row claims --
# conv (full_groups, rest_tiles, wide), dense (grid_y, wide).
Case = namedtuple("Case", "name kind C N code_max H W NB form code_lim codes raster gates")


def _case(name, kind, C, N, code_max, H, W, NB, form, code_lim=None, codes="rand", raster="rand", gates="sigmoid"):
  return Case(name, kind, C, N, code_max, H, W, NB, tuple(form), code_max if code_lim is None else code_lim,
              codes, raster, gates)


def _cv(name, C, N, code_max, H, W, NB, form, **kw):
  return _case(name, "conv", C, N, code_max, H, W, NB, form, **kw)


def _dn(name, C, N, code_max, HW, NB, form, **kw):
  return _case(name, "dense", C, N, code_max, HW, 1, NB, form, **kw)


# ---- conv: every launch form, narrow and wide ------------------------------------------------------
# Patches of 4 x 8 pixels, four per workgroup: 1x1 (one pixel of a patch), 4x8 (one full patch),
# 3x9 and 5x11 (clipped patches, two and four per image).  npatch = NB tiles: 3, 1, 6, 4, 4, 5, 2,
# 2, 4 / 1, 6, 4, 3, 4, 2, 2, 2, 6.  Cin 32 and 96: lane half 1 has a word group beyond the raster
# in the transpose.  Cout 1 and 33: one output in the last tile.
CONV_FORMS = [
    _cv("n_nt1_cout1", 32, 1, 7, 1, 1, 3, (0, 1, False)),
    _cv("n_nt2_cout33", 64, 33, 7, 4, 8, 1, (0, 2, False)),
    _cv("n_nt3_cout96", 96, 96, 7, 3, 9, 3, (0, 3, False)),
    _cv("n_nt4_cout128", 128, 128, 7, 5, 11, 1, (1, 0, False)),
    _cv("n_nt4_1_cout129", 32, 129, 7, 3, 9, 2, (1, 1, False)),
    _cv("n_nt4_2_cout161", 64, 161, 7, 1, 1, 5, (1, 2, False)),
    _cv("n_nt4_3_cout224", 96, 224, 7, 4, 8, 2, (1, 3, False)),
    _cv("n_two_groups_cout256", 128, 256, 7, 3, 9, 1, (2, 0, False)),
    _cv("n_two_groups_2_cout300", 64, 300, 7, 5, 11, 1, (2, 2, False)),
    _cv("w_nt1_cout1", 96, 1, 127, 4, 8, 1, (0, 1, True)),
    _cv("w_nt2_cout33", 128, 33, 15, 3, 9, 3, (0, 2, True)),
    _cv("w_nt3_cout70", 32, 70, 31, 5, 11, 1, (0, 3, True)),
    _cv("w_nt4_cout128", 64, 128, 127, 1, 1, 3, (1, 0, True)),
    _cv("w_nt4_1_cout129_codes_to_7", 32, 129, 8, 3, 9, 2, (1, 1, True), code_lim=7),
    _cv("w_nt4_2_cout192", 128, 192, 127, 4, 8, 2, (1, 2, True)),
    _cv("w_nt4_3_cout200", 32, 200, 15, 3, 9, 1, (1, 3, True)),
    _cv("w_two_groups_cout256", 64, 256, 31, 1, 1, 2, (2, 0, True)),
    _cv("w_two_groups_2_cout300", 96, 300, 127, 3, 9, 3, (2, 2, True)),
]
ALL_CONV_FORMS = {(f, r, w) for w in (False, True)
                  for f, r in ((0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 2))}

# ---- dense: grid_y 1, 2, 3; every live tile count of a wave; narrow and wide ------------------------
# HW 6 and 11: the last position is one whose six bits straddle two dwords (positions 5 and 10).
DENSE_FORMS = [
    _dn("n_n1", 32, 1, 7, 1, 1, (1, False)),
    _dn("n_n32", 64, 32, 7, 5, 31, (1, False)),
    _dn("n_n33", 96, 33, 7, 6, 32, (1, False)),
    _dn("n_n70", 128, 70, 7, 10, 33, (1, False)),
    _dn("n_n128", 32, 128, 7, 11, 65, (1, False)),
    _dn("n_n160", 64, 160, 7, 15, 1, (1, False)),
    _dn("n_n512", 96, 512, 7, 16, 31, (1, False)),
    _dn("n_n513", 128, 513, 7, 6, 32, (2, False)),
    _dn("n_n600", 32, 600, 7, 11, 33, (2, False)),
    _dn("n_n1100", 64, 1100, 7, 16, 65, (3, False)),
    _dn("w_n1", 128, 1, 127, 16, 33, (1, True)),
    _dn("w_n32", 96, 32, 15, 15, 65, (1, True)),
    _dn("w_n33", 64, 33, 31, 11, 1, (1, True)),
    _dn("w_n70_codes_to_7", 128, 70, 8, 10, 33, (1, True), code_lim=7),
    _dn("w_n128", 128, 128, 127, 6, 32, (1, True)),
    _dn("w_n160", 96, 160, 15, 5, 33, (1, True)),
    _dn("w_n512", 64, 512, 31, 1, 65, (1, True)),
    _dn("w_n513", 32, 513, 127, 11, 1, (2, True)),
    _dn("w_n600", 128, 600, 127, 6, 31, (2, True)),
    _dn("w_n1100", 96, 1100, 127, 16, 32, (3, True)),
]
# (narrow row, the wide row on the same data): codes up to 7 packed as two digits give the same bits
SAME_DATA = [("n_nt4_1_cout129", "w_nt4_1_cout129_codes_to_7"), ("n_n70", "w_n70_codes_to_7")]

# ---- saturation: all-ones rasters, |I| = 9 code_max (interior pixels) and 16 code_max ---------------
SATURATION = [
    _cv("conv_sat_%s_%d" % (codes, cm), 128, 32, cm, 4, 8, 2, (0, 1, cm > 7), codes=codes, raster="ones")
    for cm in (7, 127) for codes in ("plus", "minus", "alt")
] + [
    _dn("dense_sat_%s_%d" % (codes, cm), 128, 32, cm, 16, 3, (1, cm > 7), codes=codes, raster="ones")
    for cm in (7, 127) for codes in ("plus", "minus", "alt")
]

# ---- gates: zero, -0.0, negative, subnormal, huge, mixed; one +inf, one NaN -------------------------
# (subnormal gates, products and currents are kept, not flushed: the kernels' fmaf, division and
# product run with float32 denormals on, as the C library's do -- the rows hold bit for bit)
GATE_EDGES = [
    _cv("conv_gates_edges_narrow", 64, 70, 7, 5, 11, 8, (0, 3, False), gates="edges"),
    _cv("conv_gates_edges_wide", 96, 129, 127, 3, 9, 8, (1, 1, True), gates="edges"),
    _dn("dense_gates_edges_narrow", 96, 70, 7, 11, 40, (1, False), gates="edges"),
    _dn("dense_gates_edges_wide", 64, 513, 127, 6, 40, (2, True), gates="edges"),
    _cv("conv_gate_inf", 64, 70, 127, 3, 9, 3, (0, 3, True), gates="inf"),
    _cv("conv_gate_nan", 64, 70, 7, 3, 9, 3, (0, 3, False), gates="nan"),
    _dn("dense_gate_inf", 64, 70, 7, 6, 35, (1, False), gates="inf"),
    _dn("dense_gate_nan", 64, 70, 127, 6, 35, (1, True), gates="nan"),
]
NONFINITE_AT = (1, 5)                 # (image, channel) of the one +inf / NaN gate

CASES = CONV_FORMS + DENSE_FORMS + SATURATION + GATE_EDGES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# rows that also run as a whole SpikingBlock (BatchNorm, scan, pool 1 and 2 / dense: the scan): even
# H and W, Cout > 128 narrow and wide; N > 512
BLOCK_ROWS = ["n_nt4_3_cout224", "w_nt4_2_cout192", "w_n1100"]


def hw(c):
  return c.H * c.W


def dequant(c):
  """(L, m) of a row: L as DuQ has it (the largest code), m no power of two."""
  return float(c.code_lim), 0.37


def live_tiles(c):
  """dense: the live output tiles of every wave of a workgroup column, [grid_y][4]."""
  OT = -(-c.N // 32)
  return [[min(4, max(0, OT - 4 * (4 * y + w))) for w in range(4)] for y in range(c.form[0])]


def _seed(c):
  # (rows that differ only in name and declared code_max share their data)
  key = "%s %d %d %d %d %d %d %s %s %s" % (c.kind, c.C, c.N, c.code_lim, c.H, c.W, c.NB, c.codes, c.raster, c.gates)
  return zlib.crc32(key.encode())


def _edge_gates(rng, NB, C):
  """Per image one of four profiles, so that no profile drowns another: 0 tiny (zero, -0.0,
  +-2^-130 and mixed x 2^-128: subnormal products and sums), 1 plain (zero, -0.0, negative
  sigmoids, mixed), 2 huge (+-2^100, mixed x 2^90), 3 everything."""
  g = np.empty((NB, C), F32)
  sig = (1.0 / (1.0 + np.exp(-rng.standard_normal((NB, C)) * 1.5))).astype(F32)
  mix = mixed(rng, (NB, C))
  pick = rng.integers(0, 4, (NB, C))
  tiny = np.choose(pick, [np.zeros((NB, C), F32), np.full((NB, C), -0.0, F32),
                          np.where(mix < 0, F32(-2.0 ** -130), F32(2.0 ** -130)), mix * F32(2.0 ** -128)])
  plain = np.choose(pick, [np.zeros((NB, C), F32), np.full((NB, C), -0.0, F32), -sig, mix])
  huge = np.choose(pick, [np.full((NB, C), 2.0 ** 100, F32), np.full((NB, C), -2.0 ** 100, F32),
                          mix * F32(2.0 ** 90), mix * F32(2.0 ** 90)])
  every = np.choose(rng.integers(0, 3, (NB, C)), [tiny, plain, huge])
  for i in range(NB):
    g[i] = (tiny, plain, huge, every)[i % 4][i]
  return g.astype(F32)


@lru_cache(maxsize=None)
def data(name):
  """(spikes uint8 [NB, H, W, C], gate float32 [NB, C], codes int8 -- conv HWIO [3, 3, C, N], dense
  [C HW, N] rows channel-major).  Read-only, made once per process."""
  c = BY_NAME[name]
  rng = np.random.Generator(np.random.PCG64(_seed(c)))
  wshape = (3, 3, c.C, c.N) if c.kind == "conv" else (c.C * hw(c), c.N)
  if c.codes == "rand":
    codes = rng.integers(-c.code_lim, c.code_lim + 1, wshape)
    codes[rng.random(wshape) < 0.3] = 0                       # pruned weights
    flat = codes.reshape(-1, c.N)
    flat[0, 0], flat[-1, -1] = c.code_lim, -c.code_lim        # the extremes occur
  else:
    sign = {"plus": 1, "minus": -1}.get(c.codes)
    if sign is None:
      idx = np.indices(wshape).sum(0)
      sign = 1 - 2 * (idx & 1)
    codes = np.broadcast_to(np.asarray(sign * c.code_lim), wshape)
  codes = np.ascontiguousarray(codes, np.int8)
  shape = (c.NB, c.H, c.W, c.C)
  s = np.ones(shape, np.uint8) if c.raster == "ones" else (rng.random(shape) < 0.3).astype(np.uint8)
  if c.raster == "rand":
    s.reshape(-1, c.C)[-1, -1] = 1                            # the last channel of the last word fires
  gate = (1.0 / (1.0 + np.exp(-rng.standard_normal((c.NB, c.C)) * 1.5))).astype(F32)
  if c.gates == "edges":
    gate = _edge_gates(rng, c.NB, c.C)
  elif c.gates in ("inf", "nan"):
    gate[NONFINITE_AT] = np.inf if c.gates == "inf" else np.nan
  for a in (s, gate, codes):
    a.setflags(write=False)
  return s, gate, codes


def weight(c, codes):
  L, m = dequant(c)
  return RawWeight(codes, L, m)


@lru_cache(maxsize=None)
def reference(name):
  """float32 currents, conv [NB, H, W, N] / dense [NB, N]: the oracle on the raw codes.  Computed
  once per process, read-only."""
  c = BY_NAME[name]
  s, gate, codes = data(name)
  qw = weight(c, codes)
  y = oracle.gated_conv(s, gate, qw) if c.kind == "conv" else oracle.gated_dense(s, gate, qw)
  y.setflags(write=False)
  return y


def channel_sums(c, s, codes):
  """The exact integers I, float64: conv [NB, H, W, C, N] / dense [NB, C, N], gathered with explicit
  index ranges (no padded copy: nothing shared with oracle.im2col)."""
  if c.kind == "dense":
    sp = s.reshape(c.NB, hw(c), c.C).astype(F64)
    return np.einsum("bpc,cpn->bcn", sp, codes.reshape(c.C, hw(c), c.N).astype(F64))
  I = np.zeros((c.NB, c.H, c.W, c.C, c.N), F64)
  sf, cf = s.astype(F64), codes.astype(F64)
  for kh in range(3):
    oy0, oy1 = max(0, 1 - kh), min(c.H, c.H + 1 - kh)
    for kw in range(3):
      ox0, ox1 = max(0, 1 - kw), min(c.W, c.W + 1 - kw)
      if oy0 < oy1 and ox0 < ox1:
        I[:, oy0:oy1, ox0:ox1] += (sf[:, oy0 + kh - 1:oy1 + kh - 1, ox0 + kw - 1:ox1 + kw - 1, :, None]
                                   * cf[kh, kw][None, None, None])
  return I


# ---- decoder cases: every code value at every tap / position of every channel, alone ----------------
# L = m = 1 and gate = 1, so the current IS the code the one spike meets.
# Wide layout: code = 16 hi + lo with lo = ((code + 8) & 15) - 8 in [-8, 7] and hi in [-8, 8]; the
# e3m2 entry for 8 serves lo = -8 (every code = 8 mod 16) as well as hi = +-8 (|code| >= 120).
DEC_C, DEC_N, DEC_HW = 128, 256, 16
DECODERS = [("conv_wide", "conv", 127), ("conv_narrow", "conv", 7), ("dense_wide", "dense", 127),
            ("dense_narrow", "dense", 7)]


def decoder_code(o, c, p, code_max):
  """The code of output o, channel c, tap / position p: ((o + 7 c + 29 p) mod (2 code_max + 1)) - code_max."""
  return (o + 7 * c + 29 * p) % (2 * code_max + 1) - code_max


@lru_cache(maxsize=None)
def decoder(name):
  """(spikes uint8, codes int8, expected float32) of a decoder case.
  conv: image c is 3 x 3 with one spike, at the centre in channel c: output pixel (oy, ox) sees it
  through tap (2 - oy, 2 - ox) alone, expected[c, oy, ox, o] = code[3 (2 - oy) + (2 - ox), c, o].
  dense: image c HW + p has one spike, at position p in channel c: expected[c HW + p, o] =
  code[c HW + p, o]."""
  _, kind, code_max = next(d for d in DECODERS if d[0] == name)
  o = np.arange(DEC_N)
  ch = np.arange(DEC_C)
  if kind == "conv":
    tap = np.arange(9)
    codes = decoder_code(o[None, None, :], ch[None, :, None], tap[:, None, None], code_max)     # [9, C, N]
    s = np.zeros((DEC_C, 3, 3, DEC_C), np.uint8)
    s[ch, 1, 1, ch] = 1
    expected = np.empty((DEC_C, 3, 3, DEC_N), F32)
    for oy in range(3):
      for ox in range(3):
        expected[:, oy, ox, :] = codes[3 * (2 - oy) + (2 - ox)]
    codes = codes.reshape(3, 3, DEC_C, DEC_N)
  else:
    p = np.arange(DEC_HW)
    codes = decoder_code(o[None, None, :], ch[:, None, None], p[None, :, None], code_max)       # [C, HW, N]
    r = np.arange(DEC_C * DEC_HW)
    s = np.zeros((DEC_C * DEC_HW, DEC_HW, 1, DEC_C), np.uint8)
    s[r, r % DEC_HW, 0, r // DEC_HW] = 1
    expected = codes.reshape(DEC_C * DEC_HW, DEC_N).astype(F32)
    codes = codes.reshape(DEC_C * DEC_HW, DEC_N)
  codes = np.ascontiguousarray(codes, np.int8)
  for a in (s, codes, expected):
    a.setflags(write=False)
  return s, codes, expected


def decoder_mismatches(name, got, limit=8):
  """'' if `got` equals the decoder's expected currents bit for bit, else the first mismatches by
  tap or position, channel, output and code."""
  _, kind, code_max = next(d for d in DECODERS if d[0] == name)
  expected = decoder(name)[2]
  bad = np.argwhere(np.asarray(got).view(np.uint32) != expected.view(np.uint32))
  lines = []
  for idx in bad[:limit]:
    if kind == "conv":
      c, oy, ox, o = (int(v) for v in idx)
      where = "tap %d (kh %d, kw %d)" % (3 * (2 - oy) + (2 - ox), 2 - oy, 2 - ox)
    else:
      r, o = (int(v) for v in idx)
      c, p = divmod(r, DEC_HW)
      where = "position %d" % p
    lines.append("%s: %s, channel %d, output %d: code %d, got %r"
                 % (name, where, c, o, int(expected[tuple(idx)]), float(np.asarray(got)[tuple(idx)])))
  if len(bad) > limit:
    lines.append("... %d mismatches in all" % len(bad))
  return "\n".join(lines)


# ---- the fused dense head (csrc/dense_wide.hip, plan_wide): (T, B, K, N1, N2) -> (RT, CT, csplit) ---
# the shapes of test_dense_head_as_one_launch / test_dense_head_on_float32_rows (tests/test_parity_gpu.py)
HEAD_SHAPES = {
    (20, 256, 2048, 512, 110): (2, 1, 1),
    (6, 5, 208, 200, 70): (4, 1, 0),
    (64, 3, 96, 300, 30): (4, 1, 1),
    (1, 40, 64, 512, 120): (2, 1, 1),
    (9, 131, 1040, 384, 110): (2, 1, 1),
    (3, 77, 320, 160, 50): (4, 1, 0),
    (20, 3000, 96, 300, 30): (4, 2, 0),
    (40, 3, 96, 300, 30): (3, 1, 1),
    (20, 300, 96, 512, 30): (2, 2, 0),
    (40, 260, 96, 300, 30): (3, 2, 0),
}
ALL_HEAD_FORMS = {(2, 1, 1), (4, 1, 0), (4, 1, 1), (4, 2, 0), (3, 1, 1), (2, 2, 0), (3, 2, 0)}
