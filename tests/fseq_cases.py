"""The float32-MFMA connection (csrc/fseq_gemm.hip) one launch at a time: the table of cases that
reaches each of its 14 instantiations at the smallest shapes where it can go wrong, their data,
and a plain reference.  No GPU here; tests/test_fseq_gemm_cpu.py and test_fseq_gemm_gpu.py use it.

The contract (include/snnqp.h, snnqp_conv_forward): y[m][n] = the float32 fmaf chain from +0 over
k ascending of x[m][k] w[k][n], rows m = (image, oy, ox), k = (kh, kw, cin), a tap outside the
image reading 0.0.  The reference gathers x[m][k] with explicit index ranges (no padded copy, so
it shares nothing with oracle.im2col) and runs oracle.fseq_matmul, the C fmaf chain.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import snn_oracle as oracle
from tests.helpers import packbits_lastaxis
from tests.train_helpers import mixed

F32 = np.float32

# kind "f32" / "u8" / "bits"; NB images of H x W x Cin; KH x KW kernel to Cout; pads ((top, bottom),
# (left, right)); form = (staging mode, tile) the entry claims; offset: the uint8 tensor starts this
# many bytes past an aligned address; nonfinite: inf and NaN in x
Case = namedtuple("Case", "name kind NB H W Cin Cout ks pads form offset nonfinite")

P0 = ((0, 0), (0, 0))
P1 = ((1, 1), (1, 1))
P2 = ((2, 2), (2, 2))


def _c(name, kind, NB, H, W, Cin, Cout, ks, pads, form, offset=0, nonfinite=False):
  return Case(name, kind, NB, H, W, Cin, Cout, tuple(ks), pads, tuple(form), offset, nonfinite)


# M = NB H W, K = KH KW Cin, N = Cout.
# Small tile: M on 1, 63, 64, 65, 129 (one row; one short of, exactly, one past a tile; a third
# tile of one row); N on 1, 31, 33, 63, 64, 65 (N % 4 != 0: the scalar B path; 64: the vector path;
# 65: a second column tile of one column); K on 1, 15, 16, 17, 33 and >= 48 (chunks of 16, two LDS
# buffers: from 48 on buffer 0 is written a second time).
SMALL = [
    # float32, mode 2 (element by element): Cin 1, 3, 2, 17
    _c("f32_m2_one_of_everything", "f32", 1, 1, 1, 1, 1, (1, 1), P0, (2, 64)),                  # M 1 K 1 N 1
    _c("f32_m2_cin3_1x5_k15", "f32", 1, 7, 9, 3, 31, (1, 5), ((0, 0), (2, 2)), (2, 64)),       # M 63 K 15 N 31
    _c("f32_m2_cin2_3x3_n65", "f32", 1, 3, 43, 2, 65, (3, 3), P1, (2, 64)),                    # M 129 K 18 N 65
    _c("f32_m2_dense_k17", "f32", 65, 1, 1, 17, 33, (1, 1), P0, (2, 64)),                      # M 65 K 17 N 33
    # float32, mode 1 (runs of 4 channels): Cin 4, 12
    _c("f32_m1_cin4_1x4_pads_1_2", "f32", 1, 5, 13, 4, 63, (1, 4), ((0, 0), (1, 2)), (1, 64)),  # M 65 K 16 N 63
    _c("f32_m1_cin12_uneven_pads", "f32", 1, 7, 9, 12, 33, (3, 3), ((0, 2), (2, 0)), (1, 64)),  # M 63 K 108 N 33
    # float32, mode 0 (a chunk in one tap): Cin 16 (a tap is one chunk), 48 (three)
    _c("f32_m0_cin16_1x1", "f32", 1, 8, 8, 16, 64, (1, 1), P0, (0, 64)),                       # M 64 K 16 N 64
    _c("f32_m0_cin48_3x3_on_1x1_image", "f32", 129, 1, 1, 48, 31, (3, 3), P1, (0, 64)),        # M 129 K 432: 8 of 9 taps are padding
    _c("f32_m0_cin16_5x5", "f32", 1, 8, 8, 16, 1, (5, 5), P2, (0, 64)),                        # M 64 K 400 N 1
    _c("f32_m0_nonfinite_x", "f32", 1, 5, 13, 16, 33, (3, 3), P1, (0, 64), nonfinite=True),    # M 65 K 144 N 33
    # uint8, mode 2: the 2-channel event input; a dense row of 33 (no multiple of 8)
    _c("u8_m2_cin2_3x3_n65", "u8", 1, 3, 43, 2, 65, (3, 3), P1, (2, 64)),                      # M 129 K 18 N 65
    _c("u8_m2_dense_k33", "u8", 63, 1, 1, 33, 64, (1, 1), P0, (2, 64)),                        # M 63 K 33 N 64
    # uint8, mode 3: dense rows of 24 (% 8, not % 16), a 1 x 1 kernel on an image, 3 x 3 with Cin 16
    _c("u8_m3_dense_k24", "u8", 65, 1, 1, 24, 31, (1, 1), P0, (3, 64)),                        # M 65 K 24 N 31
    _c("u8_m3_cin8_1x1", "u8", 1, 5, 13, 8, 1, (1, 1), P0, (3, 64)),                           # M 65 K 8 N 1
    _c("u8_m3_cin16_3x3", "u8", 1, 7, 9, 16, 33, (3, 3), P1, (3, 64)),                         # M 63 K 144 N 33
    # uint8 off 8-byte alignment: mode 2 on shapes that are mode 3 when aligned
    _c("u8_odd_address_cin16_3x3", "u8", 1, 5, 13, 16, 64, (3, 3), P1, (2, 64), offset=1),     # M 65 K 144 N 64
    _c("u8_odd_address_dense_k24", "u8", 64, 1, 1, 24, 33, (1, 1), P0, (2, 64), offset=3),     # M 64 K 24 N 33
    # spike words, mode 2: Cin 40 (no multiple of 16) under a 3 x 3 kernel
    _c("bits_m2_cin40_3x3", "bits", 1, 8, 8, 40, 63, (3, 3), P1, (2, 64)),                     # M 64 K 360 N 63
    # spike words, mode 3: a ragged dense row; 3 x 3 with a tap inside a word, on a word, across words
    _c("bits_m3_dense_k50", "bits", 129, 1, 1, 50, 65, (1, 1), P0, (3, 64)),                   # M 129 K 50 N 65
    _c("bits_m3_cin16_3x3", "bits", 1, 7, 9, 16, 31, (3, 3), P1, (3, 64)),                     # M 63 K 144 N 31
    _c("bits_m3_cin32_3x3", "bits", 1, 5, 13, 32, 33, (3, 3), P1, (3, 64)),                    # M 65 K 288 N 33
    _c("bits_m3_cin48_3x3", "bits", 1, 8, 8, 48, 64, (3, 3), P1, (3, 64)),                     # M 64 K 432 N 64
]

# Large tile: ceil(M / 128) ceil(N / 128) >= 192 and N > 64, reached with a thin K.  Rows: 3 x 91 x 90
# = 24570 (192 row tiles, the last of 122 rows) for one column tile; 111 x 110 = 12210 (96, the last of
# 50) for two; 90 x 90 = 8100 (64, the last of 36) for three.  Columns ragged in the last tile below
# its 64-column half (129, 257: one column) and above it (70, 100: 6 and 36 columns in the upper half);
# 100 and 72 take the vector B path.
LARGE = [
    _c("f32_m0_big_cin16_3x3_n70", "f32", 3, 91, 90, 16, 70, (3, 3), P1, (0, 128)),            # K 144
    _c("f32_m1_big_cin4_3x3_n257", "f32", 1, 90, 90, 4, 257, (3, 3), P1, (1, 128)),            # K 36
    _c("f32_m2_big_cin3_3x3_n129", "f32", 1, 111, 110, 3, 129, (3, 3), P1, (2, 128)),          # K 27
    _c("u8_m3_big_cin16_3x3_n100", "u8", 3, 91, 90, 16, 100, (3, 3), P1, (3, 128)),            # K 144
    _c("u8_m3_big_dense_k24_n129", "u8", 12170, 1, 1, 24, 129, (1, 1), P0, (3, 128)),          # K 24: the second load of a thread ends the row
    _c("u8_m2_big_cin2_3x3_n129", "u8", 1, 111, 110, 2, 129, (3, 3), P1, (2, 128)),            # K 18
    _c("u8_odd_address_big_cin16_n72", "u8", 3, 91, 90, 16, 72, (1, 1), P0, (2, 128), offset=5),   # K 16
    _c("bits_m3_big_cin16_3x3_n257", "bits", 1, 90, 90, 16, 257, (3, 3), P1, (3, 128)),        # K 144
    _c("bits_m3_big_dense_k50_n257", "bits", 8100, 1, 1, 50, 257, (1, 1), P0, (3, 128)),       # K 50
    _c("bits_m2_big_cin8_3x3_n129", "bits", 1, 111, 110, 8, 129, (3, 3), P1, (2, 128)),        # K 72
]

CASES = SMALL + LARGE
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the 14 instantiations of fseq_gemm_kernel<MODE, IN, TM>
ALL_FORMS = {(k, m, t) for t in (64, 128) for k, ms in (("f32", (0, 1, 2)), ("u8", (2, 3)), ("bits", (2, 3)))
             for m in ms}

# float32 kernels the connection does not serve (fseq_gemm_unsupported): strided, dilated, an output
# that is not the input's size -- (H, W, Cin, Cout, ks, stride, pads, kernel dilation)
DIRECT = [
    ("strided", 8, 8, 16, 32, (3, 3), (2, 2), P1, (1, 1)),
    ("dilated", 8, 8, 16, 32, (3, 3), (1, 1), ((2, 2), (2, 2)), (2, 2)),
    ("valid_padding", 8, 8, 16, 32, (3, 3), (1, 1), P0, (1, 1)),
    ("pad_wider_than_same", 8, 8, 16, 32, (3, 3), (1, 1), ((1, 2), (1, 1)), (1, 1)),
]

# the tile rule at its edges: (name, NB rows of a dense layer, N, tile)
TILE_EDGES = [
    ("191_tiles", 191 * 128, 65, 64),
    ("192_tiles", 191 * 128 + 1, 65, 128),                   # a 192nd row tile of one row
    ("n65_192_full_tiles", 192 * 128, 65, 128),
    ("190_tiles_two_columns", 95 * 128, 129, 64),            # 95 x 2
    ("192_tiles_two_columns", 95 * 128 + 1, 129, 128),       # 96 x 2
    ("189_tiles_three_columns", 63 * 128, 257, 64),          # 63 x 3
    ("192_tiles_three_columns", 63 * 128 + 1, 257, 128),     # 64 x 3
    ("n64_192_tiles", 191 * 128 + 1, 64, 64),
    ("n64_many_rows", 1 << 20, 64, 64),
    ("n1_many_rows", 1 << 20, 1, 64),
    ("n128_one_column_tile", 191 * 128 + 1, 128, 128),
]

IN_TYPES = {"f32": 0, "u8": 1, "bits": 2}            # SNNQP_F32 / SNNQP_U8 / SNNQP_BITS


def dims(c):
  """(M, K, N) of a case."""
  return c.NB * c.H * c.W, c.ks[0] * c.ks[1] * c.Cin, c.Cout


def _seed(c):
  return 4000 + CASES.index(c)


@lru_cache(maxsize=None)
def data(name):
  """(x as the kernel reads it, x as float32 [NB, H, W, Cin], w float32 [KH, KW, Cin, Cout]).
  float32: mixed magnitudes, so that any other summation order shows in the bits; uint8: Poisson
  counts with a few values up to 255; bits: spikes at about 0.2, packed into words."""
  c = BY_NAME[name]
  rng = np.random.Generator(np.random.PCG64(_seed(c)))
  shape = (c.NB, c.H, c.W, c.Cin)
  w = mixed(rng, c.ks + (c.Cin, c.Cout))
  if c.kind == "f32":
    x = mixed(rng, shape)
    if c.nonfinite:
      flat = x.reshape(-1)
      idx = rng.choice(flat.size, 9, replace=False)
      flat[idx[:3]], flat[idx[3:6]], flat[idx[6:]] = np.inf, -np.inf, np.nan
    xk = x
  elif c.kind == "u8":
    xk = rng.poisson(0.7, shape).astype(np.uint8)
    flat = xk.reshape(-1)
    flat[rng.choice(flat.size, max(1, flat.size // 89), replace=False)] = 129
    flat[rng.choice(flat.size, max(1, flat.size // 97), replace=False)] = 255
    x = xk.astype(F32)
  else:
    s = (rng.random(shape) < 0.2).astype(np.uint8)
    s.reshape(-1, c.Cin)[0, -1] = 1                      # the last channel of a row's last word fires
    xk = packbits_lastaxis(s)
    x = s.astype(F32)
  for a in (xk, x, w):
    a.setflags(write=False)
  return xk, x, w


def im2col(x, ks, pads):
  """[NB, H, W, C] -> [NB H W, KH KW C]: column (kh, kw, c) of row (img, oy, ox) is
  x[img, oy + kh - top, ox + kw - left, c], or the literal 0.0 outside the image (output size =
  input size: pads sum to K - 1)."""
  NB, H, W, C = x.shape
  (KH, KW), ((pt, pb), (pl, pr)) = ks, pads
  assert pt + pb == KH - 1 and pl + pr == KW - 1
  cols = np.zeros((NB, H, W, KH, KW, C), F32)
  for kh in range(KH):
    oy0, oy1 = max(0, pt - kh), min(H, H + pt - kh)      # rows whose tap kh lies inside the image
    if oy0 >= oy1:
      continue
    for kw in range(KW):
      ox0, ox1 = max(0, pl - kw), min(W, W + pl - kw)
      if ox0 >= ox1:
        continue
      cols[:, oy0:oy1, ox0:ox1, kh, kw, :] = x[:, oy0 + kh - pt:oy1 + kh - pt, ox0 + kw - pl:ox1 + kw - pl, :]
  return cols.reshape(NB * H * W, KH * KW * C)


@lru_cache(maxsize=None)
def reference(name):
  """float32 [NB, H, W, Cout]: the fmaf chain on the gathered rows.  Computed once per process,
  read-only."""
  c = BY_NAME[name]
  _, x, w = data(name)
  M, K, N = dims(c)
  y = oracle.fseq_matmul(im2col(x, c.ks, c.pads), w.reshape(K, N)).reshape(c.NB, c.H, c.W, N)
  y.setflags(write=False)
  return y
