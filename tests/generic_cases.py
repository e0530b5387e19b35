"""Geometries of the direct-form block (csrc/generic_block.hip) off the 3x3 / stride 1 / pad 1
path, shared by tests/test_generic_block_cpu.py (the oracle against torch) and
tests/test_generic_block_gpu.py (the kernel against the oracle).

Each row: name, spatial, Cin, Cout, kernel, strides, padding, input dilation, kernel dilation,
groups, batch, expected output spatial size (worked out by hand from flax_qconv.py:114-144 and
lax.conv_general_dilated's shape rule; asserted literally by the CPU test).
"""
import zlib
from collections import namedtuple

import numpy as np

from snnquantprune_amd import synthetic as syn
from tests.helpers import qweight_of

F32 = np.float32

Geom = namedtuple("Geom", "name spatial cin cout kernel strides padding in_dil k_dil groups B out")

T = 4
DENSITY = 0.3
GAIN = 5.0
CODES = ((4, 0.5), (8, 0.3))            # (bits, pruned fraction)

TABLE = [
    # everything at once; groups start at bits 16 and 32 of the packed input; ragged Cout
    Geom("dilated_grouped", (9, 11), 48, 66, (3, 2), (2, 1), ((1, 2), (0, 1)), (1, 2), (2, 1), 3, 2, (4, 21)),
    # group 1 starts at bit 40 and spans two words; Cout % 32 == 0: ballot output
    Geom("group_straddles_word", (6, 7), 80, 64, (3, 3), (1, 1), "SAME", None, None, 2, 2, (6, 7)),
    # CinG = CoutG = 1
    Geom("depthwise", (8, 6), 33, 33, (3, 3), (1, 1), "SAME", None, None, 33, 2, (8, 6)),
    # output odd in both axes under the pool
    Geom("k5_stride2_valid", (13, 17), 5, 40, (5, 5), (2, 2), "VALID", None, None, 1, 2, (5, 7)),
    # the reference resolves SAME as if the dilation were 1 (flax_qconv.py:129-142): 8x8, not 10x10
    Geom("same_kernel_dilation", (10, 10), 4, 32, (3, 3), (1, 1), "SAME", None, (2, 2), 1, 2, (8, 8)),
    # transposed-convolution shape
    Geom("input_dilation", (5, 6), 8, 36, (3, 3), (1, 1), ((2, 2), (2, 2)), (2, 2), None, 1, 2, (11, 13)),
    # most taps fall in the padding
    Geom("kernel_larger_than_image", (2, 3), 3, 34, (5, 5), (1, 1), "SAME", None, None, 1, 2, (2, 3)),
    # 1-D runs as H = 1
    Geom("1d_dilated_stride", (23,), 32, 96, (3,), (2,), ((3, 3),), None, (3,), 1, 2, (12,)),
    # the TCJA convolution, as a block
    Geom("1d_same_k4", (10,), 5, 7, (4,), (1,), "SAME", None, None, 1, 2, (10,)),
    # the dilated, grouped case of test_quant_conv_3d
    Geom("explicit_dilated_grouped", (4, 5, 6), 6, 64, (2, 3, 2), (1, 2, 1), ((1, 0), (1, 2), (0, 1)),
         (1, 2, 1), (2, 1, 2), 2, 3, (3, 5, 5)),
]
BY_NAME = {g.name: g for g in TABLE}
NAMES = [g.name for g in TABLE]


def seed_of(name, bits=0):
  """A seed derived from the case name (and the bit width)."""
  return (zlib.crc32(name.encode()) + 7919 * bits) & 0x3FFFFFFF


def oracle_kwargs(g):
  """What oracle.quant_conv / oracle.conv_block take for the geometry."""
  return dict(strides=g.strides, padding=g.padding, input_dilation=g.in_dil, kernel_dilation=g.k_dil,
              feature_group_count=g.groups)


def conv_kwargs(g):
  """What QuantConv takes for the geometry."""
  kw = dict(strides=g.strides, padding=g.padding, feature_group_count=g.groups)
  if g.in_dil is not None:
    kw["input_dilation"] = g.in_dil
  if g.k_dil is not None:
    kw["kernel_dilation"] = g.k_dil
  return kw


def mixed_magnitudes(rng, shape):
  """Real-valued float32 whose sum depends on the order it is taken in."""
  return (rng.standard_normal(shape) * 2.0 ** rng.integers(-6, 7, size=shape)).astype(F32)


def build(o, name, bits):
  """Everything a test needs for one row at one bit width, from a seed derived from the name:
  leaf (reference-style parameters), qw (oracle.QWeight), bn (dict), x (uint8 spikes
  [T, B, *spatial, Cin]), u0 (float32 [B, *out, Cout]), xr (real-valued float32 like x)."""
  g = BY_NAME[name]
  prune = dict(CODES)[bits]
  seed = seed_of(name, bits)
  leaf = syn.quant_leaf(tuple(g.kernel) + (g.cin // g.groups, g.cout), GAIN, seed, True, prune)
  bp, bs = syn.bn_leaf(g.cout, True, seed + 1)
  bn = dict(mean=bs["mean"], var=bs["var"], scale=bp["scale"], bias=bp["bias"])
  rng = np.random.Generator(np.random.PCG64(seed + 2))
  x = (rng.random((T, g.B) + tuple(g.spatial) + (g.cin,)) < DENSITY).astype(np.uint8)
  u0 = (0.3 * rng.standard_normal((g.B,) + tuple(g.out) + (g.cout,))).astype(F32)
  xr = mixed_magnitudes(rng, x.shape)
  return dict(g=g, bits=bits, leaf=leaf, qw=qweight_of(o, leaf, bits), bn=bn, x=x, u0=u0, xr=xr)
