"""Shared by tests/test_dense_fp6_plans_cpu.py and tests/test_dense_fp6_plans_gpu.py: the table of
small shapes at which every (row tiles, K split) plan of the fp4 x fp6 dense kernel
(csrc/dense_fp6.hip) is forced through SNNQP_DENSE_FP6_PLAN, the launch geometry of a plan restated
from include/snnqp.h (snnqp_dense_fp6_plan), the inputs, and the oracle's results.

The kernel walks K in chunks of 256; the two wave groups of a workgroup take the chunks 2 j + g, so
a workgroup walks `ngc_all` = ceil(chunks / 2) group-chunks, and a K split over `ks` workgroups
hands workgroup z the group-chunks [z gcz, z gcz + gcz) that exist.  Its register and LDS rings
are three deep and its prologue touches group-chunks 0..3, so the counts at which a launch meets
"dead" chunks are 0..5: the K list below reaches each of them at K of a few thousand.

References are computed once per (shape, neuron form), cached, and handed out read-only.
"""
import functools

import numpy as np

from snnquantprune_amd import synthetic as syn
from tests.helpers import packbits_lastaxis, qweight_of

F32 = np.float32
BITS = 4                      # DuQ width of the codes: magnitudes <= 7, exact in fp6

# K -> what its chunk structure reaches
K_LIST = (31,      # one partial spike word
          64,      # exactly one k-step
          65,      # a second k-step of one bit
          257,     # the only chunk of wave group 1 is one bit wide
          513,     # ngc_all = 2: group 1's second chunk is dead
          1025,    # ngc_all = 3
          1600,    # ngc_all = 4
          2305)    # ngc_all = 5; ks = 4: gcz = 2 and the last workgroup is left with 5 - 6 = -1 chunks;
                   # ks = 2: 3 and 2 chunks
# a wave switched off inside a 128-column block, a second block, a ragged last spike word
N_LIST = (33, 70, 129, 160)
KS_LIST = (1, 2, 4)
RT_LIST = (1, 2, 3, 4, 5)
TICKET_BYTES = 4096           # the fixed head of a workspace: one ticket word per tile
MAX_TILES = TICKET_BYTES // 4

# rt -> (T, B) row shapes.  SB = rt * 32 // T samples per workgroup is 1 in one and larger in
# another; B = 8 SB + 1 gives gx = 9 workgroups along the batch (every value of blockIdx.x & 7, so
# the rotated K walk starts at a nonzero chunk wherever a workgroup has two or more) with the last
# one holding a single sample; T = 32 rt fills every row tile, T = 33 / rt = 2 leaves 31 rows dead.
ROWS = {1: ((7, 33), (32, 9)),
        2: ((7, 73), (33, 9), (64, 9)),
        3: ((10, 73), (96, 9)),
        4: ((20, 49), (128, 9)),
        5: ((20, 65), (160, 9))}

# neuron forms: (oracle neuron config, BatchNorm in front)
FORMS = ("mslif", "silent", "bn_lif")


def ceil_div(a, b):
  return -(-a // b)


def ngc_all(K):
  """Group-chunks over all of K: chunks of 256 k, two wave groups."""
  return ceil_div(ceil_div(ceil_div(K, 64), 4), 2)


def gcz_of(K, ks):
  return 0 if ks == 1 else ceil_div(ngc_all(K), ks)


def ngc_per_z(K, ks):
  """Group-chunks each of the `ks` workgroups of a tile walks; `raw` before the clamp at 0."""
  if ks == 1:
    return [ngc_all(K)]
  g = gcz_of(K, ks)
  return [max(0, min(g, ngc_all(K) - z * g)) for z in range(ks)]


def ngc_raw_last(K, ks):
  return ngc_all(K) - (ks - 1) * gcz_of(K, ks)


def sb_of(rt, T):
  return rt * 32 // T


def grid(rt, T, B, N):
  sb = sb_of(rt, T)
  return ceil_div(B, sb), ceil_div(N, 128)


def workspace_bytes(rt, ks, T, B, N):
  """snnqp.h: 4096 + tiles * ks * rt * 32 * 128 * 4 for a split launch, nothing otherwise."""
  if ks == 1:
    return 0
  gx, gy = grid(rt, T, B, N)
  return TICKET_BYTES + gx * gy * ks * rt * 32 * 128 * 4


def row_cases():
  """[(rt, T, B, K, N)]: every row shape of every rt at every K; N walks N_LIST so that every rt
  meets each of them."""
  out, ci = [], 0
  for rt in RT_LIST:
    for T, B in ROWS[rt]:
      for ki, K in enumerate(K_LIST):
        out.append((rt, T, B, K, N_LIST[(ki + ci) % len(N_LIST)]))
      ci += 1
  return out


def plan_cells():
  """[(rt, ks, T, B, K, N)]: the full table the GPU file launches."""
  return [(rt, ks, T, B, K, N) for rt, T, B, K, N in row_cases() for ks in KS_LIST]


# BatchNorm and the LIF-with-decay neuron: one plan per rt
BN_LIF_CELLS = ((1, 4, 7, 33, 2305, 70), (2, 2, 33, 9, 1025, 129), (3, 4, 10, 73, 513, 33),
                (4, 1, 20, 49, 1600, 160), (5, 2, 160, 9, 2305, 160))
# one shape per rt for the cross-check against the int8 formulation (T <= 96)
INT8_CELLS = ((1, 2, 7, 33, 2305, 129), (2, 4, 33, 9, 2305, 70), (3, 2, 96, 9, 1025, 33),
              (4, 4, 20, 49, 2305, 160), (5, 1, 20, 65, 513, 70))
# more tiles than the ticket head has words: 1025 workgroups along the batch, one column block
TICKET_GUARD_CELL = (1, 2, 32, 1025, 513, 33)


@functools.lru_cache(maxsize=None)
def leaf(K, N):
  """Reference-style parameter leaf: DuQ at 4 bits with a = c = 3 sigma, half of the kernel pruned."""
  return syn.quant_leaf((K, N), 4.0, 7100 + 13 * K + N, True, 0.5)


@functools.lru_cache(maxsize=4)
def inputs(T, B, K, N):
  """(spikes uint8 [T, B, K] at density 0.1, u0 float32 [B, N] in [0, 0.5))."""
  rng = np.random.Generator(np.random.PCG64([T, B, K, N]))
  x = (rng.random((T, B, K)) < 0.1).astype(np.uint8)
  u0 = (rng.random((B, N)) * 0.5).astype(F32)
  x.setflags(write=False)
  u0.setflags(write=False)
  return x, u0


@functools.lru_cache(maxsize=None)
def form(name, N):
  """-> (oracle neuron config, BatchNorm dict or None) of a neuron form."""
  if name == "mslif":
    return {"kind": "multi_step_LIF", "tau": 2.0, "v_threshold": 1.0, "v_reset": 0.0}, None
  if name == "silent":       # a threshold no current reaches: u_T depends on every current of every step
    return {"kind": "multi_step_LIF", "tau": 2.0, "v_threshold": 1e30, "v_reset": 0.0}, None
  assert name == "bn_lif"
  rng = np.random.Generator(np.random.PCG64(7700 + N))
  bn = {"mean": rng.normal(0, 0.1, N).astype(F32), "var": (0.5 + rng.random(N)).astype(F32),
        "scale": (0.8 + 0.4 * rng.random(N)).astype(F32), "bias": rng.normal(0, 0.1, N).astype(F32)}
  tau_vec = rng.uniform(-1.0, 1.0, N).astype(F32)
  return {"kind": "LIF", "tau_vec": tau_vec, "v_threshold": 1.0, "v_reset": 0.0}, bn


_EXPECTED = {}
_QWEIGHT = {}


def expected(o, T, B, K, N, name="mslif"):
  """The oracle's (u_T float32 [B, N], spike words uint32 [T, B, ceil(N / 32)], mean rate): exact
  integer sums, dequantisation, [BatchNorm], neuron, from the carried-in u0.  Read-only, cached."""
  key = (T, B, K, N, name)
  if key not in _EXPECTED:
    x, u0 = inputs(T, B, K, N)
    if (K, N) not in _QWEIGHT:
      _QWEIGHT[(K, N)] = qweight_of(o, leaf(K, N), BITS)
    qw = _QWEIGHT[(K, N)]
    cfg, bn = form(name, N)
    if bn is None:
      u, s = o.dense_block(x, qw, cfg, "int", u0=u0)
    else:
      u, s = o.spiking_block(u0, x, lambda xx: o.quant_dense(xx, qw, "int"), o._neuron(cfg),
                             lambda y: o.batchnorm_eval(y, bn["mean"], bn["var"], bn["scale"], bn["bias"], 1e-5))
    u = np.ascontiguousarray(u, dtype=F32)
    words = packbits_lastaxis(s)
    u.setflags(write=False)
    words.setflags(write=False)
    _EXPECTED[key] = (u, words, float(np.mean(s, dtype=np.float64)))
  return _EXPECTED[key]
