"""Shared by tests/test_dense_int8_plans_cpu.py and tests/test_dense_int8_plans_gpu.py: the table of
small shapes at which every row-tile plan of the two int8 dense kernels is forced through its
measurement knob, the inputs, and the oracle's results.

  csrc/dense_mfma.hip   128 columns per workgroup, rt = 1..3 row tiles of 32 rows (uint8 rows: 1..2),
                        SNNQP_DENSE_MFMA_RT; K in chunks of 256, the two wave groups of a workgroup
                        take the chunks 2 j + g, so a group walks ceil(chunks / 2) group-chunks
                        through a ring 4 deep unrolled 4 times (uint8 rows: 3 deep, 6 times)
  csrc/dense_wide.hip   256 ct columns per workgroup (ct = 2 from N = 257 on), rt = 1..4 row tiles
                        holding floor(16 rt / T) samples per lane half, SNNQP_DENSE_WIDE_RT; K in
                        chunks of 128 over three LDS images, the prologue touches chunks 0..3, the
                        walk starts at chunk (blockIdx.x & 7) chunks / 8

The leaves are DuQ at EIGHT bits: 4-bit codes fit fp6 and would run csrc/dense_fp6.hip instead.
References are computed once per (shape, data, neuron form), cached, and handed out read-only; the
integer currents of a (shape, data) are shared by its neuron forms."""
import functools

import numpy as np

from snnquantprune_amd import synthetic as syn
from tests.helpers import packbits_lastaxis, qweight_of

F32 = np.float32
BITS = 8                      # DuQ width of the codes: magnitudes up to 127, beyond fp6

# ---- K lists: K -> what its chunk structure reaches --------------------------------------------------
# 128-column kernel, bit rows: group-chunk counts 1..7 (chunks of 256, two wave groups)
MFMA_K_BITS = (31,     # one partial spike word: one group-chunk, group 1 has none
               256,    # exactly one chunk: group 1's only chunk is dead
               257,    # group 1's only chunk is one bit wide
               513,    # 3 chunks, 2 group-chunks: group 1's second chunk is dead
               1025,   # 5 chunks, 3 group-chunks: the ring not yet full
               1537,   # 7 chunks, 4 group-chunks: the ring (D = 4) and one unrolled body (U = 4) exactly
               2049,   # 9 chunks, 5 group-chunks: a second body of one live chunk and three dead ones
               2561,   # 11 chunks, 6 group-chunks: two live, two dead
               3073)   # 13 chunks, 7 group-chunks: three live, one dead
# 128-column kernel, uint8 rows (K % 16 == 0): the same chunk counts, the last chunk 16 bytes wide
MFMA_K_U8 = (16,       # one 16-byte piece: one group-chunk
             256,      # exactly one chunk
             272,      # group 1's only chunk is one piece wide
             528,      # 2 group-chunks, group 1's second chunk dead
             1040,     # 3 group-chunks: the ring (D = 3) exactly
             1552,     # 4 group-chunks
             2064,     # 5 group-chunks
             2576,     # 6 group-chunks: one unrolled body (U = 6) exactly
             3088)     # 7 group-chunks: a second body of one live chunk
# wide kernel, bit rows: 1..7 chunks of 128 (nsteps is rounded up to 3, 6, 9)
WIDE_K_BITS = (31,     # 1 chunk, a partial spike word; two dead steps
               128,    # 1 chunk exactly
               129,    # 2 chunks, the second one bit wide; one dead step
               257,    # 3 chunks: one round of the three LDS images
               385,    # 4 chunks: every chunk the prologue touches is live
               513,    # 5 chunks: staging four ahead reaches its first chunk beyond the prologue
               641,    # 6 chunks: two rounds
               769)    # 7 chunks: a third round with two dead steps
# wide kernel, uint8 and float32 rows: the same chunk counts, the last chunk 16 elements wide
WIDE_K_U8 = (16, 128, 144, 272, 400, 528, 656, 784)

# ---- N lists -------------------------------------------------------------------------------------------
MFMA_N = (33, 70, 128)        # a wave of one live column, a ragged last spike word, the full block
MFMA_N_LONG = (129, 160)      # a second column block: the 128-column kernel has N > 128 for T > 64 only
# wide kernel, by column tiles: 129 a lone live column in wave 4, 160 a ragged last spike word inside
# column tile 0, 256 the full tile; 257 and 300: ct = 2 with waves switched off
WIDE_N = {1: (129, 160, 256), 2: (257, 300)}
WIDE_N_BLOCKS = (512, 513, 700)      # ct = 2 filled exactly; a second column block (gy = 2), nearly empty and ragged
WIDE_N_ALL = (129, 160, 256, 257, 300, 512, 513, 700)

# ---- row shapes: plan -> ((T, B), ...) ------------------------------------------------------------------
# 128-column kernel: SB = 32 rt // T samples per workgroup.  T = 32 rt fills the row tiles; T = 20
# gives SB = 1, 3, 4; B = 8 SB + 1: nine workgroups along the batch, the last one with ONE sample.
# (20, 24) at rt = 2 is the even-tailed batch: eight full workgroups.
MFMA_ROWS = {1: ((32, 9), (20, 9), (7, 33)),
             2: ((64, 9), (20, 25), (33, 9), (20, 24)),
             3: ((96, 9), (20, 33), (65, 9))}
MFMA_PLANS = (("bits", 1), ("bits", 2), ("bits", 3), ("u8", 1), ("u8", 2))
# wide kernel: sph = 16 rt // T samples per lane half, 2 sph per workgroup.  T = 16 rt fills the
# rows of a half; T = 3 or 5 holds several samples and leaves a row dead; T = 16 (rt - 1) + 1 has
# sph = 1 and 15 dead rows per half (rt = 1: T = 5, one dead row).  B = 16 sph + 1: nine workgroups
# along the batch -- every value of blockIdx.x & 7, so the rotated K walk starts at every offset --
# the last one with ONE sample: its lane half 1 has none.  (3, 160) at rt = 2 is the even-tailed batch.
WIDE_ROWS = {1: ((16, 17), (3, 81), (5, 49)),
             2: ((32, 17), (3, 161), (17, 17), (3, 160)),
             3: ((48, 17), (5, 145), (33, 17)),
             4: ((64, 17), (5, 193), (49, 17))}
WIDE_PLANS = tuple((rt, ct) for rt in (1, 2, 3, 4) for ct in (1, 2))


def ceil_div(a, b):
  return -(-a // b)


def mfma_group_chunks(K):
  """Group-chunks a wave group of the 128-column kernel walks: chunks of 256 k, two groups."""
  return ceil_div(ceil_div(K, 256), 2)


def wide_chunks(K):
  return ceil_div(K, 128)


def mfma_sb(rt, T):
  return 32 * rt // T


def mfma_grid(rt, T, B, N):
  return ceil_div(B, mfma_sb(rt, T)), ceil_div(N, 128)


def wide_sph(rt, T, fused=False):
  return min(16 * rt // T, 8 if fused else 64)


def wide_ct(N):
  return 2 if N > 256 else 1


def wide_grid(rt, T, B, N, fused=False):
  return ceil_div(B, 2 * wide_sph(rt, T, fused)), 1 if fused else ceil_div(N, 256 * wide_ct(N))


def mfma_k_list(in_type):
  return MFMA_K_BITS if in_type == "bits" else MFMA_K_U8


def wide_k_list(kind):
  return WIDE_K_BITS if kind == "bits" else WIDE_K_U8


def _three(ks):
  """Three K of a list for the cells outside the full sweep: the smallest, a ragged middle, the largest."""
  return (ks[0], ks[len(ks) // 2], ks[-1])


def mfma_cells(in_type, rt):
  """[(T, B, K, N)] of one plan of the 128-column kernel: every row shape at every K; N walks its
  list so that every rt meets every N.  Rows of more than 64 steps (bit rows, rt = 3) also walk the
  two N beyond one column block."""
  out, ci = [], 0
  for T, B in MFMA_ROWS[rt]:
    if in_type == "u8" and T > 64:
      continue
    ns = MFMA_N + (MFMA_N_LONG if T > 64 else ())
    for ki, K in enumerate(mfma_k_list(in_type)):
      out.append((T, B, K, ns[(ki + ci) % len(ns)]))
    ci += 1
  return out


def wide_cells(rt, ct, kind):
  """[(T, B, K, N)] of one plan of the wide kernel on rows of `kind` ("bits": the bit rows' K list,
  "u8": the K list of uint8 and float32 rows): every row shape at every K with N walking the N of
  this ct up to 300; for ct = 2 each N of WIDE_N_BLOCKS at three K, walking the row shapes."""
  out, ci = [], 0
  ks = wide_k_list(kind)
  for T, B in WIDE_ROWS[rt]:
    ns = WIDE_N[ct]
    for ki, K in enumerate(ks):
      out.append((T, B, K, ns[(ki + ci) % len(ns)]))
    ci += 1
  if ct == 2:
    rows = WIDE_ROWS[rt]
    for ni, N in enumerate(WIDE_N_BLOCKS):
      for ki, K in enumerate(_three(ks)):
        T, B = rows[(ni + ki + rt) % len(rows)]
        out.append((T, B, K, N))
  return out


# BatchNorm and the LIF-with-decay neuron: one cell per plan of both kernels
MFMA_BN_CELLS = (("bits", 1, 7, 33, 3073, 70), ("bits", 2, 33, 9, 1025, 33), ("bits", 3, 65, 9, 513, 160),
                 ("u8", 1, 20, 9, 3088, 128), ("u8", 2, 20, 25, 528, 70))
# (rt, ct, kind, T, B, K, N)
WIDE_BN_CELLS = ((1, 1, "bits", 3, 81, 769, 160), (1, 2, "u8", 5, 49, 784, 300), (2, 1, "u8", 17, 17, 528, 129),
                 (2, 2, "bits", 3, 161, 513, 700), (3, 1, "bits", 33, 17, 641, 256), (3, 2, "u8", 5, 145, 400, 513),
                 (4, 1, "u8", 5, 193, 656, 160), (4, 2, "bits", 49, 17, 385, 257))
# rows with strides: one plan per rt at the raggedest K (a partial last chunk in the deepest walk)
MFMA_STRIDE_CELLS = (("bits", 1, 7, 33, 3073, 70), ("bits", 2, 20, 25, 3073, 33), ("bits", 3, 65, 9, 3073, 129),
                     ("u8", 1, 20, 9, 3088, 70), ("u8", 2, 33, 9, 3088, 128))
WIDE_STRIDE_CELLS = ((1, 2, 5, 49, 300), (2, 1, 17, 17, 160), (3, 2, 5, 145, 513), (4, 1, 49, 17, 129))   # (rt, ct, T, B, N)
WIDE_STRIDE_K = {"bits": 769, "u8": 784}
# plans that ship, without the knob: (in_type, T, B, K, N) -> (rt, sb)
SHIPPED_CELLS = {("bits", 20, 801, 513, 110): (3, 4), ("u8", 20, 601, 528, 110): (2, 3)}
# the fused head at RT = 1: (T, B, K, N1, N2) by the (rt, ct, csplit) form it is forced into
HEAD_N2, HEAD_GROUP = 110, 10
HEAD_CELLS = {(1, 1, 0): (16, 17, 144, 160, HEAD_N2),
              (1, 2, 0): (5, 17, 400, 300, HEAD_N2),
              (1, 1, 1): (16, 17, 272, 512, HEAD_N2)}
HEAD_STATE_FORM = (1, 1, 1)    # two windows of T against one stateless window of 2 T <= 16
HEAD_STATE_CELL = (8, 17, 272, 300, HEAD_N2)


@functools.lru_cache(maxsize=None)
def leaf(K, N):
  """Reference-style parameter leaf: DuQ (8 bits here) with a = c = 3 sigma, half of the kernel pruned."""
  return syn.quant_leaf((K, N), 4.0, 7100 + 13 * K + N, True, 0.5)


_QWEIGHT = {}


def qweight(o, K, N):
  """The oracle's weight of leaf(K, N) at 8 bits.  Code magnitudes must exceed 7: codes that fit
  fp6 would be taken by the fp4 x fp6 kernel and this table would test the wrong one."""
  if (K, N) not in _QWEIGHT:
    qw = qweight_of(o, leaf(K, N), BITS)
    assert int(np.abs(qw.q).max()) > 7, (K, N, "codes that fit fp6")
    _QWEIGHT[(K, N)] = qw
  return _QWEIGHT[(K, N)]


@functools.lru_cache(maxsize=4)
def inputs(T, B, K, N, data="binary"):
  """(rows uint8 [T, B, K], u0 float32 [B, N] in [0, 0.5)).  "binary": spikes at density 0.1;
  "counts": Poisson 0.15 with 0.2 % of the entries 255 and x[0, 0, :3] = (128, 127, 200) -- the
  offset of the x - 128 operand, its neighbour and a large count."""
  rng = np.random.Generator(np.random.PCG64([T, B, K, N]))
  x = (rng.random((T, B, K)) < 0.1).astype(np.uint8)
  if data == "counts":
    x = np.minimum(rng.poisson(0.15, (T, B, K)), 255).astype(np.uint8)
    x[rng.random(x.shape) < 0.002] = 255
    x[0, 0, :3] = (128, 127, 200)
  else:
    assert data == "binary"
  u0 = (rng.random((B, N)) * 0.5).astype(F32)
  x.setflags(write=False)
  u0.setflags(write=False)
  return x, u0


@functools.lru_cache(maxsize=None)
def form(name, N):
  """-> (oracle neuron config, BatchNorm dict or None, carried-in state?) of a neuron form."""
  mslif = {"kind": "multi_step_LIF", "tau": 2.0, "v_threshold": 1.0, "v_reset": 0.0}
  if name == "mslif":
    return mslif, None, True
  if name == "silent":       # a threshold no current reaches: u_T depends on every current of every step
    return dict(mslif, v_threshold=1e30), None, True
  if name == "no_state":     # u0 and u_out both null: the walk that keeps no potential in memory
    return mslif, None, False
  rng = np.random.Generator(np.random.PCG64(7700 + N))
  bn = {"mean": rng.normal(0, 0.1, N).astype(F32), "var": (0.5 + rng.random(N)).astype(F32),
        "scale": (0.8 + 0.4 * rng.random(N)).astype(F32), "bias": rng.normal(0, 0.1, N).astype(F32)}
  tau_vec = rng.uniform(-1.0, 1.0, N).astype(F32)
  if name == "no_state_bn":
    return mslif, bn, False
  assert name == "bn_lif"
  return {"kind": "LIF", "tau_vec": tau_vec, "v_threshold": 1.0, "v_reset": 0.0}, bn, True


@functools.lru_cache(maxsize=2)
def _currents(o, T, B, K, N, data):
  x, _ = inputs(T, B, K, N, data)
  y = o.quant_dense(x, qweight(o, K, N), "int")          # exact integer sums, dequantised: [T, B, N]
  y.setflags(write=False)
  return y


_EXPECTED = {}


def expected(o, T, B, K, N, name="mslif", data="binary"):
  """The oracle's (u_T float32 [B, N], spike words uint32 [T, B, ceil(N / 32)], mean rate): exact
  integer sums, dequantisation, [BatchNorm], neuron, from the carried-in u0 (the no_state forms:
  from zero).  Read-only, cached."""
  key = (T, B, K, N, name, data)
  if key not in _EXPECTED:
    _, u0 = inputs(T, B, K, N, data)
    cfg, bn, state = form(name, N)
    norm = None if bn is None else (
        lambda y: o.batchnorm_eval(y, bn["mean"], bn["var"], bn["scale"], bn["bias"], 1e-5))
    u, s = o.spiking_block(u0 if state else None, _currents(o, T, B, K, N, data), lambda y: y, o._neuron(cfg), norm)
    u = np.ascontiguousarray(u, dtype=F32)
    words = packbits_lastaxis(s)
    u.setflags(write=False)
    words.setflags(write=False)
    _EXPECTED[key] = (u, words, float(np.mean(s, dtype=np.float64)))
  return _EXPECTED[key]


# ---- the fused head -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def head_leaves(K, N1, N2):
  return (syn.quant_leaf((K, N1), 4.0, 8100 + 13 * K + N1, True, 0.5),
          syn.quant_leaf((N1, N2), 4.0, 8300 + 13 * N1 + N2, True, 0.5))


@functools.lru_cache(maxsize=8)
def head_inputs(T, B, K, data):
  """Rows uint8 [T, B, K] of the head: "binary" spikes at density 0.1 or "counts" as inputs()."""
  rng = np.random.Generator(np.random.PCG64([T, B, K, 5]))
  x = (rng.random((T, B, K)) < 0.1).astype(np.uint8)
  if data == "counts":
    x = np.minimum(rng.poisson(0.15, (T, B, K)), 255).astype(np.uint8)
    x[rng.random(x.shape) < 0.002] = 255
    x[0, 0, :3] = (128, 127, 200)
  x.setflags(write=False)
  return x


_HEAD = {}


def head_expected(o, T, B, K, N1, N2, data):
  """oracle.dense2_forward on the head's rows -> {"s1", "s2" spike words, "logits", "rate1", "rate2",
  "counts" int32 [B, N2]}."""
  key = (T, B, K, N1, N2, data)
  if key not in _HEAD:
    l1, l2 = head_leaves(K, N1, N2)
    q1, q2 = qweight_of(o, l1, BITS), qweight_of(o, l2, BITS)
    assert int(np.abs(q1.q).max()) > 7 and int(np.abs(q2.q).max()) > 7
    e = o.dense2_forward(head_inputs(T, B, K, data), q1, q2, mode="int", group=HEAD_GROUP)
    r = {"s1": packbits_lastaxis(e["s1"]), "s2": packbits_lastaxis(e["s2"]),
         "logits": np.ascontiguousarray(e["logits"], dtype=F32),
         "u1": np.ascontiguousarray(e["u1"], dtype=F32), "u2": np.ascontiguousarray(e["u2"], dtype=F32),
         "counts": np.asarray(e["s2"] != 0).sum(0).astype(np.int32),
         "rate1": float(np.mean(e["s1"], dtype=np.float64)), "rate2": float(np.mean(e["s2"], dtype=np.float64))}
    for v in r.values():
      if isinstance(v, np.ndarray):
        v.setflags(write=False)
    _HEAD[key] = r
  return _HEAD[key]
