"""Exact threshold ties for the fused forward epilogues.

DuQ takes its codes from `a` and its scale from `c` (quant.py:443,466-467).  With `a` left at
gaussian_init(W) the codes use their whole range; with c = L * 2^-k (L = n_lv - 1) the current
fl(fl(acc / L) * c) is acc * 2^-k for almost every accumulator, so currents -- and, with a
power-of-two tau and dyadic v_threshold / v_reset, membrane potentials -- sit on a dyadic grid and
land EXACTLY on the threshold often.  Whatever the float32 roundings of the remaining accumulators
are, the oracle computes the same bits: the kernels are compared with it, not with the grid.

This module (numpy only: it imports nothing that needs a GPU) holds the builders of such layers,
the census that replays a block through the oracle and counts its ties, and the list of cases both
tests/test_threshold_ties_cpu.py (census conditions) and tests/test_threshold_ties_gpu.py (bit
parity of the kernels) walk."""
import functools

import numpy as np

from snnquantprune_amd import synthetic as syn

F32 = np.float32


def _rng(seed):
  return np.random.Generator(np.random.PCG64(seed))


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------


def dyadic_leaf(shape, bits, k, seed, prune_p=0.5, gain=4.0):
  """A reference-style DuQ leaf: a = syn.gaussian_ac(W) (the reference's gaussian_init, as every
  synthetic leaf of this package has it), c = L * 2^-k (exact in float32)."""
  w = syn.kernel(shape, gain, seed)
  L = 2 ** (bits - 1) - 1
  leaf = {"kernel": w,
          "DuQ_0": {"a": np.array([syn.gaussian_ac(w)], F32), "c": np.array([F32(L) * F32(2.0 ** -k)], F32)}}
  if prune_p >= 0:
    leaf["prune_0"] = {"mask": syn.magnitude_mask(w, prune_p)}
  return leaf


def float_leaf(shape, seed, nmax=4, zero_p=0.5, nmin=None):
  """An unquantised leaf (a = -1: DuQ passes the kernel through) whose weights are n * 2^-4 with
  nmin <= n <= nmax (nmin = -nmax unless given): every partial sum over 0/1 inputs is exact in
  float32, in any order."""
  r = _rng(seed)
  n = r.integers(-nmax if nmin is None else nmin, nmax + 1, size=shape)
  n[r.random(shape) < zero_p] = 0
  return {"kernel": (n * F32(2.0 ** -4)).astype(F32),
          "DuQ_0": {"a": np.array([-1], F32), "c": np.array([-1], F32)}}


def dyadic_bn(n, kind, seed=7, t=1.0):
  """A BatchNorm whose folded coefficients (oracle bn_coeffs) are dyadic: var = fl(t - 1e-5) for
  t in {1, 4, 0.25} gives fl(var + eps) == t and mul in {1, 0.5, 2}; means and biases are
  multiples of 2^-3.  kind: "uniform" (one t, zero mean and bias: the uniform-multiplier fold),
  "per_channel" (mixed t, means, biases), "negative" (per_channel with scale -1 on every third
  channel)."""
  if kind is None:
    return None
  r = _rng(seed)
  if kind == "uniform":
    tt = np.full(n, t, F32)
    mean = bias = np.zeros(n, F32)
    scale = np.ones(n, F32)
  else:
    tt = r.choice(np.array([1.0, 4.0, 0.25], F32), size=n).astype(F32)
    mean = (r.integers(-2, 3, n) * F32(0.125)).astype(F32)
    bias = (r.integers(-2, 3, n) * F32(0.125)).astype(F32)
    scale = np.ones(n, F32)
    if kind == "negative":
      scale[::3] = -1
  var = (tt - F32(1e-5)).astype(F32)
  return dict(mean=mean, var=var, scale=scale, bias=bias)


def bn_flags(kind):
  """Names of the fold flags (include/snnqp.h) the host may assert for dyadic_bn(kind)."""
  return ("BN_MEAN_ZERO", "BN_BIAS_ZERO", "BN_MUL_UNIFORM") if kind == "uniform" else ()


def neuron_cfg(form, n=0, v_threshold=None):
  """Oracle neuron configs by epilogue form (conv_tile.h): every constant dyadic.
    mul0   multi_step_LIF tau 2, v_reset 0          u += (x - u) / 2
    plif   parametric_leaky_IF tau_param 0          k = sigmoid(0) = 0.5, the same update
    mul    multi_step_LIF tau 4, v_th 0.75, v_reset 0.25
    div    multi_step_LIF tau 3, v_th 0.75          a true division; x = 2.25 gives 0.75 exactly
    decay  LIF, tau_vec 0 (decay 0.5), every fourth feature 20 (decay 1.0 in float32)
    decay1 LIF, tau_vec 20 everywhere: integrate and fire, the grid never refines"""
  if form == "mul0":
    c = {"kind": "multi_step_LIF", "tau": 2.0, "v_threshold": 1.0, "v_reset": 0.0}
  elif form == "plif":
    c = {"kind": "parametric_leaky_IF", "tau_param": F32(0), "v_threshold": 1.0, "v_reset": 0.0}
  elif form == "mul":
    c = {"kind": "multi_step_LIF", "tau": 4.0, "v_threshold": 0.75, "v_reset": 0.25}
  elif form == "div":
    c = {"kind": "multi_step_LIF", "tau": 3.0, "v_threshold": 0.75, "v_reset": 0.0}
  elif form in ("decay", "decay1"):
    tv = np.zeros(n, F32)
    tv[slice(None) if form == "decay1" else slice(3, None, 4)] = 20
    c = {"kind": "LIF", "tau_vec": tv, "v_threshold": 1.0, "v_reset": 0.0}
  else:
    raise ValueError(form)
  if v_threshold is not None:
    c["v_threshold"] = v_threshold
  return c


def spikes(shape, density, seed):
  return (_rng(seed).random(shape) < density).astype(np.uint8)


def counts(shape, density, seed, top=3):
  """Event counts 0..top (small, so that currents stay on the grid)."""
  r = _rng(seed)
  return ((r.random(shape) < density) * r.integers(1, top + 1, size=shape)).astype(np.uint8)


def dyadic_u0(shape, v_threshold, seed):
  """Carried-in potentials on the 2^-3 grid in [0, v_threshold], about one in eight ON it."""
  r = _rng(seed)
  u = (r.integers(0, int(v_threshold * 8) + 1, size=shape) * F32(0.125)).astype(F32)
  u[r.random(shape) < 0.125] = v_threshold
  return u


def gates(shape, seed):
  return _rng(seed).choice(np.array([0.25, 0.5, 0.75, 1.0], F32), size=shape).astype(F32)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
# Common keys: id, path, T, B, bits, k (c = L 2^-k), density, prune, seed, form (neuron_cfg),
# u0 (bool).  Dense: K, N, rows.  Conv: H, W, cin, cout, bn, pools.  The knobs were tuned on the
# oracle alone until tests/test_threshold_ties_cpu.py's conditions held.
# walk="fast" (dense_wide.hip): a neuron of the form u += (x - u) m with v_reset 0 and no carried-in
# state takes neuron_walk_fast -- but only in a launch that does not return u_T either (the
# launcher's `straight`); the GPU file runs such a case both ways, so its raster is compared on
# the fast walk and raster and u_T on the general one.


def _d(id, path, T, B, K, N, bits, k, density, prune, form="mul0", rows="bits", u0=False, seed=1, **kw):
  return dict(id=id, path=path, T=T, B=B, K=K, N=N, bits=bits, k=k, density=density, prune=prune,
              form=form, rows=rows, u0=u0, seed=seed, **kw)


def _c(id, path, T, B, H, W, cin, cout, bits, k, density, prune, form="mul0", bn=None, u0=False, seed=1,
       pools=(1,), **kw):
  return dict(id=id, path=path, T=T, B=B, H=H, W=W, cin=cin, cout=cout, bits=bits, k=k, density=density,
              prune=prune, form=form, bn=bn, u0=u0, seed=seed, pools=pools, **kw)


CASES = [
    # ---- dense ------------------------------------------------------------------------------
    _d("dense_mfma_8bit_bits", "dense", 6, 5, 256, 70, 8, 5, 0.02, 0.8, kernel="mfma", seed=39),
    _d("dense_mfma_8bit_u8", "dense", 6, 5, 208, 70, 8, 5, 0.02, 0.8, rows="u8", kernel="mfma", seed=34),
    _d("dense_mfma_4bit_no_fp6", "dense", 6, 5, 200, 70, 4, 2, 0.06, 0.5, kernel="mfma", drop_fp6=True, seed=3),
    _d("dense_fp6_4bit", "dense", 6, 5, 200, 70, 4, 2, 0.06, 0.5, kernel="fp6", seed=3),
    _d("dense_fp6_2bit", "dense", 6, 5, 200, 70, 2, 1, 0.2, 0.5, kernel="fp6", seed=4),
    _d("dense_fp6_div", "dense", 6, 5, 200, 70, 4, 2, 0.06, 0.5, form="div", kernel="fp6", seed=5),
    _d("dense_fp6_split_k", "dense", 7, 20, 32768, 200, 4, 6, 0.1, 0.9, kernel="fp6_split", seed=6),
    _d("dense_wide_fast_u8", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, rows="u8", kernel="wide", walk="fast", seed=7),
    _d("dense_wide_fast_bits", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, kernel="wide", walk="fast", seed=7),
    _d("dense_wide_fast_f32", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, rows="f32", kernel="wide", walk="fast", seed=7),
    _d("dense_wide_plif", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, form="plif", kernel="wide", walk="fast", seed=8),
    _d("dense_wide_fast_bn", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, kernel="wide", walk="fast",
       bn="per_channel", seed=18),
    _d("dense_wide_u0", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, rows="u8", u0=True, kernel="wide", seed=9),
    _d("dense_wide_mul", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, form="mul", kernel="wide", seed=10),
    _d("dense_wide_decay", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, rows="u8", form="decay", kernel="wide",
       seed=11),
    _d("dense_wide_div_f32", "dense", 3, 70, 160, 256, 8, 5, 0.04, 0.8, rows="f32", form="div", kernel="wide",
       seed=12),
    _d("dense_generic", "dense", 6, 5, 200, 70, 4, 2, 0.06, 0.5, kernel="generic", seed=3),
    _d("dense_head", "head", 6, 5, 208, 200, 8, 5, 0.04, 0.8, N2=70, bits2=4, k2=2, prune2=0.5, rows="u8", seed=13),
    _d("dense_head_bits", "head", 6, 5, 208, 200, 8, 5, 0.04, 0.8, N2=70, bits2=4, k2=2, prune2=0.5, seed=13),
    _d("dense_gated_4bit", "gated_dense", 2, 33, 64 * 6, 70, 4, 2, 0.05, 0.5, H=2, W=3, C=64, seed=14),
    _d("dense_gated_6bit", "gated_dense", 2, 33, 64 * 6, 70, 6, 2, 0.03, 0.7, H=2, W=3, C=64, seed=15),
    _d("dense_fseq_float", "fseq_dense", 37, 1, 20, 7, 0, 0, 0.3, 0.5, rows="f32", form="decay1", nmax=3, nmin=-1,
       seed=16),
    # ---- conv -------------------------------------------------------------------------------
    _c("bits_c32_o40_table", "conv_bits", 3, 2, 8, 8, 32, 40, 4, 2, 0.03, 0.8, pools=(1, 2), dq="table"),
    _c("bits_c64_o128_uniform_bn", "conv_bits", 3, 2, 5, 11, 64, 128, 4, 1, 0.03, 0.8, bn="uniform", bn_t=4.0,
       dq="table", seed=2),
    _c("bits_c128_o128_arith_bn", "conv_bits", 3, 2, 8, 8, 128, 128, 8, 5, 0.02, 0.9, bn="per_channel",
       pools=(1, 2), dq="arith", seed=3),
    _c("bits_c64_o40_one_negbn", "conv_bits", 3, 2, 8, 8, 64, 40, 2, 1, 0.03, 0.8, bn="negative", pools=(1, 2),
       dq="one", seed=4),
    _c("bits_c128_o40_u0", "conv_bits", 3, 2, 5, 11, 128, 40, 4, 2, 0.015, 0.9, u0=True, dq="table", seed=5),
    _c("bits_c32_o128_div", "conv_bits", 3, 2, 8, 8, 32, 128, 4, 2, 0.03, 0.8, form="div", pools=(1, 2), seed=6),
    _c("bits_c64_o128_decay", "conv_bits", 3, 2, 8, 8, 64, 128, 4, 2, 0.02, 0.8, form="decay", pools=(1, 2),
       seed=7),
    _c("bits_c128_o128_mul", "conv_bits", 3, 2, 8, 8, 128, 128, 4, 2, 0.015, 0.9, form="mul", bn="per_channel",
       pools=(1, 2), seed=8),
    _c("bits_c64_o40_plif", "conv_bits", 3, 2, 5, 11, 64, 40, 4, 2, 0.03, 0.8, form="plif", seed=9),
    _c("bits_knobs_c80_o128", "conv_knobs", 3, 2, 8, 8, 80, 128, 4, 2, 0.03, 0.8, bn="uniform", bn_t=1.0,
       pools=(1, 2), dead=(32, 96), seed=10),
    _c("u8c2_binary", "conv_u8c2", 3, 2, 16, 16, 2, 128, 4, 1, 0.3, 0.3, bn="per_channel", pools=(1, 2),
       frames="binary", seed=11),
    _c("u8c2_counts", "conv_u8c2", 3, 2, 16, 16, 2, 128, 4, 2, 0.3, 0.3, bn="per_channel", pools=(1, 2),
       frames="counts", seed=12),
    _c("u8c2_counts_div", "conv_u8c2", 3, 2, 16, 16, 2, 128, 4, 2, 0.3, 0.3, form="div", pools=(1, 2),
       frames="counts", seed=17),
    _c("gated_conv_4bit", "gated_conv", 2, 3, 5, 11, 64, 70, 4, 2, 0.03, 0.8, bn="per_channel", seed=13),
    _c("gated_conv_6bit", "gated_conv", 2, 3, 5, 11, 64, 70, 6, 4, 0.03, 0.8, bn="per_channel", seed=14),
    _c("generic_strided_2d", "conv_generic", 3, 2, 9, 11, 16, 40, 4, 2, 0.08, 0.5, bn="per_channel",
       ksize=(3, 3), strides=(2, 2), padding=((1, 1), (0, 2)), seed=15),
    _c("generic_3d", "conv3d", 3, 2, 6, 7, 4, 40, 4, 2, 0.15, 0.5, bn="per_channel", D=5, ksize=(3, 3, 3),
       strides=(2, 1, 2), padding="SAME", form="decay", seed=16),
]
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def case(id):
  return CASES[CASE_IDS.index(id)]


@functools.lru_cache(maxsize=None)
def build(id):
  """The arrays of a case (read-only by convention: they are shared between the tests):
  leaf / leaf2, x, gate, bn, u0, cfg / cfg2."""
  c = case(id)
  s = 1000 * c["seed"]
  T, B = c["T"], c["B"]
  out = {"case": c}
  path = c["path"]
  if path in ("dense", "head", "gated_dense", "fseq_dense"):
    K, N = c["K"], c["N"]
    if path == "fseq_dense":
      out["leaf"] = float_leaf((K, N), s + 1, c.get("nmax", 4), c["prune"], c.get("nmin"))
    else:
      out["leaf"] = dyadic_leaf((K, N), c["bits"], c["k"], s + 1, c["prune"])
    if path == "gated_dense":
      out["x"] = spikes((T, B, c["H"], c["W"], c["C"]), c["density"], s + 2)
      out["gate"] = gates((T, B, c["C"]), s + 3)
    elif c["rows"] == "u8" and path == "dense" and c.get("kernel") == "wide":
      out["x"] = counts((T, B, K), c["density"], s + 2)        # uint8 rows: small counts too
    else:
      out["x"] = spikes((T, B, K), c["density"], s + 2)
    out["cfg"] = neuron_cfg(c["form"], N, c.get("v_threshold"))
    out["bn"] = dyadic_bn(N, c.get("bn"), s + 6, c.get("bn_t", 1.0))
    out["u0"] = dyadic_u0((B, N), out["cfg"]["v_threshold"], s + 4) if c["u0"] else None
    if path == "head":
      out["leaf2"] = dyadic_leaf((N, c["N2"]), c["bits2"], c["k2"], s + 5, c["prune2"])
      out["cfg2"] = neuron_cfg("mul0", c["N2"])
    return out
  cin, cout = c["cin"], c["cout"]
  ks = c.get("ksize", (3, 3))
  out["leaf"] = dyadic_leaf(tuple(ks) + (cin, cout), c["bits"], c["k"], s + 1, c["prune"])
  if "dead" in c:                       # output channels pruned away whole: they can never fire
    out["leaf"]["prune_0"]["mask"][..., c["dead"][0]:c["dead"][1]] = 0
  sp = ((c["D"],) if path == "conv3d" else ()) + (c["H"], c["W"])
  if c.get("frames") == "counts":
    out["x"] = counts((T, B) + sp + (cin,), c["density"], s + 2)
  else:
    out["x"] = spikes((T, B) + sp + (cin,), c["density"], s + 2)
  if path == "gated_conv":
    out["gate"] = gates((T, B, cin), s + 3)
  out["bn"] = dyadic_bn(cout, c["bn"], s + 6, c.get("bn_t", 1.0))
  out["cfg"] = neuron_cfg(c["form"], cout, c.get("v_threshold"))
  out["strides"] = c.get("strides")
  out["padding"] = c.get("padding", ((1, 1), (1, 1)))
  out["u0"] = None
  if c["u0"]:
    import oracle.snn_oracle as o
    pads = o.resolve_padding(sp, ks, c.get("strides") or (1,) * len(sp), out["padding"])
    osp = o.conv_out_spatial(sp, ks, c.get("strides") or (1,) * len(sp), pads)
    out["u0"] = dyadic_u0((B,) + tuple(osp) + (cout,), out["cfg"]["v_threshold"], s + 4)
  return out


# ---------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------


def qweight(o, leaf, bits):
  a = float(leaf["DuQ_0"]["a"][0])
  quant = None
  if a != -1.0:
    quant = {"kind": "duq", "bits": bits, "a": a, "c": float(leaf["DuQ_0"]["c"][0])}
  return o.QWeight(leaf["kernel"], quant, leaf.get("prune_0", {}).get("mask"))


def _replay(o, currents, cfg, u0, strict):
  """The oracle's own neuron over currents [T, ...], with its `heaviside` watched (and, for
  strict, replaced by x > 0): (u_T, raster, mask of the steps whose pre-reset u - v_th == 0)."""
  ties = []
  orig = o.heaviside

  def watched(x):
    x = np.asarray(x, dtype=F32)
    ties.append(x == F32(0))
    return ((x > F32(0)) if strict else (x >= F32(0))).astype(F32)
  o.heaviside = watched
  try:
    neuron = o._neuron(cfg)
    u = np.zeros_like(currents[0], dtype=F32) if u0 is None else np.asarray(u0, F32)
    out = []
    for t in range(currents.shape[0]):
      u, s = neuron(u, currents[t])
      out.append(s)
  finally:
    o.heaviside = orig
  return u, np.stack(out), np.stack(ties)


def census_of_currents(o, currents, cfg, u0=None, pooled=False):
  u, s, tie = _replay(o, currents, cfg, u0, False)
  _, s_strict, _ = _replay(o, currents, cfg, u0, True)
  out = {"u": u, "s": s.astype(np.uint8), "ties": int(tie.sum()),
         "strict_flips": int((s != s_strict).sum()), "steps": int(s.size), "rate": float(s.mean()),
         "tie_only_windows": 0}
  if pooled:
    T, B, H, W, C = s.shape
    win = lambda a: a[:, :, :H // 2 * 2, :W // 2 * 2].reshape(T, B, H // 2, 2, W // 2, 2, C)
    fired = win(s).sum(axis=(3, 5))                       # spikes per 2x2 window
    tied = win(tie & (s != 0)).sum(axis=(3, 5))
    out["tie_only_windows"] = int(((fired == 1) & (tied == 1)).sum())
    out["pooled"] = o.max_pool_2x2(s).astype(np.uint8)
  return out


def block_currents(o, b, leaf_key="leaf", x=None):
  """Currents [T, ...] of a built case through the oracle's own contraction and BatchNorm."""
  c = b["case"]
  qw = qweight(o, b[leaf_key], c["bits2" if leaf_key == "leaf2" else "bits"])
  x = b["x"] if x is None else x
  path = c["path"]
  T = x.shape[0]
  if path in ("dense", "head"):
    y = [o.quant_dense(x[t], qw, "int") for t in range(T)]
  elif path == "fseq_dense":
    y = [o.quant_dense(x[t].astype(F32), qw, "fseq") for t in range(T)]
  elif path == "gated_dense":
    y = [o.gated_dense(x[t], b["gate"][t], qw) for t in range(T)]
  elif path == "gated_conv":
    y = [o.gated_conv(x[t], b["gate"][t], qw) for t in range(T)]
  else:
    y = [o.quant_conv(x[t], qw, strides=b["strides"], padding=b["padding"], mode="int") for t in range(T)]
  bn = b.get("bn")
  if bn is not None:
    y = [o.batchnorm_eval(v, bn["mean"], bn["var"], bn["scale"], bn["bias"], 1e-5) for v in y]
  return np.stack(y).astype(F32)


@functools.lru_cache(maxsize=None)
def _census(id):
  import oracle.snn_oracle as o
  b = build(id)
  c = b["case"]
  pooled = 2 in c.get("pools", ())
  out = census_of_currents(o, block_currents(o, b), b["cfg"], b["u0"], pooled)
  if c["path"] == "head":
    out2 = census_of_currents(o, block_currents(o, b, "leaf2", out["s"]), b["cfg2"])
    out["second"] = out2
    out["logits"] = o.vote(out2["s"].astype(F32), 10)
  return out


def tie_census(o, id):
  """Replays case `id` step by step with the oracle's quant_dense / quant_conv / gated_*,
  batchnorm_eval and neuron functions.  Returns a dict: `u` (u_T), `s` (raster, uint8), `ties`
  (neuron-steps whose pre-reset u - v_th == 0), `strict_flips` (raster bits that differ when
  heaviside is x > 0 for the whole replay), `tie_only_windows` (ties that fired alone in their
  2x2 pool window; pooled cases, with `pooled`), `steps`, `rate`; a head adds `second` (the
  census of its second block on the first one's raster) and `logits`.  Computed once per case
  and shared: callers leave the arrays unchanged."""
  import oracle.snn_oracle as mod
  assert o is mod, "the census replays the live oracle"
  return _census(id)
