"""The selection rule of a prune event as a NumPy reference, and the cases the CPU
path (ops.magnitude_prune on CPU tensors) and the kernel (csrc/prune.hip) are compared on: the
smallest shapes at which the kernel can go wrong.  Nothing here needs a GPU.

The kernel cuts the index into contiguous ranges of a multiple of 256 entries, one workgroup each,
at least 4096 entries in all but the last: n = 4099 is two ranges, of 2304 and 1795 entries."""
import numpy as np

F32, U32 = np.float32, np.uint32
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 4099)
LAYERS = (7, 300, 1153)            # the three "layers" of the global path
EDGE = 2304                        # first index of the second workgroup's range at n = 4099


def keys(w):
  """bits(|w|) as uint32: -0 = +0, denormals in order, Inf above every finite value, NaN above Inf."""
  return np.ascontiguousarray(w, F32).reshape(-1).view(U32) & U32(0x7FFFFFFF)


def unpruned(mask):
  return (np.ascontiguousarray(mask, F32).reshape(-1).view(U32) & U32(0x7FFFFFFF)) != 0


def reference_prune(w, mask, k):
  """The mask after a prune event with target k: a copy of `mask` (float32, its shape) in which the
  first max(k - m, 0) entries of the stable order on (mask != 0, key, index) past the m pruned ones
  are +0.0.  Nothing else is touched."""
  mask = np.array(mask, F32)
  flat = mask.reshape(-1)
  live = unpruned(flat)
  m = int(flat.size - live.sum())
  assert 0 <= k <= flat.size
  if k > m:
    order = np.lexsort((np.arange(flat.size), keys(w), live))      # last key first: pruned, then by key, then index
    flat[order[m:k]] = 0.0
  return mask


def _bits(u):
  return np.asarray(u, U32).view(F32)


def _rng(seed):
  return np.random.Generator(np.random.PCG64(seed))


def _mask(rng, n, kind):
  if kind == "none":
    return np.ones(n, F32)
  if kind == "all":
    return np.zeros(n, F32)
  m = (rng.random(n) < 0.7).astype(F32)
  if kind == "drift":              # values weight decay lets drift from 1.0; a -0.0 counts as pruned
    m = np.where(m != 0, F32(0.97) + (rng.random(n) * F32(0.02)).astype(F32), m).astype(F32)
    m[rng.integers(0, n)] = F32(-0.0)
    if n > 2:
      m[rng.integers(0, n)] = F32(-1.25)
  return m


def _ks(n, m):
  return sorted({k for k in (0, 1, m, m + 1, n - 1, n, (n + m) // 2) if 0 <= k <= n})


def cases():
  """[(name, w float32 [n], mask float32 [n], k)]"""
  out = []

  def add(name, w, mask, ks=None):
    w, mask = np.ascontiguousarray(w, F32), np.ascontiguousarray(mask, F32)
    m = int((~unpruned(mask)).sum())
    for k in (_ks(w.size, m) if ks is None else ks):
      out.append(("%s-n%d-m%d-k%d" % (name, w.size, m, k), w, mask, int(k)))

  # every edge size, every k of the list, masks with m = 0 / some / n
  for n in SIZES:
    rng = _rng(n)
    w = rng.standard_normal(n).astype(F32)
    add("normal", w, _mask(rng, n, "none"))
    add("normal-some", w, _mask(rng, n, "some"))
  for n in (1, 65, 257):
    add("normal-all", _rng(n).standard_normal(n).astype(F32), _mask(None, n, "all"))
  # all magnitudes equal: one bucket in every radix pass, the cut decided by index alone
  for n in (64, 65, 257, 4099):
    rng = _rng(100 + n)
    w = np.where(rng.random(n) < 0.5, F32(0.375), F32(-0.375)).astype(F32)
    add("equal", w, _mask(rng, n, "none"))
    add("equal-some", w, _mask(rng, n, "some"))
  # keys that differ in the low 10 bits only / in the top 11 bits only
  for n in (257, 4099):
    rng = _rng(200 + n)
    sign = (rng.integers(0, 2, n).astype(U32) << U32(31))
    add("low10", _bits(U32(0x3F800000) | rng.integers(0, 1024, n).astype(U32) | sign), _mask(rng, n, "some"))
    add("top11", _bits((rng.integers(1, 1020, n).astype(U32) << U32(21)) | sign), _mask(rng, n, "some"))
    add("mid11", _bits(U32(0x3F800000) | (rng.integers(0, 4, n).astype(U32) << U32(10)) | sign), _mask(rng, n, "none"))
  # +-0 together with denormals
  for n in (65, 1025):
    rng = _rng(300 + n)
    u = rng.integers(0, 6, n).astype(U32)                          # 0 and the five smallest denormals
    add("zeros-denormals", _bits(u | (rng.integers(0, 2, n).astype(U32) << U32(31))), _mask(rng, n, "some"))
  # equal magnitudes of opposite sign straddling a workgroup's edge, exactly at the cut
  n = 4099
  rng = _rng(400)
  w = (rng.random(n).astype(F32) + F32(1.0))                       # everything else is larger than the pair's value
  small = rng.choice(np.setdiff1d(np.arange(n), np.arange(EDGE - 2, EDGE + 2)), 40, replace=False)
  w[small] = F32(0.01)
  w[EDGE - 2], w[EDGE - 1], w[EDGE], w[EDGE + 1] = F32(0.5), F32(-0.5), F32(0.5), F32(-0.5)
  add("straddle", w, np.ones(n, F32), ks=[40, 41, 42, 43, 44, 45])
  mask = np.ones(n, F32)
  mask[[3, EDGE - 1, n - 1]] = 0.0                                  # one of the four is already pruned
  add("straddle-some", w, mask, ks=[43, 44, 45, 46])
  # an Inf and a NaN present (either sign, a payload)
  for n in (65, 1025):
    rng = _rng(500 + n)
    w = rng.standard_normal(n).astype(F32)
    w[[1, n // 2]] = [np.inf, -np.inf]
    w.view(U32)[[0, n - 1, n // 3]] = [0x7FC00001, 0xFFC12345, 0x7F800001]
    add("nonfinite", w, _mask(rng, n, "some"), ks=[0, n - 6, n - 5, n - 4, n - 3, n - 2, n - 1, n])
  # mask values other than 0 / 1: they come back untouched
  for n in (63, 256, 4099):
    rng = _rng(600 + n)
    add("drift", rng.standard_normal(n).astype(F32), _mask(rng, n, "drift"))
  # three layers of odd sizes, concatenated
  w, mask = layer_tensors()
  add("layers", np.concatenate([a.reshape(-1) for a in w]), np.concatenate([a.reshape(-1) for a in mask]))
  return out


def layer_tensors():
  """([kernel], [mask]) of three layers with LAYERS entries, shaped: layer 1 holds values of the
  scale of layer 0 / 10, so that a global cut and the per-layer cuts differ; ties inside and across
  layers; some entries pruned already."""
  rng = _rng(700)
  shapes = ((7,), (3, 10, 10), (1153, 1))
  w, mask = [], []
  for i, (n, shape) in enumerate(zip(LAYERS, shapes)):
    a = (rng.standard_normal(n) * (0.1 if i == 1 else 1.0)).astype(F32)
    a[rng.integers(0, n, max(1, n // 10))] = F32(0.0625) * (1 if i else -1)     # ties, also across layers
    w.append(a.reshape(shape))
    mask.append((rng.random(n) < 0.85).astype(F32).reshape(shape))
  return w, mask


def as_i32(a):
  """The bits, for comparisons that count NaN payloads, the sign of a zero and untouched values."""
  return np.ascontiguousarray(a, F32).reshape(-1).view(np.int32)
