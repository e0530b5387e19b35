"""Cases of the currents form of the bit-input MFMA conv (csrc/conv3x3_currents.hip): the 3x3 /
stride 1 / pad 1 connection alone over a spike raster.  Seeded inputs and the oracle's expected
accumulators and currents; tests/test_conv_currents_cpu.py checks the cases themselves,
tests/test_conv_currents_gpu.py the kernel against them.  No GPU here.

Kernels are oracle.synth_kernel, quantised by DuQ with a = c = gaussian_init's 3 sigma bound
(`a_sigma` other than 3: that many standard deviations, so that more codes saturate):
  q4p90  4-bit, 90 % pruned   codes of magnitude <= 7: the f8f6f4 instruction
  q4     4-bit, unpruned
  q2     2-bit                L == 1
  q8p30  8-bit, 30 % pruned   the int8 instruction

Rasters:
  bern     seeded Bernoulli(0.5), zero bits beyond Cin in a pixel's last word (packing does that)
  ones     every spike set
  zeros    none set
  aligned  bern, but around the centre pixel of image 0 the 3x3xCin window is (code of channel 0 >
           0): that output is the sum of channel 0's positive codes, the largest accumulator any
           raster can give it.  A kernel of mean zero cancels on an all-ones raster (|acc| is some
           sqrt(9 Cin) codes there), so it is these cases -- with a = 0.75 sigma, i.e. most codes
           saturated -- that carry an fp6 accumulator past 2047 (the bound of the fused kernel's
           dequantisation table) and an int8 one past 32767 (16 bits).
"""
import numpy as np

from oracle import snn_oracle as oracle
from snnquantprune_amd import synthetic as syn

F32 = np.float32
QUANTS = {"q4p90": (4, 0.9), "q4": (4, -1.0), "q2": (2, -1.0), "q8p30": (8, 0.3)}
PADS = ((1, 1), (1, 1))


def _case(quant, cin, cout, H, W, NB, raster="bern", a_sigma=3.0, wt_cin=0):
  return dict(quant=quant, cin=cin, cout=cout, H=H, W=W, NB=NB, raster=raster, a_sigma=a_sigma,
              wt_cin=wt_cin)


# Every Cin, Cout, H x W and NB of the grid once per instruction.  Small axes are not combined
# with each other (one input channel into one output channel on one pixel is one number), and the
# 90 % pruned kernel is not given a single input channel (most channels would keep no code).
_GEOMS = [(16, 31, 3, 5, 3), (17, 32, 4, 8, 1), (32, 33, 5, 9, 3), (33, 128, 13, 17, 1),
          (48, 129, 3, 5, 1), (64, 160, 4, 8, 3), (79, 33, 5, 9, 1), (96, 1, 13, 17, 3),
          (100, 32, 1, 1, 3), (128, 129, 5, 9, 1)]
GRID = ([_case("q4", 1, 160, 13, 17, 1)] + [_case("q4p90", *g) for g in _GEOMS] +
        [_case("q8p30", 1, 160, 13, 17, 1)] + [_case("q8p30", *g) for g in _GEOMS] +
        [_case("q4", 128, 128, 4, 8, 1), _case("q4", 79, 33, 3, 5, 3), _case("q4", 33, 160, 5, 9, 1),
         _case("q2", 64, 129, 5, 9, 1), _case("q2", 100, 31, 13, 17, 1), _case("q2", 17, 32, 4, 8, 3),
         _case("q2", 128, 128, 1, 1, 1)])
FURTHER = [
    _case("q4p90", 32, 32, 16, 32, 40),                    # 640 patches: a second patch per workgroup, the XCD split
    _case("q4", 128, 64, 5, 9, 1, raster="ones"),
    _case("q8p30", 128, 64, 5, 9, 1, raster="ones"),
    _case("q4", 128, 33, 5, 9, 1, raster="aligned", a_sigma=0.75),
    _case("q8p30", 128, 33, 5, 9, 1, raster="aligned", a_sigma=0.75),
    _case("q4p90", 64, 40, 3, 5, 1, raster="zeros"),
    _case("q4p90", 40, 33, 5, 9, 3, wt_cin=128),            # codes padded wider than needed
    _case("q8p30", 40, 33, 5, 9, 3, wt_cin=128),
]
CASES = GRID + FURTHER


def case_id(c):
  s = "%s-c%d-o%d-%dx%d-n%d" % (c["quant"], c["cin"], c["cout"], c["H"], c["W"], c["NB"])
  if c["raster"] != "bern":
    s += "-" + c["raster"]
  if c["wt_cin"]:
    s += "-wt%d" % c["wt_cin"]
  return s


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def _seed(c):
  return 7100 + CASES.index(c) if c in CASES else 7099


def bits_of(c):
  return QUANTS[c["quant"]][0]


def leaf_of(c, seed=None):
  """The layer's parameter leaf in the reference's naming: kernel, DuQ's a and c, the prune mask."""
  bits, p = QUANTS[c["quant"]]
  seed = _seed(c) if seed is None else seed
  w = oracle.synth_kernel((3, 3, c["cin"], c["cout"]), 1.0, seed)
  ac = syn.gaussian_ac(w) if c["a_sigma"] == 3.0 else F32(c["a_sigma"] * np.std(w, dtype=F32))
  leaf = {"kernel": w, "DuQ_0": {"a": np.array([ac], F32), "c": np.array([ac], F32)}}
  if p >= 0:
    leaf["prune_0"] = {"mask": syn.magnitude_mask(w, p)}
  return leaf


def qweight_of(leaf, bits):
  quant = {"kind": "duq", "bits": bits, "a": float(leaf["DuQ_0"]["a"][0]), "c": float(leaf["DuQ_0"]["c"][0])}
  return oracle.QWeight(leaf["kernel"], quant, leaf.get("prune_0", {}).get("mask"))


def raster_of(c, qw, seed=None):
  """uint8 0/1 [NB, H, W, Cin]."""
  seed = _seed(c) if seed is None else seed
  shape = (c["NB"], c["H"], c["W"], c["cin"])
  if c["raster"] == "ones":
    return np.ones(shape, np.uint8)
  if c["raster"] == "zeros":
    return np.zeros(shape, np.uint8)
  rng = np.random.Generator(np.random.PCG64(seed + 50000))
  x = (rng.random(shape) < 0.5).astype(np.uint8)
  if c["raster"] == "aligned":
    cy, cx = c["H"] // 2, c["W"] // 2
    assert 1 <= cy < c["H"] - 1 and 1 <= cx < c["W"] - 1
    x[0, cy - 1:cy + 2, cx - 1:cx + 2, :] = (qw.q[:, :, :, 0] > 0)
  return x


_expected = {}


def expected(c):
  """{"leaf", "qw", "x", "acc" int32, "y" float32 [NB, H, W, Cout]} by the oracle; computed once per
  case and shared (nothing modifies it)."""
  key = case_id(c)
  if key not in _expected:
    leaf = leaf_of(c)
    qw = qweight_of(leaf, bits_of(c))
    x = raster_of(c, qw)
    acc = oracle.quant_conv(x, qw, None, PADS, mode="int", return_acc=True)
    y = qw.dequant_acc(acc)
    assert np.abs(acc).max(initial=0) < 2 ** 24
    _expected[key] = dict(leaf=leaf, qw=qw, x=x, acc=acc.astype(np.int32), y=y)
  return _expected[key]


def fp6(c):
  """Whether the case's codes fit the f8f6f4 instruction (magnitude <= 7)."""
  return bits_of(c) <= 4
