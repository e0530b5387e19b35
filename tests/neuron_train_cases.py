"""The cases of the PLIF / LIF training-kernel tests (tests/test_neuron_train_cpu.py checks the
conditions on them without a GPU, tests/test_neuron_train_gpu.py runs them).

Shapes (T, R, C): one element; C below, at and beside a half wave (30, 33); more rows than a
default range and C one past a wave (70, 65); more than one workgroup per range and C over two
waves (257, 130).  For each, v_reset in {0, 0.1}; PLIF with m in {0.5, sigmoid(0.3)}; LIF with
decays that include 0.5 and one within 2^-10 of 1.  Potentials come from
train_reference.planted_h (the surrogates' edges), currents and upstream gradients are random.

`splits` in {1, 2, 3, R, default}, those the interface takes (1..max(R, 1)): the others are its
refusals, which the tests check as refusals.
"""
import numpy as np

from oracle import snn_oracle as oracle
from tests import train_reference as tr
from tests.train_helpers import mixed

F32 = np.float32
VTH = 1.0
SHAPES = [(1, 1, 1), (7, 5, 30), (4, 3, 33), (3, 70, 65), (2, 257, 130)]
VRS = (0.0, 0.1)
PLIF_TAUS = (0.0, 0.3)                 # m = sigmoid: 0.5 and 0.5744...
NON_SLAYER = ("fast_sigmoid", "atan", "smooth_step", "piecewise_linear")
SHIFT = 0.0                            # of planted_h: half the potentials on either side of vth


def splits_of(R, default):
  return sorted({s for s in (1, 2, 3, R, default) if 1 <= s <= max(R, 1)})


def lif_taus(rng, C, vr):
  """Raw LIF parameters [C]: sigmoid(0) = 0.5 and sigmoid(8) = 1 - 3.4e-4 among them (C == 1: one
  of the two, by v_reset)."""
  tau = rng.uniform(-2.0, 3.0, C).astype(F32)
  if C == 1:
    tau[0] = 0.0 if vr == 0.0 else 8.0
  else:
    tau[0], tau[1] = 0.0, 8.0
  return tau


def potentials(rng, shape, vr):
  """planted_h; a single element takes the threshold itself (a spike) or 0.25 below it."""
  if int(np.prod(shape)) == 1:
    return np.full(shape, VTH if vr == 0.0 else VTH - 0.25, F32)
  return tr.planted_h(rng, shape, VTH, shift=SHIFT)[0]


def case(kind, shape, vr, which=0):
  """dict(h, x, gs, vth, vr, tau (raw parameter), par (float32 m or decays [C])).  which: the
  index into PLIF_TAUS (PLIF)."""
  T, R, C = shape
  rng = np.random.default_rng(T * 100003 + R * 1009 + C * 7 + int(vr * 10) + 31 * which + (kind == "lif") * 5)
  h = potentials(rng, shape, vr)
  x = (0.5 + rng.standard_normal(shape)).astype(F32)
  gs = mixed(rng, shape)
  if kind == "plif":
    tau = np.array([PLIF_TAUS[which]], F32)
    par = oracle.sigmoid_f32(tau[0])
  else:
    tau = lif_taus(rng, C, vr)
    par = oracle.sigmoid_f32(tau)
  return dict(kind=kind, shape=shape, h=h, x=x, gs=gs, vth=VTH, vr=vr, tau=tau, par=par)


def all_cases():
  """(id, kind, shape, vr, which) of every case."""
  out = []
  for shape in SHAPES:
    tag = "x".join(map(str, shape))
    for vr in VRS:
      for which in range(len(PLIF_TAUS)):
        out.append(("plif-%s-vr%g-m%d" % (tag, vr, which), "plif", shape, vr, which))
      out.append(("lif-%s-vr%g" % (tag, vr), "lif", shape, vr, 0))
  return out
