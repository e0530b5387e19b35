"""The cases of the tests of training with rematerialised blocks:
tests/test_remat_cpu.py checks the conditions on them without a GPU, tests/test_remat_kernels_gpu.py
and tests/test_remat_gpu.py run them.

Fused-scan cases: T = 6; multi_step_LIF on the inv_k path (tau 2) and the division path (tau 3),
v_reset in {0, 0.1}; n = R C elements in {1, 255, 256, 257, 513} around the 256-lane workgroup and
C in {1, 15, 16, 17, 65} for the broadcast of the per-channel coefficients.  mean, var, scale and
bias are drawn, not computed from the currents: the kernel takes them as given.  Every case fires
in the 2-30 % band (the one-element case: one spike in six steps, for which its seed is searched).

Pool cases: h around the threshold with planted h == vth ties, windows all below, all above and
all equal, odd H and W and a 1 x 1 image.
"""
import functools

import numpy as np

from tests import remat_reference as rr
from tests.train_helpers import mixed

F32, F64 = np.float32, np.float64
T, VTH, EPS = 6, 1.0, 1e-5
TAUS = {"msl2": 2.0, "msl3": 3.0}
VRS = (0.0, 0.1)
SHAPES = [(1, 1), (17, 15), (16, 16), (257, 1), (27, 19), (3, 17), (5, 65)]   # n = 1, 255, 256, 257, 513, 51, 325
SPLITS = (1, 2, 4, 6, 7)        # steps per chunk: W = 4 leaves a ragged last chunk, 7 > T is one chunk
MODEL_T = 6
MODEL_W = SPLITS


def scan_cases():
  return [("%s-%dx%d-vr%g" % (k, R, C, vr), k, R, C, vr) for k in TAUS for (R, C) in SHAPES for vr in VRS]


# mean and spread of the normalised currents, per neuron: chosen once for the 2-30 % band
NORMALISED = {"msl2": (0.45, 0.6), "msl3": (0.6, 0.8)}


def _draw(seed, R, C, y_mean, y_std):
  rng = np.random.default_rng(seed)
  cur = (3.0 * rng.standard_normal((T, R, C)) + 1.0).astype(F32)
  mean = (1.0 + 0.3 * rng.standard_normal((T, C))).astype(F32)
  var = (9.0 * rng.uniform(0.6, 1.5, (T, C))).astype(F32)
  scale = (y_std + 0.1 * rng.standard_normal(C)).astype(F32)
  bias = (y_mean + 0.1 * rng.standard_normal(C)).astype(F32)
  return rng, cur, mean, var, scale, bias


@functools.lru_cache(maxsize=None)
def scan_case(kname, R, C, vr):
  """dict(tau, vth, vr, cur [T, R, C], mean, var, mul [T, C], scale, bias [C], gs, and the whole run
  from zeros: h, s, u_T, and starts [T + 1, R, C], the membrane before every step and after the
  last).  Nothing modifies it."""
  tau = TAUS[kname]
  seed = R * 1009 + C * 7 + int(vr * 10) + 31 * sorted(TAUS).index(kname)
  while True:
    rng, cur, mean, var, scale, bias = _draw(seed, R, C, *NORMALISED[kname])
    mul = rr.bn_multiplier(var, scale, EPS)
    h, s, u_T = rr.fused_ref(cur, mean, mul, bias, tau, VTH, vr)
    if 0.03 <= s.mean(dtype=F64) <= 0.28:            # (inside the band the CPU test holds)
      break
    seed += 100003                              # (the one-element case: until one spike in six steps)
  starts = np.concatenate([np.zeros((1, R, C), F32),
                           np.where((h - F32(VTH)) >= 0, F32(vr), h).astype(F32)])
  c = dict(tau=tau, vth=VTH, vr=vr, cur=cur, mean=mean, var=var, mul=mul, scale=scale, bias=bias,
           gs=mixed(rng, (T, R, C)), h=h, s=s, u_T=u_T, starts=starts)
  for v in c.values():
    if isinstance(v, np.ndarray):
      v.setflags(write=False)
  return c


def pool_cases():
  return [("%dx%dx%dx%d" % s, s) for s in ((2, 5, 7, 3), (1, 1, 1, 4), (3, 4, 6, 17), (1, 8, 8, 65), (2, 3, 2, 1))]


@functools.lru_cache(maxsize=None)
def pool_case(shape):
  """dict(h [NB, H, W, C], vth, gp [NB, H/2, W/2, C]): h within one of the threshold, one element in
  eight exactly on it; window 0 of every image all below, window 1 all above, window 2 all equal to
  the threshold."""
  NB, H, W, C = shape
  rng = np.random.default_rng(NB * 1000 + H * 100 + W * 10 + C)
  h = (VTH + rng.uniform(-1.0, 1.0, shape)).astype(F32)
  h[rng.random(shape) < 0.125] = F32(VTH)                      # ties: (h - vth) >= 0 fires
  if H >= 2 and W >= 2:
    h[:, 0:2, 0:2] = F32(VTH - 0.5)
  if H >= 2 and W >= 4:
    h[:, 0:2, 2:4] = F32(VTH + 0.5)
  if H >= 2 and W >= 6:
    h[:, 0:2, 4:6] = F32(VTH)
  gp = mixed(rng, (NB, H // 2, W // 2, C))
  h.setflags(write=False)
  gp.setflags(write=False)
  return dict(h=h, vth=VTH, gp=gp)


# ---- the models -------------------------------------------------------------------------------------

def conv_setup(dev, quantized=True, dtype="uint8", neuron="msl", dropout=None, remat=None, B=None):
  """The two-block ConvDenseSNN of tests/conv_train_reference.py (8x8x2 frames, 16 channels; 4-bit /
  90 % pruned or unquantised) at T = 6, with config.remat = `remat` (None: without the key), and
  multi_step_LIF or, under config.learn_neuron_params, PLIF."""
  import torch
  from functools import partial
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, spiking_learning as sl, synthetic as syn
  from tests import conv_train_reference as cr
  v, x = cr.fixture(quantized, dtype, T=MODEL_T, **({} if B is None else dict(B=B)))
  extra = dict(learn_neuron_params=True) if neuron == "plif" else {}
  if remat is not None:
    extra["remat"] = remat
  cfg = syn.make_config(bits=cr.BITS, prune_percentage=0.9 if quantized else -1.0, channels=cr.CHANNELS,
                        tau=cr.TAU, quantized=quantized, num_conv_blocks=cr.NBLOCKS,
                        dropout=cr.KEEP if dropout is None else dropout, **extra)
  if neuron == "plif":
    rng = np.random.default_rng(17)
    for i in range(cr.NBLOCKS + 1):
      v["params"]["parametric_leaky_IF_%d" % i] = {"tau": rng.uniform(-0.5, 0.8, 1).astype(F32)}
    cfg.neuron_dynamics = partial(sl.parametric_leaky_IF, init_tau=2.0, spike_fn=sl.atan)
  model = models.ConvDenseSNN(num_classes=cr.CLASSES, config=cfg)
  return model, v, nn.tree_from_numpy(v, dev), torch.from_numpy(x).to(dev)
