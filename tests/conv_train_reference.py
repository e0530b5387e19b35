"""Plain references for the conv training kernels (csrc/train_conv.hip); no GPU.

  wgrad_matrices / igrad_matrices   the explicitly gathered operands A [Rn, I], B [Rn, J] of the two
                                    conv gradient products (a tap outside the image is 0.0), to be
                                    fed to train_reference.gemm_chain / gemm_f64 / gemm_mag
  split_ranges / split_sum_ref      the split of r and the sequential float32 sum of the ranges' chains
  pool_vjp_first_max                the 2x2 max pool's gradient routing (first maximum, row-major)
  bn_batch_stats64 / bn_train64     batch-statistics BatchNorm in float64 (flax 0.4.0 form)
  geometry                          explicit pads / output size of the nine reference geometries
"""
import numpy as np

from oracle import snn_oracle as oracle
from tests import train_reference as tr

F32 = np.float32
F64 = np.float64


def geometry(H, W, ks, strides, padding):
  """-> (pads ((pt, pb), (pl, pr)), (OH, OW)) by the oracle's lax rules."""
  pads = oracle.resolve_padding((H, W), ks, strides, padding)
  return pads, oracle.conv_out_spatial((H, W), ks, strides, pads)


def wgrad_matrices(x, gI, ks, strides, pads):
  """x [NB, H, W, Cin], gI [NB, OH, OW, Cout] -> A [Rn, KH KW Cin], B [Rn, Cout], r = (n, oh, ow):
  gw = A^T B.  im2col reads the zero padding as literal zeros."""
  x, gI = np.asarray(x), np.asarray(gI)
  cols = oracle.im2col(x, ks, strides, pads)
  assert cols.shape[:3] == gI.shape[:3], (cols.shape, gI.shape)
  return cols.reshape(-1, cols.shape[-1]), gI.reshape(-1, gI.shape[-1])


def igrad_matrices(gI, w, H, W, strides, pads):
  """gI [NB, OH, OW, Cout], w HWIO -> A [KH KW Cout, NB H W], B [KH KW Cout, Cin], r = (kh, kw, co):
  gx = A^T B.  A(r, m) = gI[n, (ih + pt - kh) / sh, (iw + pl - kw) / sw, co] where both quotients
  are integers in range, else 0.0."""
  gI, w = np.asarray(gI), np.asarray(w)
  NB, OH, OW, Cout = gI.shape
  KH, KW, Cin, _ = w.shape
  (sh, sw), (pt, pl) = strides, (pads[0][0], pads[1][0])
  A = np.zeros((KH, KW, Cout, NB, H, W), gI.dtype)
  ih, iw = np.arange(H), np.arange(W)
  for kh in range(KH):
    th = ih + pt - kh
    okh = (th >= 0) & (th % sh == 0) & (th // sh < OH)
    for kw in range(KW):
      tw = iw + pl - kw
      okw = (tw >= 0) & (tw % sw == 0) & (tw // sw < OW)
      if not okh.any() or not okw.any():
        continue
      src = gI[:, (th // sh)[okh]][:, :, (tw // sw)[okw]]          # [NB, h', w', Cout]
      A[kh, kw][np.ix_(np.arange(Cout), np.arange(NB), ih[okh], iw[okw])] = src.transpose(3, 0, 1, 2)
  B = w.transpose(0, 1, 3, 2).reshape(KH * KW * Cout, Cin)
  return A.reshape(KH * KW * Cout, NB * H * W), np.ascontiguousarray(B)


def split_ranges(Rn, splits):
  """[(begin, end)] of the `splits` contiguous ranges of L = 16 ceil(ceil(Rn / 16) / splits) rows;
  trailing ranges may be empty."""
  L = 16 * -(-(-(-Rn // 16)) // splits)
  return [(min(s * L, Rn), min((s + 1) * L, Rn)) for s in range(splits)]


def split_sum_ref(a_ri, b_rj, splits):
  """((p0 + p1) + p2) + ... in float32, p_s the chain from +0 over range s."""
  a_ri, b_rj = np.asarray(a_ri, F32), np.asarray(b_rj, F32)
  out = None
  for lo, hi in split_ranges(a_ri.shape[0], splits):
    if hi > lo:
      p = tr.gemm_chain(a_ri[lo:hi], b_rj[lo:hi])
    else:
      p = np.zeros((a_ri.shape[1], b_rj.shape[1]), F32)
    out = p if out is None else (out + p).astype(F32)
  return out


def pool_vjp_first_max(s, gp):
  """s [..., H, W, C], gp [..., H/2, W/2, C] -> gs like s.  Each gp element goes to the first
  position, in the order (0,0), (0,1), (1,0), (1,1), holding the window's maximum; a trailing odd
  row or column gets 0."""
  s, gp = np.asarray(s), np.asarray(gp)
  H, W, C = s.shape[-3:]
  PH, PW = H // 2, W // 2
  lead = s.shape[:-3]
  win = s[..., :2 * PH, :2 * PW, :].reshape(lead + (PH, 2, PW, 2, C))
  win = np.moveaxis(win, -4, -3).reshape(lead + (PH, PW, 4, C))         # [.., PH, PW, (dh, dw), C]
  first = np.argmax(win, axis=-2)                                       # numpy: the first maximum
  sel = (first[..., None, :] == np.arange(4)[:, None]).astype(gp.dtype) * gp[..., None, :]
  sel = np.moveaxis(sel.reshape(lead + (PH, PW, 2, 2, C)), -3, -4)      # [.., PH, 2, PW, 2, C]
  gs = np.zeros(s.shape, gp.dtype)
  gs[..., :2 * PH, :2 * PW, :] = sel.reshape(lead + (2 * PH, 2 * PW, C))
  return gs


def bn_batch_stats64(x):
  """x [..., C] -> (mean, var) float64 over every leading axis: var = mean(x^2) - mean^2, the flax
  0.4.0 form (biased)."""
  x = np.asarray(x, F64).reshape(-1, np.shape(x)[-1])
  mean = x.mean(0)
  return mean, (x * x).mean(0) - mean * mean


def bn_train64(x, scale, bias, eps=1e-5):
  mean, var = bn_batch_stats64(x)
  return (np.asarray(x, F64) - mean) * (np.asarray(scale, F64) / np.sqrt(var + eps)) + np.asarray(bias, F64)


# ---- the model: fixtures, the float32 forward by the oracle, the float64 forward in torch --------

import torch  # noqa: E402

from tests.helpers import qweight_of  # noqa: E402

NBLOCKS, CHANNELS, HW, CIN, T_STEPS, BATCH, CLASSES = 2, 16, 8, 2, 3, 2, 2
BITS, TAU, VTH, VR, EPS, KEEP = 4, 2.0, 1.0, 0.0, 1e-5, 0.9


def fixture(quantized, dtype="uint8", B=BATCH, T=T_STEPS, seed=77):
  """(variables as numpy trees, frames [B, T, 8, 8, 2]) of the two-block ConvDenseSNN the model tests
  run: 4-bit / 90 % pruned or unquantised, BatchNorm with a positive bias so that blocks fire."""
  from snnquantprune_amd import synthetic as syn
  v = syn.conv_net_variables(CHANNELS, CIN, NBLOCKS, HW, CLASSES * 10, quantized,
                             0.9 if quantized else -1.0,
                             gains=(4.0, 5.0, 8.0 if quantized else 5.0), random_bn=True)
  rng = np.random.default_rng(seed)
  for i in range(NBLOCKS):
    p = v["params"]["BatchNorm_%d" % i]
    p["scale"] = (1.5 + 0.2 * rng.standard_normal(CHANNELS)).astype(F32)
    p["bias"] = (0.5 + 0.1 * rng.standard_normal(CHANNELS)).astype(F32)
  x = np.minimum(rng.poisson(0.6, (B, T, HW, HW, CIN)), 255).astype(np.uint8)
  return v, (x.astype(F32) if dtype == "float32" else x)


def oracle_forward(params, x_bt, mask, quantized, stats=None, bits=BITS):
  """The training forward in float32 by the oracle.  `mask` [T, B, K] is the read-out's dropout
  mask; `stats` {i: (mean, var) float32 [T, C]} replaces the batch statistics (the sown ones).
  -> {"h%d", "s%d", "mean%d", "var%d" per block, "hd", "sd", "flat", "logits"}."""
  mode = "int" if quantized else "fseq"
  x = np.swapaxes(np.asarray(x_bt, F32), 0, 1)
  out = {}
  i = 0
  while "QuantConv_%d" % i in params:
    qw = qweight_of(oracle, params["QuantConv_%d" % i], bits, quantized)
    bn = params["BatchNorm_%d" % i]
    cur = np.stack([oracle.quant_conv(x[t], qw, None, ((1, 1), (1, 1)), mode=mode)
                    for t in range(x.shape[0])])
    if stats is None:
      mv = [bn_batch_stats64(cur[t]) for t in range(cur.shape[0])]
      mean = np.stack([m for m, _ in mv]).astype(F32)
      var = np.stack([s for _, s in mv]).astype(F32)
    else:
      mean, var = stats[i]
    y = np.stack([oracle.batchnorm_eval(cur[t], mean[t], var[t], bn["scale"], bn["bias"], EPS)
                  for t in range(cur.shape[0])])
    h, s = tr.lif_save_ref(y, TAU, VTH, VR)
    out.update({"cur%d" % i: cur, "mean%d" % i: mean, "var%d" % i: var, "h%d" % i: h, "s%d" % i: s})
    x = oracle.max_pool_2x2(s)
    i += 1
  flat = oracle.flatten_channel_major(x) * np.asarray(mask, F32)
  cur = oracle.quant_dense(flat, qweight_of(oracle, params["QuantDense_0"], bits, quantized), mode)
  h, s = tr.lif_save_ref(cur, TAU, VTH, VR)
  out.update(flat=flat, hd=h, sd=s,
             logits=s.astype(F64).mean(0).reshape(s.shape[1], -1, 10).mean(-1))
  return out


class _FirstMaxPool(torch.autograd.Function):
  """The 2x2 max pool of a spike raster [T, B, H, W, C], its gradient routed by pool_vjp_first_max."""

  @staticmethod
  def forward(ctx, s):
    ctx.s = s.detach().numpy()
    return torch.from_numpy(oracle.max_pool_2x2(ctx.s))

  @staticmethod
  def backward(ctx, g):
    return torch.from_numpy(pool_vjp_first_max(ctx.s, g.numpy()))


class TorchConvDenseSNN64:
  """The training forward of ConvDenseSNN (models.py:101-147, :189-190, :219-255) in float64 torch
  on the CPU; its backward is torch.autograd's, through the batch statistics too.  The spikes are
  the saved float32 ones (train_reference._SavedSpike), the pool routes by the first maximum."""

  def __init__(self, params, surrogate="atan", bits=BITS, group=10):
    self.surrogate, self.levels, self.group = surrogate, float(2 ** (bits - 1) - 1), group
    t64 = lambda v: torch.from_numpy(np.asarray(v, F64).copy())   # noqa: E731
    self.leaf = {}
    for name, leaf in params.items():
      if name.startswith("BatchNorm"):
        self.leaf[name] = {k: t64(leaf[k]).requires_grad_(True) for k in ("scale", "bias")}
      else:
        mask = leaf.get("prune_0", {}).get("mask")
        self.leaf[name] = {"kernel": t64(leaf["kernel"]).requires_grad_(True),
                           "a": t64(leaf["DuQ_0"]["a"]).requires_grad_(True),
                           "c": t64(leaf["DuQ_0"]["c"]).requires_grad_(True),
                           "mask": None if mask is None else t64(mask)}
    self.h_gap = 0.0
    self.wq, self.cur, self.xin = {}, {}, {}     # kept by forward(): kernel_fwd, currents, inputs

  def kernel_fwd(self, name):
    """prune(DuQ(kernel)), flax_qdense.py:74-85."""
    l = self.leaf[name]
    w = l["kernel"]
    if float(l["a"].detach()[0]) != -1.0:
      w = l["c"] * tr._round_ste(tr._hard_tanh(w / l["a"]), self.levels)
    if l["mask"] is not None:
      w = w * l["mask"]
    w.retain_grad()
    self.wq[name] = w
    return w

  def _scan(self, cur, h_saved, s_saved):
    """multi_step_LIF over cur [T, ...] replaying the saved spikes; records how far the float64 h
    is from the saved float32 one."""
    h32 = np.asarray(h_saved, F32)
    dsig = torch.from_numpy(tr.sg64(self.surrogate, (h32 - F32(VTH)).astype(F64)))
    s_sv = torch.from_numpy(np.asarray(s_saved, F64).copy())
    u = torch.zeros_like(cur[0])
    out = []
    for t in range(cur.shape[0]):
      h = u + (cur[t] - (u - VR)) / TAU
      self.h_gap = max(self.h_gap, float((h.detach() - torch.from_numpy(h32[t].astype(F64))).abs().max()))
      s = tr._SavedSpike.apply(h - VTH, s_sv[t], dsig[t])
      u = torch.where(s.bool(), torch.full_like(h, VR), h)
      out.append(s)
    return torch.stack(out)

  def forward(self, x_bt, mask, saved):
    """x_bt [B, T, H, W, C]; mask [T, B, K]; saved {"h%d", "s%d", "hd", "sd"} float32 as the forward
    under test sowed them -> logits float64 [B, classes]."""
    t64 = lambda v: torch.from_numpy(np.asarray(v, F64).copy())   # noqa: E731
    x = t64(x_bt).transpose(0, 1)
    self.stats = {}
    i = 0
    while "QuantConv_%d" % i in self.leaf:
      T, B, H, W, C = x.shape
      wq = self.kernel_fwd("QuantConv_%d" % i)
      cur = torch.nn.functional.conv2d(x.reshape(T * B, H, W, C).permute(0, 3, 1, 2),
                                       wq.permute(3, 2, 0, 1), padding=1)
      cur = cur.permute(0, 2, 3, 1).reshape(T, B, H, W, -1)
      cur.retain_grad()
      self.cur[i], self.xin[i] = cur, x.detach().numpy().reshape(T * B, H, W, C)
      mean = cur.mean((1, 2, 3))
      var = (cur * cur).mean((1, 2, 3)) - mean * mean
      bn = self.leaf["BatchNorm_%d" % i]
      mul = torch.rsqrt(var + EPS) * bn["scale"]
      y = (cur - mean[:, None, None, None]) * mul[:, None, None, None] + bn["bias"]
      self.stats[i] = (mean.detach().numpy(), var.detach().numpy())
      s = self._scan(y, saved["h%d" % i], saved["s%d" % i])
      x = _FirstMaxPool.apply(s)
      i += 1
    T, B = x.shape[:2]
    flat = x.permute(0, 1, 4, 2, 3).reshape(T, B, -1) * t64(mask)
    s = self._scan(flat @ self.kernel_fwd("QuantDense_0"), saved["hd"], saved["sd"])
    return s.mean(0).reshape(B, -1, self.group).mean(-1)

  def c_gamma_bound(self, i):
    """After a backward: what the float32 chain of conv block i's weight gradient may put into the
    gradient of DuQ's c, element-wise: sum_k |d wq_k / d c| gamma(Rn) (|A|^T |gI|)_k with A the
    gathered input, gI the currents' gradient and d wq / d c = wq / c."""
    wq = self.wq["QuantConv_%d" % i].detach().numpy()
    c = float(self.leaf["QuantConv_%d" % i]["c"].detach()[0])
    gI = self.cur[i].grad.numpy()
    a, b = wgrad_matrices(self.xin[i], gI.reshape((-1,) + gI.shape[2:]), wq.shape[:2], (1, 1),
                          ((1, 1), (1, 1)))
    mag = tr.gemm_mag(a, b).reshape(wq.shape)
    return float((np.abs(wq / c) * tr.gamma(a.shape[0]) * mag).sum())

  def grads(self):
    """{(layer, name): float64 array} after a backward, zeros where nothing reached a leaf."""
    out = {}
    for name, leaf in self.leaf.items():
      for k, t in leaf.items():
        if k != "mask":
          out[(name, k)] = np.zeros(t.shape) if t.grad is None else t.grad.numpy()
    return out
