"""Plain references for CextNet training (csrc/train_gate.hip, tcja_train.py, models.CextNet); no GPU.

  fma                                    fl(a b + c), one rounding (float32), element-wise
  first_max_gated                        the winning position of every 2x2 window of y = fl(x gate)
  gate_grad_gate_ref / gate_grad_input_ref   the two kernels, in their stated orders (float32), or
                                         the same rule in float64
  wgrad_f64_ref                          the float64-chain conv weight gradient of the model's first block
  conv1d_same4 / conv1d_vjp              the gate's 1-D convolutions (k = 4, padding (1, 2)) and their VJP
  stage_backward_ref                     the hand-derived backward of one gated stage
  stage64                                p = maxpool(x * sigmoid(conv_c(mean x) * conv_t(mean x))) in
                                         float64 torch, differentiated by autograd
  fixture / oracle_forward               the small model the tests train, its float32 forward by the oracle
  TorchCextNet64                         the training forward in float64 torch, replaying the saved spikes
"""
import numpy as np
import torch

from oracle import snn_oracle as oracle
from tests import conv_train_reference as cr
from tests import train_reference as tr
from tests.helpers import qweight_of

F32, F64 = np.float32, np.float64


# ---- the two kernels ---------------------------------------------------------------------------------

def fma(a, b, c):
  """fl(a b + c) with ONE rounding.  float32: the product is exact in float64; the float64 sum is
  taken to round-to-odd by the error term of TwoSum, so the second rounding (to float32) cannot
  differ from rounding the exact value.  float64 operands: a * b + c, two roundings."""
  a, b, c = np.asarray(a), np.asarray(b), np.asarray(c)
  if a.dtype != F32:
    return a * b + c
  with np.errstate(invalid="ignore", over="ignore"):
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _windows(v, H, W):
  """v [NB, H, W, C] -> [NB, PH, PW, 4, C], positions in the order (0,0), (0,1), (1,0), (1,1)."""
  NB, C = v.shape[0], v.shape[-1]
  PH, PW = H // 2, W // 2
  w = v[:, :2 * PH, :2 * PW].reshape(NB, PH, 2, PW, 2, C)
  return w.transpose(0, 1, 3, 2, 4, 5).reshape(NB, PH, PW, 4, C)


def first_max_gated(x, gate):
  """x [NB, H, W, C], gate [NB, C] -> best [NB, PH, PW, C] in 0..3: the first position at which
  y_i = fl(x_i gate) attains the window's maximum; a later position replaces the choice only when
  strictly greater (the compare rule of snnqp_maxpool2x2_backward, applied to y)."""
  x, gate = np.asarray(x), np.asarray(gate)
  NB, H, W, C = x.shape
  with np.errstate(invalid="ignore", over="ignore"):
    y = _windows((x * gate[:, None, None, :]).astype(x.dtype), H, W)
    best = np.zeros(y.shape[:3] + (C,), np.int64)
    vb = y[:, :, :, 0].copy()
    for k in range(1, 4):
      up = y[:, :, :, k] > vb
      vb = np.where(up, y[:, :, :, k], vb)
      best = np.where(up, k, best)
  return best


def gate_grad_gate_ref(x, gate, gp):
  """ggate[n, c] = the fmaf chain from +0 over the windows in ascending (ph, pw) of
  gp[n, ph, pw, c] x[n, p*, c]."""
  x, gate, gp = np.asarray(x), np.asarray(gate), np.asarray(gp)
  NB, H, W, C = x.shape
  acc = np.zeros((NB, C), x.dtype)
  if NB == 0 or H < 2 or W < 2:
    return acc
  best = first_max_gated(x, gate)
  xsel = np.take_along_axis(_windows(x, H, W), best[:, :, :, None, :], axis=3)[:, :, :, 0]
  for ph in range(H // 2):
    for pw in range(W // 2):
      acc = fma(gp[:, ph, pw], xsel[:, ph, pw], acc)
  return acc


def gate_grad_input_ref(x, gate, gp, gm):
  """gx = fl(route + fl(gm / (float)(H W))), route = fl(gp gate) at p* of each window, +0 elsewhere
  (and in a trailing odd row or column)."""
  x, gate, gp, gm = np.asarray(x), np.asarray(gate), np.asarray(gp), np.asarray(gm)
  NB, H, W, C = x.shape
  PH, PW = H // 2, W // 2
  route = np.zeros(x.shape, x.dtype)
  with np.errstate(invalid="ignore", over="ignore"):
    if NB and PH and PW:
      best = first_max_gated(x, gate)
      val = (gp * gate[:, None, None, :]).astype(x.dtype)
      sel = np.where(best[:, :, :, None, :] == np.arange(4)[:, None], val[:, :, :, None, :],
                     np.zeros((), x.dtype))                                   # [NB, PH, PW, 4, C]
      route[:, :2 * PH, :2 * PW] = sel.reshape(NB, PH, PW, 2, 2, C).transpose(
          0, 1, 3, 2, 4, 5).reshape(NB, 2 * PH, 2 * PW, C)
    mean_term = (gm / x.dtype.type(H * W)).astype(x.dtype)
    return (route + mean_term[:, None, None, :]).astype(x.dtype)


def wgrad_f64_ranges(Rn):
  """[(begin, end)] of the S = min(1024, max(1, ceil(Rn / 1024))) ranges of ceil(Rn / S) rows."""
  S = min(1024, max(1, -(-Rn // 1024)))
  Lr = -(-Rn // S) if Rn else 0
  return [(min(s * Lr, Rn), min((s + 1) * Lr, Rn)) for s in range(S)]


def wgrad_f64_ref(x, gI, ks, strides, pads):
  """snnqp_conv_weight_grad_f64: per range the r-ascending float64 chain acc = acc + x gI from +0
  (the product of two float32 values is exact in float64), the ranges summed in order in float64,
  one rounding to float32.  -> gw HWIO float32."""
  x, gI = np.asarray(x, F32), np.asarray(gI, F32)
  a, b = cr.wgrad_matrices(x, gI, ks, strides, pads)
  a, b = a.astype(F64), b.astype(F64)
  total = None
  with np.errstate(over="ignore", invalid="ignore"):
    for lo, hi in wgrad_f64_ranges(a.shape[0]):
      acc = np.zeros((a.shape[1], b.shape[1]), F64)
      for r in range(lo, hi):
        acc = acc + a[r][:, None] * b[r][None, :]
      total = acc if total is None else total + acc
    return total.astype(F32).reshape(tuple(ks) + (x.shape[-1], gI.shape[-1]))


# ---- the stage by hand ---------------------------------------------------------------------------------

def conv1d_same4(x, w):
  """x [B, L, Cin], w [4, Cin, Cout] -> [B, L, Cout], padding (1, 2) (SAME for k = 4)."""
  B, L, _ = x.shape
  xp = np.pad(x, ((0, 0), (1, 2), (0, 0)))
  return sum(np.einsum("bli,io->blo", xp[:, k:k + L], w[k]) for k in range(4))


def conv1d_vjp(x, w, g):
  """-> (gx like x, gw like w) of conv1d_same4 for the upstream g [B, L, Cout]."""
  B, L, _ = x.shape
  xp = np.pad(x, ((0, 0), (1, 2), (0, 0)))
  gxp = np.zeros_like(xp)
  gw = np.zeros_like(w)
  for k in range(4):
    gw[k] = np.einsum("bli,blo->io", xp[:, k:k + L], g)
    gxp[:, k:k + L] += np.einsum("blo,io->bli", g, w[k])
  return gxp[:, 1:1 + L], gw


def stage_forward_ref(x, wt, wc):
  """x [T, B, H, W, C], wt [4, T, T], wc [4, C, C] (float64) -> dict(m, a, b, gate, p)."""
  T, B, H, W, C = x.shape
  m = x.mean((2, 3))
  xb = m.transpose(1, 0, 2)                                      # [B, T, C]
  xc = xb.transpose(0, 2, 1)                                     # [B, C, T]
  a = conv1d_same4(xc, wt).transpose(2, 0, 1)                    # conv_t_out as [T, B, C]
  b = conv1d_same4(xb, wc).transpose(1, 0, 2)                    # conv_c_out as [T, B, C]
  gate = 1.0 / (1.0 + np.exp(-(a * b)))
  y = x * gate[:, :, None, None, :]
  return dict(m=m, a=a, b=b, gate=gate, p=oracle_pool(y))


def oracle_pool(y):
  H, W = y.shape[-3], y.shape[-2]
  v = y[..., :2 * (H // 2), :2 * (W // 2), :]
  v = v.reshape(y.shape[:-3] + (H // 2, 2, W // 2, 2, y.shape[-1]))
  return v.max(axis=(-4, -2))


def stage_backward_ref(x, wt, wc, gp):
  """The backward tcja_train.TcjaGate states, in the dtype of x (float64 for the autograd check):
  -> dict(ggate, gx, gwt, gwc, gm)."""
  T, B, H, W, C = x.shape
  f = stage_forward_ref(x, wt, wc)
  g = f["gate"]
  x4, gp4 = x.reshape(T * B, H, W, C), gp.reshape(T * B, H // 2, W // 2, C)
  ggate = gate_grad_gate_ref(x4, g.reshape(T * B, C), gp4).reshape(T, B, C)
  gz = ggate * (g * (1.0 - g))
  ga = (gz * f["b"]).transpose(1, 2, 0)                          # [B, C, T]
  gb = (gz * f["a"]).transpose(1, 0, 2)                          # [B, T, C]
  xb = f["m"].transpose(1, 0, 2)
  xc = xb.transpose(0, 2, 1)
  gxc, gwt = conv1d_vjp(xc, wt, ga)
  gxb, gwc = conv1d_vjp(xb, wc, gb)
  gm = (gxb + gxc.transpose(0, 2, 1)).transpose(1, 0, 2)         # [T, B, C]
  gx = gate_grad_input_ref(x4, g.reshape(T * B, C), gp4, gm.reshape(T * B, C)).reshape(x.shape)
  return dict(ggate=ggate, gx=gx, gwt=gwt, gwc=gwc, gm=gm)


# ---- the stage in float64 torch --------------------------------------------------------------------------

class FirstMaxPool(torch.autograd.Function):
  """2x2 max pool of [..., H, W, C]; the gradient goes to the first maximum of each window."""

  @staticmethod
  def forward(ctx, y):
    ctx.y = y.detach().numpy()
    return torch.from_numpy(oracle_pool(ctx.y).copy())

  @staticmethod
  def backward(ctx, g):
    return torch.from_numpy(cr.pool_vjp_first_max(ctx.y, g.numpy()))


def _conv1d_t(x, w):
  """torch: x [B, L, Cin], w [4, Cin, Cout] -> [B, L, Cout], padding (1, 2)."""
  xp = torch.nn.functional.pad(x.transpose(1, 2), (1, 2))
  return torch.nn.functional.conv1d(xp, w.permute(2, 1, 0)).transpose(1, 2)


def gate64(s, wt, wc):
  """s [T, B, H, W, C] -> gate [T, B, C], models.py:42-95 in torch."""
  m = s.mean((2, 3))
  xb = m.transpose(0, 1)
  xc = xb.transpose(1, 2)
  a = _conv1d_t(xc, wt).permute(2, 0, 1)
  b = _conv1d_t(xb, wc).transpose(0, 1)
  return torch.sigmoid(b * a)


def stage64(x, wt, wc, first_max=False):
  """The stated forward in torch: with first_max the pool routes by the first-maximum rule,
  otherwise it is torch's own max (for inputs without ties both are the derivative)."""
  y = x * gate64(x, wt, wc)[:, :, None, None, :]
  if first_max:
    return FirstMaxPool.apply(y)
  T, B, H, W, C = y.shape
  if min(H, W) < 2:                                              # no window: an empty raster
    return y[:, :, :H // 2, :W // 2]
  p = torch.nn.functional.max_pool2d(y.reshape(T * B, H, W, C).permute(0, 3, 1, 2), 2)
  return p.permute(0, 2, 3, 1).reshape(T, B, H // 2, W // 2, C)


# ---- the model -----------------------------------------------------------------------------------------

CHANNELS, HW, CIN, T_STEPS, BATCH, CLASSES = 16, 64, 2, 4, 2, 2
BITS, TAU, VTH, VR, EPS, KEEP = 4, 2.0, 1.0, 0.0, 1e-5, 0.9
NCONV = 5
CONV_OF_BLOCK = (0, 1, 2, 3, 6)          # QuantConv index of the five 3x3 blocks
GATE_CONVS = ((4, 5), (7, 8))            # (conv_t, conv_c) of the two gates


def fixture(quantized, dtype="uint8", B=BATCH, T=T_STEPS, seed=91):
  """(variables as numpy trees, frames [B, T, 64, 64, 2]) of the small CextNet the model tests train:
  16 channels, 4-bit / 90 % pruned or unquantised (a == -1, no mask), BatchNorm with a positive
  bias so that every block fires, gate kernels large enough for the gates to spread."""
  from snnquantprune_amd import synthetic as syn
  C = CHANNELS
  shapes = {0: (3, 3, CIN, C), 1: (3, 3, C, C), 2: (3, 3, C, C), 3: (3, 3, C, C), 4: (4, T, T),
            5: (4, C, C), 6: (3, 3, C, C), 7: (4, T, T), 8: (4, C, C)}
  gains = {0: 4.0, 1: 5.0, 2: 5.0, 3: 5.0, 6: 5.0, 4: 6.0, 5: 12.0, 7: 6.0, 8: 12.0}
  prune = 0.9 if quantized else -1.0
  params, stats = {}, {}
  for i in range(9):
    # the gates' T x T kernels keep a quarter of their 4 T T weights: ten percent of 64 would be six
    p = (0.75 if i in (4, 7) else prune) if quantized else -1.0
    params["QuantConv_%d" % i] = syn.quant_leaf(shapes[i], gains[i], seed + i, quantized, p)
  rng = np.random.default_rng(seed)
  for i in range(NCONV):
    p, s = syn.bn_leaf(C, True, seed + 100 + i)
    p["scale"] = (1.5 + 0.2 * rng.standard_normal(C)).astype(F32)
    p["bias"] = (0.5 + 0.1 * rng.standard_normal(C)).astype(F32)
    params["BatchNorm_%d" % i], stats["BatchNorm_%d" % i] = p, s
  flat = (HW // 32) * (HW // 32) * C
  params["QuantDense_0"] = syn.quant_leaf((flat, 4 * C), 8.0, seed + 50, quantized, prune)
  params["QuantDense_1"] = syn.quant_leaf((4 * C, CLASSES * 10), 8.0, seed + 51, quantized, prune)
  x = np.minimum(rng.poisson(0.6, (B, T, HW, HW, CIN)), 255).astype(np.uint8)
  return {"params": params, "batch_stats": stats}, (x.astype(F32) if dtype == "float32" else x)


def oracle_conv_block(x, leaf, bn, quantized, mode, stats=None):
  """x [T, B, H, W, Cin] float32 -> dict(cur, mean, var, h, s): the conv block's training forward
  by the oracle; `stats` (mean, var) [T, C] replaces the batch statistics."""
  qw = qweight_of(oracle, leaf, BITS, quantized)
  cur = np.stack([oracle.quant_conv(x[t], qw, None, ((1, 1), (1, 1)), mode=mode)
                  for t in range(x.shape[0])])
  if stats is None:
    mv = [cr.bn_batch_stats64(cur[t]) for t in range(cur.shape[0])]
    mean = np.stack([m for m, _ in mv]).astype(F32)
    var = np.stack([v for _, v in mv]).astype(F32)
  else:
    mean, var = stats
  y = np.stack([oracle.batchnorm_eval(cur[t], mean[t], var[t], bn["scale"], bn["bias"], EPS)
                for t in range(cur.shape[0])])
  h, s = tr.lif_save_ref(y, TAU, VTH, VR)
  return dict(cur=cur, mean=mean, var=var, h=h, s=s)


def oracle_gate(s, params, j, quantized):
  """The eval TCJA arithmetic on the raster s [T, B, H, W, C]: -> (gated raster, gate)."""
  it, ic = GATE_CONVS[j]
  return oracle.tcja(s, qweight_of(oracle, params["QuantConv_%d" % it], BITS, quantized),
                     qweight_of(oracle, params["QuantConv_%d" % ic], BITS, quantized))


def oracle_dense_block(x, leaf, quantized, mode):
  cur = oracle.quant_dense(x, qweight_of(oracle, leaf, BITS, quantized), mode)
  return tr.lif_save_ref(cur, TAU, VTH, VR)


def oracle_forward(params, x_bt, masks, quantized):
  """The whole training forward in float32 by the oracle, on its own batch statistics.
  masks (m0 [T, B, K], m1 [T, B, 4 C]).  -> {"in%d", "h%d", "s%d", "mean%d", "var%d" per conv block,
  "gate0", "gate1", "hd1", "sd1", "hd2", "sd2", "logits"}."""
  mode = "int" if quantized else "fseq"
  x = np.swapaxes(np.asarray(x_bt, F32), 0, 1)
  out = {}
  for i in range(NCONV):
    blk = oracle_conv_block(x, params["QuantConv_%d" % CONV_OF_BLOCK[i]], params["BatchNorm_%d" % i],
                            quantized, "fseq" if i == 4 else mode)
    out["in%d" % i] = x
    out.update({"%s%d" % (k, i): v for k, v in blk.items()})
    if i < 3:
      x = oracle.max_pool_2x2(blk["s"])
    else:
      y, gate = oracle_gate(blk["s"], params, i - 3, quantized)
      out["gate%d" % (i - 3)] = gate
      x = oracle.max_pool_2x2(y)
  flat = oracle.flatten_channel_major(x) * np.asarray(masks[0], F32)
  out["hd1"], out["sd1"] = oracle_dense_block(flat, params["QuantDense_0"], quantized, "fseq")
  out["hd2"], out["sd2"] = oracle_dense_block(out["sd1"] * np.asarray(masks[1], F32),
                                              params["QuantDense_1"], quantized, mode)
  s = out["sd2"]
  out["logits"] = s.astype(F64).mean(0).reshape(s.shape[1], -1, 10).mean(-1)
  return out


class TorchCextNet64(cr.TorchConvDenseSNN64):
  """The training forward of CextNet (models.py:101-257) in float64 torch on the CPU; its backward
  is torch.autograd's, through the batch statistics, the spatial means and the gates too.  The
  spikes are the saved float32 ones, every pool routes by the first maximum (the gated stages' on
  y = s * gate), the surrogate derivative is taken at the saved float32 h."""

  def forward(self, x_bt, masks, saved):
    """x_bt [B, T, H, W, C]; masks (m0, m1) as drawn; saved {"h%d", "s%d" for the five conv blocks,
    "hd1", "sd1", "hd2", "sd2"} float32 -> logits float64 [B, classes]."""
    t64 = lambda v: torch.from_numpy(np.asarray(v, F64).copy())   # noqa: E731
    x = t64(x_bt).transpose(0, 1)
    self.stats, self.gates = {}, {}
    for i in range(NCONV):
      T, B, H, W, C = x.shape
      wq = self.kernel_fwd("QuantConv_%d" % CONV_OF_BLOCK[i])
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
      if i < 3:
        x = FirstMaxPool.apply(s)
      else:
        it, ic = GATE_CONVS[i - 3]
        gate = gate64(s, self.kernel_fwd("QuantConv_%d" % it), self.kernel_fwd("QuantConv_%d" % ic))
        self.gates[i - 3] = gate.detach().numpy()
        x = FirstMaxPool.apply(s * gate[:, :, None, None, :])
    T, B = x.shape[:2]
    flat = x.permute(0, 1, 4, 2, 3).reshape(T, B, -1) * t64(masks[0])
    s1 = self._scan(flat @ self.kernel_fwd("QuantDense_0"), saved["hd1"], saved["sd1"])
    s2 = self._scan((s1 * t64(masks[1])) @ self.kernel_fwd("QuantDense_1"), saved["hd2"], saved["sd2"])
    return s2.mean(0).reshape(B, -1, self.group).mean(-1)

  def c_gamma_bound(self, i):
    """As the base class's, for conv block i (its kernel is QuantConv_<CONV_OF_BLOCK[i]>)."""
    name = "QuantConv_%d" % CONV_OF_BLOCK[i]
    wq = self.wq[name].detach().numpy()
    c = float(self.leaf[name]["c"].detach()[0])
    gI = self.cur[i].grad.numpy()
    a, b = cr.wgrad_matrices(self.xin[i], gI.reshape((-1,) + gI.shape[2:]), wq.shape[:2], (1, 1),
                             ((1, 1), (1, 1)))
    mag = tr.gemm_mag(a, b).reshape(wq.shape)
    return float((np.abs(wq / c) * tr.gamma(a.shape[0]) * mag).sum())
