"""Times one DenseSNN train_step at config C2 (B = 256, T = 20, 2048 -> 512 -> 110, 8-bit DuQ,
50 % pruned, uint8 spikes, atan surrogate, Adam) on the HIP path, per step and per backward
kernel, against a plain PyTorch-eager float32 autograd statement of the same step on the same GPU
(the reference's own training comparison is against a PyTorch SNN, examples/norse_cmp).
Prints one JSON line.

  python tools/train_step_time.py [--steps 20] [--warmup 5] [--batch 256] [--frames 20]

--conv times one ConvDenseSNN train_step at the C3 topology instead (three 3x3 conv blocks of 128
channels on 128 x 128 x 2 frames, 4-bit DuQ, 90 % pruned, default B = 2, T = 20: the reference's
per-device batch), against the same step in PyTorch eager float32 autograd, and conv1's weight
gradient with one range of r against the default split.  It also prints the step and the
connection launch of conv1 and conv2 with nn.set_train_conv_mfma on and off (alternating, --reps
timings each), and conv0's direct-form connection.

  python tools/train_step_time.py --conv [--steps 5] [--warmup 2] [--batch 2] [--frames 20] [--hw 128] [--reps 3]

--conv --neuron multi_step_LIF|plif|lif times that step with the given neuron only (PLIF and LIF
learn their `tau` under config.learn_neuron_params), --reps timings in one process, and the BPTT
scan alone on conv1's shape, for PLIF / LIF at each --lanes target of its row split.

  python tools/train_step_time.py --conv --neuron plif [--lanes 0 65536 262144 1048576]

--cext times one CextNet train_step on the reference's geometry (128 x 128 x 2 frames, 128 channels,
4-bit DuQ, 90 % pruned, default B = 2, T = 20, atan, Adam), the two kernels of csrc/train_gate.hip
alone on both gated stages' shapes, block 0's weight gradient on the float64 and the float32 chain, and the same step in PyTorch eager float32 autograd; --reps
timings of each.

  python tools/train_step_time.py --cext [--steps 5] [--warmup 2] [--batch 2] [--frames 20] [--hw 128] [--reps 3]

--window W (the dense step and --conv): the recording is trained as windows of W steps with carried
membranes (train_utils.train_step_windows), ceil(T / W) updates per recording; prints
the time per recording, and the allocator's level before and its peak
(torch.cuda.max_memory_allocated()) over one more recording run from a cleared packing cache, and
nothing else.  Without it the step's line carries the same two figures.

  python tools/train_step_time.py --conv --window 5

--conv --remat W [--batch B]: the step with config.remat = W -- the conv blocks keep neither their
currents nor h and recompute them in the backward in chunks of W steps (conv_train.RematConvBlock,
DESIGN.md 19), one update per recording with the whole-run gradient.  Prints ms per step, the
allocator's level before the step, its level after the training forward (what the blocks keep;
taken over one forward and backward of the model on copies of the parameters) and the step's
peak, from a cleared packing cache, and nothing else.  The --conv line without the flag carries
the same three figures.

  python tools/train_step_time.py --conv --remat 5 --batch 16
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time_and_peak(fn, steps, warmup):
  """_time, then the allocator's level before and its peak over one more call (bytes), taken from
  a cleared packing cache: that cache keeps the packed kernels of up to 128 earlier parameter
  versions (DuQ's a and c are part of its key and move with every update), so its level grows
  with the number of updates so far and would hide what one call needs."""
  from snnquantprune_amd import packing
  ms = _time(fn, steps, warmup)
  packing.clear_cache()
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  fn()
  torch.cuda.synchronize()
  return ms, (before, torch.cuda.max_memory_allocated())


def _after_forward(model, state, batch, tu):
  """The allocator's growth over one training forward of `model` on gradient-carrying copies of the
  state's parameters, the logits alive: what the blocks keep for the backward (bytes).  The
  backward then runs, so the graph is whole."""
  from snnquantprune_amd import packing

  def leaves(tree):
    return {k: (leaves(t) if isinstance(t, dict) else t.detach().clone().requires_grad_(True))
            for k, t in tree.items()}

  params = leaves(state.params["params"])
  packing.clear_cache()
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()
  (logits, _), _ = model.apply({"params": params, "batch_stats": state.batch_stats}, batch["dvs_matrix"],
                               train=True, rng=0, mutable=["batch_stats"])
  torch.cuda.synchronize()
  kept = torch.cuda.memory_allocated() - before
  tu.mse_loss(logits, batch["label"]).backward()
  torch.cuda.synchronize()
  return kept


def _remat_line(args, model, batch, box, tu):
  """The --conv --remat run: one JSON line."""
  def step():
    box[0], _ = tu.train_step(box[0], batch, 0, lambda s: 1e-4, 0.0, 0.0, tu.mse_loss)

  ms, peak = _time_and_peak(step, args.steps, args.warmup)
  kept = _after_forward(model, box[0], batch, tu)
  print(json.dumps({"workload": "conv_dense_snn_c3_train_step", "batch": args.batch, "frames": args.frames,
                    "hw": args.hw, "remat": args.remat, "chunks": -(-args.frames // args.remat),
                    "hip_train_step_ms": round(ms, 3), "hip_memory_before_bytes": peak[0],
                    "hip_memory_after_forward_bytes": peak[0] + kept, "hip_peak_memory_bytes": peak[1],
                    "samples_per_s": round(args.batch / ms * 1e3, 1)}))


def _window_line(workload, args, batch, box, tu):
  """The --window run of the dense and the conv step: one JSON line."""
  def step():
    box[0], _, _ = tu.train_step_windows(box[0], batch, 0, lambda s: 1e-4, 0.0, 0.0, tu.mse_loss,
                                         window=args.window)

  ms, peak = _time_and_peak(step, args.steps, args.warmup)
  print(json.dumps({"workload": workload, "batch": args.batch, "frames": args.frames, "window": args.window,
                    "updates_per_recording": -(-args.frames // args.window),
                    "hip_recording_ms": round(ms, 3), "hip_memory_before_bytes": peak[0],
                    "hip_peak_memory_bytes": peak[1],
                    "samples_per_s": round(args.batch / ms * 1e3, 1)}))


def _time(fn, steps, warmup):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(steps):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / steps


class _Spike(torch.autograd.Function):
  @staticmethod
  def forward(ctx, x):
    ctx.save_for_backward(x)
    return (x >= 0).to(x.dtype)

  @staticmethod
  def backward(ctx, g):
    (x,) = ctx.saved_tensors
    return g / (1 + (torch.pi * x) ** 2)


def _eager_loss(params, x, labels, tau=2.0, L=127.0):
  """The same step as float32 torch autograd: DuQ + prune, two dense blocks, LIF, vote, MSE."""
  def wq(leaf):
    w, a, c, m = leaf["kernel"], leaf["DuQ_0"]["a"], leaf["DuQ_0"]["c"], leaf["prune_0"]["mask"]
    y = torch.nn.functional.hardtanh(w / a)
    y = y + (torch.round(y * L) / L - y).detach()
    return y * c * m

  def block(xs, w):
    cur = torch.einsum("tbk,kn->tbn", xs, w)
    u = torch.zeros_like(cur[0])
    out = []
    for t in range(cur.shape[0]):
      u = u + (cur[t] - u) / tau
      s = _Spike.apply(u - 1.0)
      u = u * (1 - s.detach())
      out.append(s)
    return torch.stack(out)

  x0 = x.transpose(0, 1).to(torch.float32)
  s1 = block(x0, wq(params["QuantDense_0"]))
  s2 = block(s1, wq(params["QuantDense_1"]))
  logits = s2.mean(0).reshape(s2.shape[1], -1, 10).mean(-1)
  oh = torch.nn.functional.one_hot(labels, logits.shape[1]).to(torch.float32)
  return torch.mean(torch.square(logits - oh))


def _eager_conv_loss(params, x, labels, nblocks, keep_mask, tau=2.0, L=7.0, eps=1e-5):
  """The ConvDenseSNN step as float32 torch autograd: DuQ + prune, conv + batch-statistics
  BatchNorm per time step + LIF + max pool, flatten, dropout, dense + LIF, vote, MSE."""
  def wq(leaf):
    w, a, c, m = leaf["kernel"], leaf["DuQ_0"]["a"], leaf["DuQ_0"]["c"], leaf["prune_0"]["mask"]
    y = torch.nn.functional.hardtanh(w / a)
    y = y + (torch.round(y * L) / L - y).detach()
    return y * c * m

  def scan(cur):
    u = torch.zeros_like(cur[0])
    out = []
    for t in range(cur.shape[0]):
      u = u + (cur[t] - u) / tau
      s = _Spike.apply(u - 1.0)
      u = u * (1 - s.detach())
      out.append(s)
    return torch.stack(out)

  xs = x.transpose(0, 1).to(torch.float32).permute(0, 1, 4, 2, 3)            # [T, B, C, H, W]
  for i in range(nblocks):
    T, B = xs.shape[:2]
    w = wq(params["QuantConv_%d" % i]).permute(3, 2, 0, 1)
    cur = torch.nn.functional.conv2d(xs.reshape((T * B,) + tuple(xs.shape[2:])), w, padding=1)
    cur = cur.reshape((T, B) + tuple(cur.shape[1:]))
    mean = cur.mean((1, 3, 4), keepdim=True)
    var = (cur * cur).mean((1, 3, 4), keepdim=True) - mean * mean
    bn = params["BatchNorm_%d" % i]
    cur = (cur - mean) * (torch.rsqrt(var + eps) * bn["scale"][None, None, :, None, None]) \
        + bn["bias"][None, None, :, None, None]
    s = scan(cur)
    xs = torch.nn.functional.max_pool2d(s.reshape((T * B,) + tuple(s.shape[2:])), 2)
    xs = xs.reshape((T, B) + tuple(xs.shape[1:]))
  flat = xs.reshape(xs.shape[0], xs.shape[1], -1) * keep_mask
  s2 = scan(torch.einsum("tbk,kn->tbn", flat, wq(params["QuantDense_0"])))
  logits = s2.mean(0).reshape(s2.shape[1], -1, 10).mean(-1)
  oh = torch.nn.functional.one_hot(labels, logits.shape[1]).to(torch.float32)
  return torch.mean(torch.square(logits - oh))


def _eager_cext_loss(params, x, labels, keep0, keep1, tau=2.0, L=7.0, eps=1e-5):
  """The CextNet step as float32 torch autograd: five conv blocks (batch-statistics BatchNorm per
  time step), the two TCJA gates, 2x2 max pools, flatten, two dropout masks, two dense blocks, vote,
  MSE."""
  def wq(leaf):
    w, a, c, m = leaf["kernel"], leaf["DuQ_0"]["a"], leaf["DuQ_0"]["c"], leaf["prune_0"]["mask"]
    y = torch.nn.functional.hardtanh(w / a)
    y = y + (torch.round(y * L) / L - y).detach()
    return y * c * m

  def scan(cur):
    u = torch.zeros_like(cur[0])
    out = []
    for t in range(cur.shape[0]):
      u = u + (cur[t] - u) / tau
      s = _Spike.apply(u - 1.0)
      u = u * (1 - s.detach())
      out.append(s)
    return torch.stack(out)

  def conv1d(v, w):                                      # v [B, L, Cin], w [4, Cin, Cout], SAME
    vp = torch.nn.functional.pad(v.transpose(1, 2), (1, 2))
    return torch.nn.functional.conv1d(vp, w.permute(2, 1, 0)).transpose(1, 2)

  def pool(v):
    T, B = v.shape[:2]
    p = torch.nn.functional.max_pool2d(v.reshape((T * B,) + tuple(v.shape[2:])), 2)
    return p.reshape((T, B) + tuple(p.shape[1:]))

  xs = x.transpose(0, 1).to(torch.float32).permute(0, 1, 4, 2, 3)            # [T, B, C, H, W]
  q = 0
  for i in range(5):
    T, B = xs.shape[:2]
    w = wq(params["QuantConv_%d" % q]).permute(3, 2, 0, 1)
    q += 1
    cur = torch.nn.functional.conv2d(xs.reshape((T * B,) + tuple(xs.shape[2:])), w, padding=1)
    cur = cur.reshape((T, B) + tuple(cur.shape[1:]))
    mean = cur.mean((1, 3, 4), keepdim=True)
    var = (cur * cur).mean((1, 3, 4), keepdim=True) - mean * mean
    bn = params["BatchNorm_%d" % i]
    cur = (cur - mean) * (torch.rsqrt(var + eps) * bn["scale"][None, None, :, None, None]) \
        + bn["bias"][None, None, :, None, None]
    s = scan(cur)
    if i >= 3:
      m = s.mean((3, 4)).transpose(0, 1)                                     # [B, T, C]
      a = conv1d(m.transpose(1, 2), wq(params["QuantConv_%d" % q])).permute(2, 0, 1)
      b = conv1d(m, wq(params["QuantConv_%d" % (q + 1)])).transpose(0, 1)
      q += 2
      s = s * torch.sigmoid(b * a)[:, :, :, None, None]
    xs = pool(s)
  flat = xs.reshape(xs.shape[0], xs.shape[1], -1) * keep0
  s1 = scan(torch.einsum("tbk,kn->tbn", flat, wq(params["QuantDense_0"])))
  s2 = scan(torch.einsum("tbk,kn->tbn", s1 * keep1, wq(params["QuantDense_1"])))
  logits = s2.mean(0).reshape(s2.shape[1], -1, 10).mean(-1)
  oh = torch.nn.functional.one_hot(labels, logits.shape[1]).to(torch.float32)
  return torch.mean(torch.square(logits - oh))


def cext_main(args):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, synthetic as syn, train_utils as tu
  dev = torch.device("cuda:0")
  B, T, HW, C = args.batch, args.frames, args.hw, 128
  cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=C, dropout=0.9)
  cfg.optimizer = "adam"
  model = models.CextNet(num_classes=11, config=cfg)
  v = syn.cextnet_variables(C, T, HW, 110, 0.9)
  variables = nn.tree_from_numpy(v, dev)
  x = torch.from_numpy(syn.poisson_counts((B, T, HW, HW, 2), 0.3, seed=941)).to(dev)
  labels = torch.arange(B, device=dev) % 11
  batch = {"dvs_matrix": x, "label": labels}
  box = [tu.create_train_state(variables, cfg, model)]

  def hip_step():
    box[0], _ = tu.train_step(box[0], batch, 0, lambda s: 1e-4, 0.0, 0.0, tu.mse_loss)

  _time(hip_step, 1, args.warmup)
  hip_ms = [_time(hip_step, args.steps, 0) for _ in range(args.reps)]

  # the two gate kernels alone, on the shapes of both gated stages
  kern = {}
  for j, hw in enumerate((HW // 8, HW // 16)):
    xs = (torch.rand((T, B, hw, hw, C), device=dev) < 0.2).to(torch.float32)
    gate = torch.rand((T, B, C), device=dev)
    gp = torch.randn((T, B, hw // 2, hw // 2, C), device=dev)
    gm = torch.randn((T, B, C), device=dev)
    kern["gate%d_grad_gate_ms" % j] = [_time(lambda: ops.gate_pool_grad_gate(xs, gate, gp), 50, 5)
                                       for _ in range(args.reps)]
    kern["gate%d_grad_input_ms" % j] = [_time(lambda: ops.gate_pool_grad_input(xs, gate, gp, gm), 50, 5)
                                        for _ in range(args.reps)]
    del xs, gate, gp, gm

  # block 0's weight gradient on the step's shapes: the float64 chain the model uses, and the
  # float32 MFMA chain of the other blocks
  geom0 = ops.ConvGeom(HW, HW, 2, C, 3, 3, (1, 1), ((1, 1), (1, 1)))
  x0 = x.transpose(0, 1).reshape(T * B, HW, HW, 2).to(torch.float32).contiguous()
  g0 = torch.randn((T * B, HW, HW, C), device=dev)
  kern["conv0_weight_grad_f64_ms"] = [_time(lambda: ops.conv_weight_grad_f64(x0, g0, geom0), 10, 2)
                                      for _ in range(args.reps)]
  kern["conv0_weight_grad_f32_ms"] = [_time(lambda: ops.conv_weight_grad(x0, g0, geom0), 10, 2)
                                      for _ in range(args.reps)]
  del x0, g0

  eparams = {k: {kk: ({kkk: t.detach().clone().requires_grad_(True) for kkk, t in vv.items()}
                      if isinstance(vv, dict) else vv.detach().clone().requires_grad_(True))
                 for kk, vv in leaf.items()} for k, leaf in nn.tree_from_numpy(v, dev)["params"].items()}
  opt = torch.optim.Adam([t for _, t in tu._flatten(eparams)], lr=1e-4, eps=1e-8)
  K = (HW >> 5) ** 2 * C
  keep0 = (torch.rand((T, B, K), device=dev) < 0.9).to(torch.float32)
  keep1 = (torch.rand((T, B, 4 * C), device=dev) < 0.9).to(torch.float32)

  def eager_step():
    opt.zero_grad(set_to_none=True)
    _eager_cext_loss(eparams, x, labels, keep0, keep1).backward()
    opt.step()

  _time(eager_step, 1, args.warmup)
  eager_ms = [_time(eager_step, args.steps, 0) for _ in range(args.reps)]
  print(json.dumps({"workload": "cextnet_train_step", "batch": B, "frames": T, "hw": HW,
                    "hip_train_step_ms": [round(t, 3) for t in hip_ms],
                    "eager_torch_train_step_ms": [round(t, 3) for t in eager_ms],
                    "speedup_vs_eager": round(min(eager_ms) / min(hip_ms), 2),
                    "samples_per_s": round(B / min(hip_ms) * 1e3, 1),
                    **{k: [round(t, 4) for t in val] for k, val in kern.items()}}))


def neuron_main(args):
  """--conv --neuron {multi_step_LIF, plif, lif}: the ConvDenseSNN step of --conv with that neuron
  (PLIF / LIF under config.learn_neuron_params, a `tau` leaf per block), --reps timings in one
  process, and the BPTT scan of conv1's shape alone for several `splits` (0: the default)."""
  from functools import partial
  import numpy as np
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, spiking_learning as sl, synthetic as syn, train_utils as tu
  dev = torch.device("cuda:0")
  B, T, HW, C, NB = args.batch, args.frames, args.hw, 128, 3
  cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=C, dropout=0.9)
  cfg.optimizer = "adam"
  v = syn.conv_net_variables(C, 2, NB, HW, 110, True, 0.9)
  if args.neuron != "multi_step_LIF":
    cls = sl.parametric_leaky_IF if args.neuron == "plif" else sl.LIF
    cfg.neuron_dynamics = partial(cls, init_tau=2.0, spike_fn=sl.atan)
    cfg.learn_neuron_params = True
    for i, width in enumerate((C,) * NB + (110,)):
      v["params"]["%s_%d" % (cls.__name__, i)] = {
          "tau": np.zeros(1 if args.neuron == "plif" else width, np.float32)}     # m = d = 0.5: tau 2
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(v, dev)
  x = torch.from_numpy(syn.poisson_counts((B, T, HW, HW, 2), 0.3, seed=941)).to(dev)
  batch = {"dvs_matrix": x, "label": torch.arange(B, device=dev) % 11}
  box = [tu.create_train_state(variables, cfg, model)]

  def hip_step():
    box[0], _ = tu.train_step(box[0], batch, 0, lambda s: 1e-4, 0.0, 0.0, tu.mse_loss)

  _time(hip_step, 1, args.warmup)
  out = {"workload": "conv_dense_snn_c3_train_step", "neuron": args.neuron, "batch": B, "frames": T, "hw": HW,
         "hip_train_step_ms": [round(_time(hip_step, args.steps, 0), 3) for _ in range(args.reps)]}
  # the scan's backward alone on conv1's shape [T, B (HW/2)^2, C]
  R = B * (HW // 2) ** 2
  h = torch.randn((T, R, C), device=dev) + 0.5
  g = torch.randn((T, R, C), device=dev)
  if args.neuron == "multi_step_LIF":
    nrn = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
    out["lif_backward_ms"] = [round(_time(lambda: ops.lif_backward(h, nrn, L.SURR_ATAN, gs=g), 20, 3), 4)
                              for _ in range(args.reps)]
  else:
    nrn = ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, 0.5, 1.0, 0.0) if args.neuron == "plif" else \
        ops.Neuron(L.NEURON_LIF, 0.0, 1.0, 0.0, decay=torch.full((C,), 0.5, device=dev))
    out["neuron_backward_default_splits"] = ops.neuron_backward_splits(T, R, C)
    for lanes in args.lanes:
      splits = None if lanes == 0 else max(1, min(R, -(-lanes // C)))
      out["neuron_backward_ms_lanes_%d" % lanes] = [
          round(_time(lambda: ops.neuron_backward(h, g, nrn, L.SURR_ATAN, gs=g, splits=splits), 20, 3), 4)
          for _ in range(args.reps)]
  print(json.dumps(out))


def conv_main(args):
  if args.neuron is not None:
    return neuron_main(args)
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, synthetic as syn, train_utils as tu
  dev = torch.device("cuda:0")
  B, T, HW, C, NB = args.batch, args.frames, args.hw, 128, 3
  cfg = syn.make_config(bits=4, prune_percentage=0.9, channels=C, dropout=0.9)
  cfg.optimizer = "adam"
  if args.remat:
    cfg.remat = args.remat
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  v = syn.conv_net_variables(C, 2, NB, HW, 110, True, 0.9)
  variables = nn.tree_from_numpy(v, dev)
  x = torch.from_numpy(syn.poisson_counts((B, T, HW, HW, 2), 0.3, seed=941)).to(dev)
  labels = torch.arange(B, device=dev) % 11
  batch = {"dvs_matrix": x, "label": labels}
  box = [tu.create_train_state(variables, cfg, model)]
  if args.window:
    return _window_line("conv_dense_snn_c3_train_windows", args, batch, box, tu)
  if args.remat:
    return _remat_line(args, model, batch, box, tu)

  def hip_step():
    box[0], _ = tu.train_step(box[0], batch, 0, lambda s: 1e-4, 0.0, 0.0, tu.mse_loss)

  hip_ms, hip_peak = _time_and_peak(hip_step, args.steps, args.warmup)
  hip_kept = _after_forward(model, box[0], batch, tu)

  # the A/B of nn.set_train_conv_mfma in one process: the whole step with the connection of conv1
  # and conv2 on the MFMA currents kernel (on) and on the direct-form kernel (off, the launch of
  # earlier versions), alternating, `reps` timings each after the warm-up above
  ab = {True: [], False: []}
  for _ in range(args.reps):
    for on in (True, False):
      nn.set_train_conv_mfma(on)
      ab[on].append(_time(hip_step, args.steps, 1))
  nn.set_train_conv_mfma(True)

  # the connection launch of every conv block alone, on the step's shapes: conv0 on the uint8
  # frames (direct form either way), conv1 and conv2 on a bit-packed raster both ways
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  conn = {}
  hw, cin = HW, 2
  for i in range(NB):
    leaf = variables["params"]["QuantConv_%d" % i]
    a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
    pk = packing.PackedKernel(leaf["kernel"], QuantDesc(L.Q_DUQ, 4, a, c, 7.0, c), leaf["prune_0"]["mask"])
    g = ops.ConvGeom(hw, hw, cin, C, 3, 3, (1, 1), ((1, 1), (1, 1)))
    if i == 0:
      xi = x.transpose(0, 1).reshape(T * B, hw, hw, cin).contiguous()
      wi = pk.int_weight()
      conn["conv0_direct_ms"] = [_time(lambda: ops.conv_forward(xi, g, wi), args.steps, 2) for _ in range(args.reps)]
    else:
      xi = ops.pack_bits((torch.rand((T * B, hw, hw, cin), device=dev) < 0.1).to(torch.uint8))
      wi = pk.int_weight_mfma(C)
      on_ms, off_ms = [], []
      for _ in range(args.reps):
        on_ms.append(_time(lambda: ops.conv_forward(xi, g, wi, impl="mfma"), args.steps, 2))
        off_ms.append(_time(lambda: ops.conv_forward(xi, g, wi, impl="generic"), args.steps, 2))
      conn["conv%d_mfma_ms" % i], conn["conv%d_direct_ms" % i] = on_ms, off_ms
    hw, cin = hw // 2, C
  del xi

  # conv1's two gradient products alone, on the step's shapes
  geom = ops.ConvGeom(HW // 2, HW // 2, C, C, 3, 3, (1, 1), ((1, 1), (1, 1)))
  x1 = (torch.rand((T * B, HW // 2, HW // 2, C), device=dev) < 0.1).to(torch.float32)
  g1 = torch.randn((T * B, HW // 2, HW // 2, C), device=dev)
  w1 = torch.randn((3, 3, C, C), device=dev)
  splits = ops.conv_grad_splits(geom, T * B)
  kern = {
      "conv1_weight_grad_splits": splits,
      "conv1_weight_grad_1_ms": _time(lambda: ops.conv_weight_grad(x1, g1, geom, splits=1), args.steps, 2),
      "conv1_weight_grad_default_ms": _time(lambda: ops.conv_weight_grad(x1, g1, geom), args.steps, 2),
      "conv1_input_grad_ms": _time(lambda: ops.conv_input_grad(g1, w1, geom), args.steps, 2),
  }
  del x1, g1, w1

  eparams = {k: {kk: ({kkk: t.detach().clone().requires_grad_(True) for kkk, t in vv.items()}
                      if isinstance(vv, dict) else vv.detach().clone().requires_grad_(True))
                 for kk, vv in leaf.items()} for k, leaf in nn.tree_from_numpy(v, dev)["params"].items()}
  opt = torch.optim.Adam([t for _, t in tu._flatten(eparams)], lr=1e-4, eps=1e-8)
  K = (HW >> NB) ** 2 * C
  keep = (torch.rand((T, B, K), device=dev) < 0.9).to(torch.float32)

  def eager_step():
    opt.zero_grad(set_to_none=True)
    _eager_conv_loss(eparams, x, labels, NB, keep).backward()
    opt.step()

  eager_ms = _time(eager_step, args.steps, args.warmup)
  print(json.dumps({"workload": "conv_dense_snn_c3_train_step", "batch": B, "frames": T, "hw": HW,
                    "hip_train_step_ms": round(hip_ms, 3), "hip_memory_before_bytes": hip_peak[0],
                    "hip_memory_after_forward_bytes": hip_peak[0] + hip_kept,
                    "hip_peak_memory_bytes": hip_peak[1],
                    "eager_torch_train_step_ms": round(eager_ms, 3),
                    "speedup_vs_eager": round(eager_ms / hip_ms, 2),
                    "samples_per_s": round(B / hip_ms * 1e3, 1),
                    "step_conv_mfma_on_ms": [round(t, 3) for t in ab[True]],
                    "step_conv_mfma_off_ms": [round(t, 3) for t in ab[False]],
                    **{k: [round(t, 4) for t in val] for k, val in conn.items()},
                    **{k: round(val, 4) for k, val in kern.items()}}))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--conv", action="store_true")
  ap.add_argument("--cext", action="store_true")
  ap.add_argument("--steps", type=int, default=None)
  ap.add_argument("--warmup", type=int, default=None)
  ap.add_argument("--batch", type=int, default=None)
  ap.add_argument("--frames", type=int, default=20)
  ap.add_argument("--hw", type=int, default=128)
  ap.add_argument("--reps", type=int, default=3, help="--conv: timings of each side of the A/B; --cext: timings of each figure")
  ap.add_argument("--neuron", choices=["multi_step_LIF", "plif", "lif"], default=None,
                  help="--conv: the step with this neuron, --reps timings, and its BPTT scan alone")
  ap.add_argument("--lanes", type=int, nargs="*", default=[0],
                  help="--conv --neuron plif|lif: lanes the scan's `splits` aims at (0: the default)")
  ap.add_argument("--window", type=int, default=0,
                  help="the dense step and --conv: train the recording as windows of this many steps")
  ap.add_argument("--remat", type=int, default=0,
                  help="--conv: the step with config.remat = this many steps per chunk")
  args = ap.parse_args()
  if args.remat < 0 or (args.remat and (not args.conv or args.window or args.neuron is not None)):
    ap.error("--remat takes a positive chunk length, for --conv without --window and --neuron")
  if args.window < 0 or (args.window and (args.cext or args.neuron is not None)):
    ap.error("--window takes a positive length, for the dense step and for --conv without --neuron")
  dflt = (5, 2, 2) if args.conv or args.cext else (20, 5, 256)
  args.steps = dflt[0] if args.steps is None else args.steps
  args.warmup = dflt[1] if args.warmup is None else args.warmup
  args.batch = dflt[2] if args.batch is None else args.batch
  if args.cext:
    return cext_main(args)
  if args.conv:
    return conv_main(args)
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, synthetic as syn, train_utils as tu
  dev = torch.device("cuda:0")
  B, T, K, H, N = args.batch, args.frames, 2048, 512, 110
  cfg = syn.make_config(bits=8, prune_percentage=0.5, hidden=H, dropout=0.9)
  cfg.optimizer = "adam"
  model = models.DenseSNN(num_classes=11, config=cfg)
  v = syn.dense_net_variables(K, H, N, True, 0.5)
  variables = nn.tree_from_numpy(v, dev)
  x = torch.from_numpy(syn.poisson_spikes((B, T, K), 0.1, seed=941)).to(dev)
  labels = torch.arange(B, device=dev) % 11
  batch = {"dvs_matrix": x, "label": labels}
  state = tu.create_train_state(variables, cfg, model)
  box = [state]
  if args.window:
    return _window_line("dense_snn_c2_train_windows", args, batch, box, tu)

  def hip_step():
    box[0], _ = tu.train_step(box[0], batch, 0, lambda s: 1e-4, 0.0, 0.0, tu.mse_loss)

  hip_ms, hip_peak = _time_and_peak(hip_step, args.steps, args.warmup)

  # the backward kernels alone, on the step's shapes
  nrn = ops.Neuron(1, 2.0, 1.0, 0.0)
  h1 = torch.randn((T, B, H), device=dev)
  h2 = torch.randn((T, B, N), device=dev)
  gl = torch.randn((B, 11), device=dev)
  x0 = x.transpose(0, 1).reshape(T * B, K).to(torch.float32)
  x1 = (torch.rand((T * B, H), device=dev) < 0.2).to(torch.float32)
  w2 = torch.randn((H, N), device=dev)
  gI1, gI2 = torch.randn((T * B, H), device=dev), torch.randn((T * B, N), device=dev)
  kern = {
      "lif_backward_vote_ms": _time(lambda: ops.lif_backward(h2, nrn, 1, glogits=gl), args.steps, 2),
      "lif_backward_ms": _time(lambda: ops.lif_backward(h1, nrn, 1, gs=h1), args.steps, 2),
      "weight_grad_1_ms": _time(lambda: ops.dense_weight_grad(x0, gI1), args.steps, 2),
      "weight_grad_2_ms": _time(lambda: ops.dense_weight_grad(x1, gI2), args.steps, 2),
      "input_grad_2_ms": _time(lambda: ops.dense_input_grad(gI2, w2, x1), args.steps, 2),
  }

  eparams = {k: {kk: ({kkk: t.detach().clone().requires_grad_(True) for kkk, t in vv.items()}
                      if isinstance(vv, dict) else vv.detach().clone().requires_grad_(True))
                 for kk, vv in leaf.items()} for k, leaf in nn.tree_from_numpy(v, dev)["params"].items()}
  flat = [t for _, t in tu._flatten(eparams)]
  opt = torch.optim.Adam(flat, lr=1e-4, eps=1e-8)

  def eager_step():
    opt.zero_grad(set_to_none=True)
    _eager_loss(eparams, x, labels).backward()
    opt.step()

  eager_ms = _time(eager_step, args.steps, args.warmup)
  print(json.dumps({"workload": "dense_snn_c2_train_step", "batch": B, "frames": T,
                    "hip_train_step_ms": round(hip_ms, 3), "hip_memory_before_bytes": hip_peak[0],
                    "hip_peak_memory_bytes": hip_peak[1],
                    "eager_torch_train_step_ms": round(eager_ms, 3),
                    "speedup_vs_eager": round(eager_ms / hip_ms, 2),
                    "samples_per_s": round(B / hip_ms * 1e3, 1),
                    **{k: round(val, 4) for k, val in kern.items()}}))


if __name__ == "__main__":
  main()
