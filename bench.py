"""bench.py -- throughput of the quantized / pruned SNN forward pass on MI355X.

Workload (BASELINE.json configs[2], "C3"): 3 x (QuantConv 3x3 + BatchNorm + LIF +
2x2 max-pool) -> flatten -> QuantDense(110) + LIF -> vote, DVS128-shaped input
[B, T=20, 128, 128, 2], 4-bit DuQ weights, 90 % magnitude-pruned, B = 1024 per
GPU.  One "step" = one model.apply() on one resident batch (uint8 event frames
already in HBM) + the all-gather of the logits.  Weak scaling: every rank owns
its own B samples; value = N * B * K / max-over-ranks time.

  python bench.py --gpus 1 --steps 5 --warmup 2
  python bench.py --gpus 8                   (spawns its own 8 rank processes)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and
prints the headline (`value`, `ms_per_step`, ...); `--dump-outputs DIR` also writes
the logits of the last timed step to DIR/logits.npy.  Everything else the benchmark
measures runs only under `--full`: `roofline` (dominant kernel, HIP events on a second
pass of the same steps, HBM traffic counted by rocprofv3 child runs), the other input
formats and BASELINE configurations (`legs`), the host-fed, captured and general
cases, the fallback / device-status checks and, at N = 1, `cpu_baseline` (the CPU
oracle in its reference-literal float mode on a bounded sample, host cores).

  python bench.py --gpus 1 --steps 20 --warmup 5 --full

Other BASELINE configs: C5 (mixed 2/4-bit, 95 % pruned, T = 50, 512 samples per GPU)
  python bench.py --frames 50 --batch 512 --layer-bits 2,4,2,4 --prune 0.95 --classes 10
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

# dense peaks, MI355X_MICROARCH.md: int8 MFMA 2x the ~2.5 PF bf16 rate; block-scaled
# fp6/fp4 MFMA ~10 PF; HBM3E 8 TB/s
F32_MFMA_PEAK_TOPS = 157.3       # v_mfma_f32_32x32x2_f32: 78.6 T fma/s (MI355X_MICROARCH.md)
INT8_MFMA_PEAK_TOPS = 5000.0
FP6_MFMA_PEAK_TOPS = 10000.0
HBM_PEAK_GBS = 8000.0
# one wave64 VALU instruction per SIMD every 2 cycles (32 lanes per cycle, MI355X_MICROARCH.md "issues
# each VALU instruction over 2 cycles"; tools/ubench/pk_f32_rate.hip measures 2.3-2.6 for add / mul /
# fma with two or more waves, 4.2 for compare / select): 256 CUs x 4 SIMDs x 2.4 GHz / 2.  Rounds 3-5
# priced this at 4 cycles, which overstated `valu_issue.frac` two-fold; `measured_mix_frac` (the
# tile's own instruction mix timed alone) is the figure to read.
VALU_PEAK_GINSTR = 256 * 4 * 2.4 / 2.0   # G wave-instructions / s (x 64 lanes each)
# HBM bytes per launch measured with rocprofv3 --pmc (separate passes of this same
# command: tools/pmc_profile.sh; FETCH_SIZE x 2 on gfx950 + WRITE_SIZE), committed
PMC_TRAFFIC = [os.path.join(ROOT, "profiles", n) for n in ("r06_pmc_traffic.json", "r06_pmc_f32_traffic.json", "r06_pmc_u8_traffic.json",
                                                           "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json",
                                                           "r02_pmc_traffic.json",
                                                           "r01_pmc_traffic.json")]
# per-kernel PMC counters of the same command (tools/pmc_profile.sh), committed: SQ_INSTS_VALU per
# launch gives the vector instructions per neuron update of the conv kernels
PMC_SUMMARY = [os.path.join(ROOT, "profiles", n) for n in ("r06_pmc_summary.json", "r05_pmc_summary.json", "r04_pmc_summary.json", "r03_pmc_summary.json",
                                                           "r02_pmc_summary.json")]
# int-vs-float deviation of the numeric contract (tools/int_vs_float.py, CPU), committed
PARITY_VS_FLOAT = next((p for p in (os.path.join(ROOT, "profiles", n) for n in
                                    ("r05_int_vs_float.json", "r04_int_vs_float.json", "r02_int_vs_float.json"))
                        if os.path.exists(p)), os.path.join(ROOT, "profiles", "r02_int_vs_float.json"))
# --dump-outputs writes at most this many bytes
DUMP_LIMIT = 64 << 20


def parse(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--gpus", type=int, default=1)
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=5,
                  help="untimed steps first (the first launches of a process run 1-2 %% slower: "
                       "85.8 k samples/s after 10 warm-up steps, 84.9 k after 2)")
  ap.add_argument("--batch", type=int, default=1024, help="samples per GPU")
  ap.add_argument("--frames", type=int, default=20)
  ap.add_argument("--bits", type=int, default=4)
  ap.add_argument("--layer-bits", type=str, default=None,
                  help="per-layer bit widths conv0,conv1,conv2,dense (mixed precision, "
                       "BASELINE config C5: 2,4,2,4); overrides --bits")
  ap.add_argument("--classes", type=int, default=11, help="read-out = 10 neurons per class")
  ap.add_argument("--prune", type=float, default=0.9)
  ap.add_argument("--lam", type=float, default=0.1,
                  help="Poisson rate of the synthetic events; spikes are (Poisson(lam) > 0)")
  ap.add_argument("--counts", action="store_true",
                  help="event COUNT frames, Poisson(lam) per pixel and polarity as the reference's "
                       "preprocessing produces them (input_pipeline.py:195-218), instead of binary")
  ap.add_argument("--model", choices=("c3", "cextnet", "dense"), default="c3",
                  help="c3: BASELINE config 3 (the headline workload); cextnet: the reference's "
                       "full TCJA model (5 conv blocks + 2 gates + 2 dense), same input")
  ap.add_argument("--input", choices=("u8", "f32", "ev1", "ev4", "bits"), default=None,
                  help="format of the resident input batch.  ev1 (default for binary frames): the "
                       "bit-packed wire format of include/snnqp.h, 81 920 B per sample -- what the "
                       "host feed can deliver (uint8 frames need 50 GB/s per GPU at this rate) and "
                       "what the event layer stages directly; u8 (default with --counts and for "
                       "--model dense): uint8 frames, 655 360 B per sample; f32: the float32 frames / "
                       "rows the reference's pipeline hands over (flax_qconv.py:101, flax_qdense.py:67), "
                       "staged in place by the first kernel and checked on the device; ev4: nibble-packed "
                       "counts <= 15 (327 680 B)")
  ap.add_argument("--feed", choices=("resident", "host"), default="resident",
                  help="resident: the batch is in HBM before the timed region (the contract's "
                       "`value`).  host: every step's batch comes from page-locked host memory "
                       "through feed.DeviceFeeder (two batches prefetched on a copy stream, as "
                       "examples/input_pipeline.py:17-27): the PCIe-inclusive rate; the line is "
                       "marked `pcie_inclusive`")
  ap.add_argument("--no-fed-leg", action="store_true",
                  help="skip the short host-fed leg (ev1 frames through the feeder) that the "
                       "--full run appends to the line as `fed`")
  ap.add_argument("--no-legs", action="store_true",
                  help="skip the other BASELINE configurations (C2, C5, the float32 formats) that the "
                       "--full run times after the headline and reports as `legs`")
  ap.add_argument("--random-bn", action="store_true",
                  help="BatchNorm with random running statistics / scale / bias (a trained "
                       "model) instead of the freshly initialised one (mean 0, var 1, scale 1, "
                       "bias 0) of a random-init model: the kernels then run all three "
                       "BatchNorm instructions instead of the multiply alone")
  ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                  help="weak: --batch samples per GPU whatever N is (the default, BASELINE C3 -> C4). "
                       "strong: --global-batch samples in total, split over the N GPUs (C4's 8192)")
  ap.add_argument("--global-batch", type=int, default=8192, help="total samples under --scaling strong")
  ap.add_argument("--cpu-samples", type=int, default=8)
  ap.add_argument("--no-cpu-baseline", action="store_true")
  ap.add_argument("--graph", action="store_true",
                  help="capture model.apply into a hipGraph after the warm-up and replay it in the "
                       "timed steps (for launch-bound configurations such as --model dense; the "
                       "per-kernel times then come from the eager warm-up steps)")
  ap.add_argument("--detail", type=str, default=None,
                  help="where the full record goes (per-kernel blocks, per-rank accounts, every leg's "
                       "rooflines ...): default bench_detail.json beside bench.py, and a copy under "
                       "gpurun_out/ when that directory exists.  stdout carries ONE compact line (< 6 KB)")
  ap.add_argument("--full-line", action="store_true",
                  help="print the full record on stdout instead of the compact line (tools/*.sh)")
  ap.add_argument("--no-live-traffic", action="store_true",
                  help="skip the two rocprofv3 --pmc child runs (FETCH_SIZE, WRITE_SIZE: one step each) that the "
                       "--full headline run uses to MEASURE `roofline.traffic`; the committed profiles/ "
                       "figure is reported instead, labelled as such")
  ap.add_argument("--allow-diag", action="store_true",
                  help="accept a diagnostic libsnnqp (SNNQP_DIAG_LIB); the line is marked")
  ap.add_argument("--full", action="store_true",
                  help="besides the headline, measure and check everything else: per-kernel rooflines "
                       "(a second, event-carrying pass of the steps), live HBM traffic, the u8 / captured / "
                       "host-fed / general cases, the other BASELINE configurations, fallback counters, the "
                       "device status word and the CPU baseline (the --no-* options above trim this run)")
  ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                  help="after the timed steps, write what the last one returned (the gathered logits) "
                       "to DIR/logits.npy (float32; a fixed, seeded sample of rows past %d MB)"
                  % (DUMP_LIMIT >> 20))
  # test plumbing: the same step / fence / all-reduce code on CPU tensors over gloo with a
  # stand-in for model.apply (tests/test_host_cpu.py); never a measurement
  ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help=argparse.SUPPRESS)
  ap.add_argument("--stand-in", action="store_true", help=argparse.SUPPRESS)
  ap.add_argument("--single-rank-collective", action="store_true",
                  help="with --gpus 1: create the RCCL process group anyway, so that the step's "
                       "all-gather, the barrier and the all-reduce of the timing run through RCCL "
                       "on the one GPU (rehearsal of the multi-GPU path; the line says so)")
  args = ap.parse_args(argv)
  if args.input is None:
    args.input = "u8" if (args.counts or args.model == "dense" or args.stand_in) else "ev1"
  if args.input == "bits" and args.model != "dense":
    ap.error("--input bits (bit-packed [B, T, K] rows, ops.PackedSpikes) is for --model dense")
  if args.input == "ev1" and args.counts:
    ap.error("--input ev1 holds binary frames; count frames travel as ev4 or u8")
  if args.layer_bits:
    args.layer_bits = [int(b) for b in args.layer_bits.split(",")]
    if len(args.layer_bits) != 4 or args.model != "c3":
      ap.error("--layer-bits takes four widths (conv0,conv1,conv2,dense) of the c3 topology")
  return args


def layer_bits(args):
  return list(args.layer_bits) if args.layer_bits else [args.bits] * 4


def issued_dtype(args, lb):
  """The operand formats of the instruction the dominant kernel issues (not a precision claim:
  every sum is an exact integer)."""
  if args.bits < 0 and not args.layer_bits:        # unquantised kernels (config C1): the float32 chain
    return "f32*f32->f32 (fmaf chain on the f32 MFMA)"
  if args.model == "dense":
    return "int8*int8->int32"
  conv = [b for b in lb[1:3]]
  if all(0 < b <= 4 for b in conv):
    return "fp6*fp4->f32 (integer-exact)"
  if all(not (0 < b <= 4) for b in conv):
    return "int8*int8->int32"
  return "fp6*fp4->f32 (integer-exact) / int8*int8->int32"


def metric_name(args):
  if args.model == "dense":
    how = ("f32 weights" if args.bits < 0 else "%d-bit" % args.bits) + "/" + \
        ("unpruned" if args.prune < 0 else "%.4g%%-pruned" % (args.prune * 100))
    return "samples/sec/node (2-layer qdense 2048-512-%d, T=%d, %s)" % (args.classes * 10, args.frames, how)
  lb = layer_bits(args)
  bits = "%d-bit" % lb[0] if len(set(lb)) == 1 else "mixed %s-bit" % "/".join(
      str(b) for b in sorted(set(lb)))
  return "samples/sec/node (DVS128 T=%d, %s/%.4g%%-pruned)" % (args.frames, bits, args.prune * 100)


# ---------------------------------------------------------------------------
# `python bench.py --gpus N` without a launcher: this process starts the N ranks
# ---------------------------------------------------------------------------


def launch_ranks(args, argv):
  """Spawns one fresh process per rank (before anything here touched a GPU), relays rank
  0's JSON line and exits non-zero if any rank failed.  Equivalent to
  `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <argv>`."""
  with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
  n = args.gpus
  base = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
              MASTER_PORT=str(port))
  # RCCL shares device buffers between the rank processes of a node through IPC handles; this
  # image's host driver only supports the dmabuf form, and with the legacy form selected
  # hipIpcGetMemHandle fails with "invalid argument" inside the first collective.  The image
  # exports the variable already (see the task environment notes); kept here so that ranks
  # started from a scrubbed environment get it too.  It changes nothing on one GPU.
  base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
  import tempfile
  procs = []
  with tempfile.TemporaryFile() as out0:
    for r in range(n):
      env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
      procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv),
                                    env=env, stdout=out0 if r == 0 else subprocess.DEVNULL,
                                    cwd=os.getcwd()))
    deadline = time.time() + float(os.environ.get("SNNQP_BENCH_LAUNCH_TIMEOUT", "1500"))
    failed = None
    while failed is None and any(p.poll() is None for p in procs):
      for r, p in enumerate(procs):
        if p.poll() not in (None, 0):
          failed = (r, p.returncode)
      if time.time() > deadline:
        failed = (-1, 124)
      time.sleep(0.1)
    for r, p in enumerate(procs):
      if failed is None and p.returncode != 0:
        failed = (r, p.returncode)
    if failed is not None:
      for p in procs:                    # the exact children started above, nothing else
        if p.poll() is None:
          p.kill()
      for p in procs:
        try:
          p.wait(timeout=30)
        except subprocess.TimeoutExpired:
          pass
      print("bench.py: rank %d failed with exit code %d" % failed, file=sys.stderr)
      return failed[1] if failed[1] > 0 else 1
    out0.seek(0)
    sys.stdout.write(out0.read().decode())
    sys.stdout.flush()
  return 0


def build_model(args, dev):
  """(model, variables on `dev`, variables as numpy) of the configuration `args` names."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  cfg = syn.make_config(bits=args.bits, prune_percentage=args.prune)
  if args.layer_bits:
    cfg.quant.layer_bits = tuple(args.layer_bits)
  if args.model == "cextnet":
    model = models.CextNet(num_classes=args.classes, config=cfg)
    variables_np = syn.cextnet_variables(prune_p=args.prune, out=args.classes * 10,
                                         random_bn=args.random_bn)
  elif args.model == "dense":     # BASELINE config C2: the head of CextNet on its own
    cfg = syn.make_config(bits=args.bits, prune_percentage=args.prune, hidden=512)
    model = models.DenseSNN(num_classes=args.classes, config=cfg)
    variables_np = syn.dense_net_variables(2048, 512, args.classes * 10, True, args.prune)
  else:
    model = models.ConvDenseSNN(num_classes=args.classes, config=cfg)
    variables_np = syn.conv_net_variables(prune_p=args.prune, out=args.classes * 10,
                                          random_bn=args.random_bn)
  return model, nn.tree_from_numpy(variables_np, dev), variables_np


def build_input(args, dev, rank, B, T, hw, ops):
  """(the resident batch in the format --input names, the same frames as uint8 | None)."""
  import numpy as np
  import torch
  gen = torch.Generator(device=dev)
  gen.manual_seed(8627169 + rank)
  p_spike = 1.0 - float(np.exp(-args.lam))       # P(Poisson(lam) > 0)
  if args.model == "dense":                      # [B, T, 2048] binary spikes
    x = (torch.rand((B, T, 2048), device=dev, generator=gen) < p_spike).to(torch.uint8)
  elif args.counts:
    x = torch.poisson(torch.full((B, T, hw, hw, 2), float(args.lam), device=dev),
                      generator=gen).clamp_(max=255).to(torch.uint8)
  else:
    x = (torch.rand((B, T, hw, hw, 2), device=dev, generator=gen) < p_spike).to(torch.uint8)
  frames_u8 = x if (args.model != "dense" and not args.stand_in) else None
  if args.input == "bits":
    x = ops.pack_bits(x)
    torch.cuda.synchronize()
  elif args.input == "f32":
    x = x.to(torch.float32)
  elif args.input in ("ev1", "ev4") and ops is not None and args.model != "dense":
    from snnquantprune_amd import _lib as L_
    x = ops.pack_frames(x, L_.EV1 if args.input == "ev1" else L_.EV4)
    torch.cuda.synchronize()
  return x, frames_u8


def config_leg(base_args, overrides, dev, steps, warmup, capture):
  """Another BASELINE configuration timed inside the default run (one GPU): the model and a
  resident batch of its own, `warmup` + `steps` eager steps, optionally the same steps as a
  hipGraph (nn.capture), then a pass with a HIP event pair around every launch for its rooflines."""
  import copy
  import torch
  from snnquantprune_amd import linen as nn, ops
  a = copy.copy(base_args)
  for k, v in overrides.items():
    setattr(a, k, v)
  B, T = a.batch, a.frames
  model, variables, _ = build_model(a, dev)
  x, _ = build_input(a, dev, 0, B, T, 128, ops)
  ops.reset_count_hints(dev)        # another data stream: what the event layer saw in the last leg does not apply

  def step():
    ops.forget_inputs()
    return model.apply(variables, x, trgt=None, train=False, rng=None)[0]

  def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
      fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n
  for _ in range(max(2, warmup)):
    step()
  dt = timed(step, steps)
  leg = {"metric": metric_name(a), "dtype": issued_dtype(a, layer_bits(a)),
         "config": {"batch_per_gpu": B, "frames": T, "bits": "/".join(str(b) for b in layer_bits(a)),
                    "prune": a.prune, "classes": a.classes, "input": a.input, "model": a.model},
         "steps": steps, "ms_per_step": dt * 1e3, "samples_per_s": B / dt,
         "launch": "eager (one C call per block from Python)"}
  if capture:
    cap = nn.capture(model, variables, x, trgt=None, train=False, rng=None)
    for _ in range(3):
      cap()
    dtc = timed(cap, steps)
    leg["captured"] = {"api": "nn.capture (one hipGraph launch per step)", "steps": steps,
                       "ms_per_step": dtc * 1e3, "samples_per_s": B / dtc}
    del cap
  ops.profile_start()
  for _ in range(min(steps, 50)):
    step()
  prof = ops.profile_stop()
  leg.update(rooflines_of(a, prof, B, T, layer_bits(a), dict(ops.PROFILE_NOTES)))
  leg["fallbacks"] = ops.fallback_counts()
  leg["device_status"] = ops.device_status()
  return leg


def dump_outputs(path, arrays):
  """Writes {name: tensor} as path/<name>.npy in float32 (float64 stays float64).  Past DUMP_LIMIT
  bytes in all, each array keeps a fixed, seeded sample of its rows, in row order."""
  import numpy as np
  host = {}
  for name, t in arrays.items():
    a = t.detach().cpu().numpy()
    host[name] = a if a.dtype == np.float64 else a.astype(np.float32)
  total = sum(a.nbytes for a in host.values())
  os.makedirs(path, exist_ok=True)
  for name, a in host.items():
    if total > DUMP_LIMIT:
      keep = max(1, a.shape[0] * DUMP_LIMIT // total)
      a = a[np.sort(np.random.default_rng(20240611).choice(a.shape[0], keep, replace=False))]
    np.save(os.path.join(path, name + ".npy"), a)


def make_feeder(x_dev, dev, nbatches=4):
  """Host side of `--feed host`: `nbatches` distinct batches in page-locked host memory (the
  resident batch and rolled copies of it: same statistics, different bytes), cycled through
  feed.DeviceFeeder -- what a loader that decodes into pinned buffers would hand over."""
  import itertools
  import torch
  from snnquantprune_amd import feed, ops
  host = []
  for k in range(nbatches):
    if isinstance(x_dev, ops.PackedFrames):
      d = torch.roll(x_dev.data, k, 0).cpu().pin_memory()
      host.append({"dvs_matrix": ops.PackedFrames(d, x_dev.H, x_dev.W, x_dev.fmt)})
    else:
      host.append({"dvs_matrix": torch.roll(x_dev, k, 0).cpu().pin_memory()})
  return feed.DeviceFeeder(itertools.cycle(host), dev, 2)


def fed_leg(args, frames_u8, apply_fn, parallel, fence, dev, steps, warmup):
  """The PCIe-inclusive figure next to the resident one: the same model on bit-packed (EV1)
  frames that arrive from page-locked host memory, two batches prefetched (feed.py), timed
  the same way.  Binary workloads only (EV1 holds no counts)."""
  import torch
  from snnquantprune_amd import _lib as L_, ops
  pf = ops.pack_frames(frames_u8, L_.EV1)
  feeder = make_feeder(pf, dev)

  def step():
    return parallel.all_gather_rows(apply_fn(next(feeder)["dvs_matrix"]))
  for _ in range(max(1, warmup)):
    step()
  fence()
  b0 = feeder.bytes_copied
  t0 = time.perf_counter()
  for _ in range(steps):
    step()
  fence()
  dt = time.perf_counter() - t0
  nbytes = feeder.bytes_copied - b0
  B = frames_u8.shape[0]
  return {"format": "ev1 (bit-packed binary frames, include/snnqp.h)", "steps": steps,
          "samples_per_s_per_gpu": B * steps / dt, "ms_per_step": dt / steps * 1e3,
          "bytes_per_sample": pf.data[0].numel() * 4, "h2d_GBps": nbytes / dt / 1e9,
          "prefetch_depth": 2, "source": "page-locked host memory, hipMemcpyAsync on a copy stream"}


def general_leg(args, model, dev, B, T, parallel, fence, steps, warmup):
  """The same C3 topology WITHOUT the three specialisations the headline takes: event COUNT
  frames (Poisson(lam) per pixel and polarity, what examples/input_pipeline.py:195-218 produces)
  instead of binary ones, a trained-looking BatchNorm (random running statistics, scale and
  bias: all three instructions of the epilogue) instead of the freshly initialised one, and
  every batch arriving from page-locked host memory in the nibble-packed wire format (EV4)
  instead of resident in HBM.  Timed like the headline, with its own per-kernel HIP events."""
  import numpy as np
  import torch
  from snnquantprune_amd import _lib as L_, linen as nn, ops, synthetic as syn
  vnp = syn.conv_net_variables(prune_p=args.prune, out=args.classes * 10, random_bn=True)
  variables = nn.tree_from_numpy(vnp, dev)
  gen = torch.Generator(device=dev)
  gen.manual_seed(8627170)
  x = torch.poisson(torch.full((B, T, 128, 128, 2), float(args.lam), device=dev),
                    generator=gen).clamp_(max=15).to(torch.uint8)
  feeder = make_feeder(ops.pack_frames(x, L_.EV4), dev)
  del x
  ops.reset_count_hints(dev)        # (a stream of count frames begins: the hint settles within two batches)

  def step():
    ops.forget_inputs()
    (logits, _) = model.apply(variables, next(feeder)["dvs_matrix"], trgt=None, train=False, rng=None)
    return parallel.all_gather_rows(logits)
  for _ in range(max(3, warmup)):          # the count hint settles within two batches
    step()
  fence()
  ops.profile_start()
  t0 = time.perf_counter()
  for _ in range(steps):
    step()
  fence()
  dt = time.perf_counter() - t0
  prof = ops.profile_stop()
  return {"what": "event-count frames (Poisson(%g), EV4 wire format) fed from host memory, BatchNorm "
                  "with random running statistics / scale / bias; same topology, bits and pruning" % args.lam,
          "steps": steps, "ms_per_step": dt / steps * 1e3, "samples_per_s_per_gpu": B * steps / dt,
          "kernels": {tag: {"launches": n, "avg_ms": ms / max(n, 1)} for tag, (n, ms) in prof.items()},
          "dequant_form": {t: v.get("dequant") for t, v in ops.PROFILE_NOTES.items()}}


def cpu_baseline(args, variables_np):
  """Reference-literal float mode of the CPU oracle (dense float32 fake-quantised
  weights, BLAS matmul on im2col, float32 spike tensors between layers, T
  sequential LIF steps) on a bounded sample of the same workload."""
  import numpy as np
  from oracle import snn_oracle as o
  from snnquantprune_amd import synthetic as syn
  from tests.helpers import bn_of, qweight_of
  p = variables_np["params"]
  lb = layer_bits(args)
  cq = [qweight_of(o, p["QuantConv_%d" % i], lb[i]) for i in range(3)]
  bns = [bn_of(variables_np, i) for i in range(3)]
  dq = qweight_of(o, p["QuantDense_0"], lb[3])
  n = max(1, args.cpu_samples)
  x = syn.poisson_spikes((n, args.frames, 128, 128, 2), args.lam, seed=4242).astype(np.float32)
  o.conv3_dense_forward(x[:1, :2], cq, bns, dq, mode="float")      # warm-up, discarded
  cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
  cpu = "unknown"
  try:
    with open("/proc/cpuinfo") as f:
      for line in f:
        if line.startswith("model name"):
          cpu = line.split(":", 1)[1].strip()
          break
  except OSError:
    pass

  def timed(xs):
    t0 = time.perf_counter()
    o.conv3_dense_forward(xs, cq, bns, dq, mode="float")
    return time.perf_counter() - t0

  # numpy/BLAS thread count: all host cores is not the fastest setting for these matrix
  # sizes, so the sample is timed at several and the best is the baseline (SURVEY 8d asks
  # for n = 1 and n = all cores; both are in `by_threads`)
  by_threads = {}
  try:
    from threadpoolctl import threadpool_limits
    for nthreads in sorted({1, 8, 32, int(cores)}):
      if nthreads > cores:
        continue
      with threadpool_limits(limits=nthreads):
        k = n if nthreads > 1 else min(n, 2)
        dt = timed(x[:k])
      by_threads[nthreads] = {"value": k / dt, "samples": k, "seconds": round(dt, 2)}
  except ImportError:
    dt = timed(x)
    by_threads[int(cores)] = {"value": n / dt, "samples": n, "seconds": round(dt, 2)}
  best = max(by_threads, key=lambda t: by_threads[t]["value"])
  out = {"value": by_threads[best]["value"], "unit": "samples/s", "cores": int(best),
         "kind": "port", "cpu": cpu, "host_cores": int(cores),
         "sample": "%d samples of the same workload (T=%d, 128x128x2), oracle float mode "
                   "(dense float32 fake-quantised weights, BLAS matmul on im2col), best of the "
                   "BLAS thread counts tried" % (by_threads[best]["samples"], args.frames),
         "by_threads": {str(k): v for k, v in sorted(by_threads.items())}}
  # the batch is embarrassingly parallel: W single-threaded worker processes, one slice of
  # samples each (fresh interpreters that never touch the GPU), W = the box's CPU share
  try:
    import tempfile
    W = int(min(16, cores))
    per = max(2, int(round(12 * 20 / max(args.frames, 1))))     # ~6-8 s of CPU work per worker
    payload = {"bits": np.int32(args.bits), "layer_bits": np.asarray(lb, np.int32),
               "x": syn.poisson_spikes((W * per, args.frames, 128, 128, 2), args.lam,
                                       seed=4243).astype(np.uint8)}
    for name, leaf in [("conv%d" % i, p["QuantConv_%d" % i]) for i in range(3)] + \
                      [("dense", p["QuantDense_0"])]:
      payload[name + "_kernel"] = leaf["kernel"]
      payload[name + "_a"] = np.float32(leaf["DuQ_0"]["a"][0])
      payload[name + "_c"] = np.float32(leaf["DuQ_0"]["c"][0])
      if "prune_0" in leaf:
        payload[name + "_mask"] = leaf["prune_0"]["mask"]
    for i in range(3):
      for k, v in bn_of(variables_np, i).items():
        payload["bn%d_%s" % (i, k)] = v
    with tempfile.TemporaryDirectory() as tmp:
      path = os.path.join(tmp, "payload.npz")
      np.savez(path, **payload)
      env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
      procs = [subprocess.Popen([sys.executable, "-m", "oracle.cpu_baseline", path,
                                 str(i * per), str((i + 1) * per)], stdout=subprocess.PIPE,
                                env=env, cwd=ROOT) for i in range(W)]
      res = [json.loads(pr.communicate(timeout=300)[0].decode().strip().splitlines()[-1])
             for pr in procs]
    secs = max(r["seconds"] for r in res)
    nproc = sum(r["samples"] for r in res)
    out["by_processes"] = {"workers": W, "samples": nproc, "seconds": round(secs, 2),
                           "value": nproc / secs}
    if nproc / secs > out["value"]:
      out.update(value=nproc / secs, cores=W,
                 sample="%d samples of the same workload (T=%d, 128x128x2), oracle float mode, "
                        "%d single-threaded worker processes" % (nproc, args.frames, W))
  except Exception as e:          # no subprocesses on this box: keep the in-process figure
    out["by_processes"] = {"value": None, "note": "not measured: %s" % type(e).__name__}
  return out


def main(argv=None):
  argv = sys.argv[1:] if argv is None else list(argv)
  args = parse(argv)
  if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
    # no launcher around us: become one (nothing in this process has touched a GPU yet)
    sys.exit(launch_ranks(args, argv))

  # (before torch loads the runtime: RCCL shares buffers between the ranks of a node through dmabuf IPC
  # handles on this image, see launch_ranks -- ranks started by an external launcher get it too)
  os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
  import numpy as np
  import torch
  from snnquantprune_amd import parallel

  gpu = args.backend == "nccl"
  rank, world, local = parallel.init_from_env(args.backend, args.single_rank_collective)
  collective = world > 1 or args.single_rank_collective
  if world != args.gpus:
    raise SystemExit("WORLD_SIZE %d != --gpus %d" % (world, args.gpus))
  if gpu:
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
  else:
    assert args.stand_in, "the gloo backend is test plumbing (--stand-in) only"
    dev = torch.device("cpu")

  if args.scaling == "strong":
    if args.global_batch % world:
      raise SystemExit("--global-batch %d is not divisible by %d ranks" % (args.global_batch, world))
    args.batch = args.global_batch // world
  B, T = args.batch, args.frames
  # who is here: every rank says which device it drives (stderr), rank 0 collects the list so
  # that a scaling record shows the collective really spanned N distinct GPUs
  ident = {"rank": rank, "local_rank": local, "pid": os.getpid(), "backend": args.backend}
  if gpu:
    p = torch.cuda.get_device_properties(local)
    ident.update(device=local, name=p.name,
                 pci="%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), getattr(p, "pci_bus_id", 0),
                                         getattr(p, "pci_device_id", 0)),
                 uuid=str(getattr(p, "uuid", "")))
    try:
      ident["rccl"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception:
      ident["rccl"] = "unknown"
  print("bench.py rank %s" % json.dumps(ident), file=sys.stderr, flush=True)
  if collective:
    ids = [None] * world
    torch.distributed.all_gather_object(ids, ident)
  else:
    ids = [ident]
  lb = layer_bits(args)
  build_flags = ""
  if args.stand_in:
    # stand-in for model.apply: a per-sample function of the input, so that the gathered
    # logits identify every rank's shard (tests/test_host_cpu.py)
    ops = None
    variables_np = None

    def apply_fn(xb):
      f = xb.reshape(xb.shape[0], -1).to(torch.float32)
      return torch.stack([f.sum(1) * (k + 1) for k in range(args.classes)], 1)
    hw = 4
  else:
    from snnquantprune_amd import _lib, linen as nn
    from snnquantprune_amd import ops
    build_flags = _lib.build_flags()
    if not args.allow_diag:
      _lib.require_product_build()
    model, variables, variables_np = build_model(args, dev)

    def apply_fn(xb):
      (logits, _) = model.apply(variables, xb, trgt=None, train=False, rng=None)
      return logits
    hw = 128

  # synthetic Poisson-spike DVS frames, resident in HBM before the timed region
  p_spike = 1.0 - float(np.exp(-args.lam))       # P(Poisson(lam) > 0)
  x, frames_u8 = build_input(args, dev, rank, B, T, hw, ops)

  feeder = None
  if args.feed == "host":
    assert gpu and ops is not None and args.model != "dense", "--feed host needs a GPU and event frames"
    feeder = make_feeder(x, dev)

  def step():
    if ops is not None:
      ops.forget_inputs()     # a new batch: whatever is cached about the last one is dropped
    xb = next(feeder)["dvs_matrix"] if feeder is not None else x
    return parallel.all_gather_rows(apply_fn(xb))

  def fence():
    if collective:
      if gpu:
        torch.distributed.barrier(device_ids=[local])
      else:
        torch.distributed.barrier()
    if gpu:
      torch.cuda.synchronize()

  # a full collection over everything imported and built so far, then park those objects in
  # the permanent generation: the interpreter's next full collection otherwise lands in one of
  # the first steps and stalls the launch thread for tens of milliseconds (38 ms measured on
  # a cold box, in the third step)
  import gc
  gc.collect()
  gc.freeze()
  # The per-kernel HIP events stay OUT of the timed steps (they cost 0.8 % there, round 4): the
  # warm-up creates them once (the first timing event of a process costs tens of milliseconds on
  # a cold box), the timed region runs bare, and a second pass of the same K steps right after it
  # carries the events the rooflines are computed from (--full).
  full = ops is not None and args.full
  if full:
    ops.profile_start()
  out = None
  for i in range(args.warmup):
    out = step()
  fence()
  if full:
    ops.profile_stop()
  eager_step = step
  if args.graph:
    assert gpu and ops is not None and args.warmup > 0, "--graph needs a GPU and a warm-up step"
    # the product API: nn.capture records model.apply once (linen.CapturedApply)
    captured = nn.capture(model, variables, x, trgt=None, train=False, rng=None)

    def step():                          # noqa: F811  (the timed steps replay the graph)
      return parallel.all_gather_rows(captured()[0])
    out = step()
    fence()
  fed_b0 = feeder.bytes_copied if feeder is not None else 0
  t0 = time.perf_counter()
  trace = os.environ.get("SNNQP_BENCH_TRACE")      # diagnostic: host time of every step's enqueue
  marks = []
  for _ in range(args.steps):
    out = step()
    if trace:
      marks.append(time.perf_counter() - t0)
  fence()
  dt = time.perf_counter() - t0
  fed_bytes = 0
  if feeder is not None:
    fed_bytes = feeder.bytes_copied - fed_b0
  if trace and rank == 0:
    print("enqueue done at (ms):", [round(m * 1e3, 2) for m in marks], "all done", round(dt * 1e3, 2),
          file=sys.stderr)
  if args.dump_outputs and rank == 0:
    dump_outputs(args.dump_outputs, {"logits": out})
  # {tag: (launches, total ms)}: a second pass of the same steps, launched eagerly with a HIP event
  # pair around every block's launch on its stream
  prof = {}
  if full:
    ops.profile_start()
    for _ in range(args.steps):
      eager_step()
    fence()
    prof = ops.profile_stop()
  assert out.shape == (world * B, args.classes), out.shape
  if args.stand_in:
    # every rank's rows arrived, in rank order: row r*B of the gathered logits is rank r's first
    # sample (seeded 8627169 + r)
    for r in range(world):
      g = torch.Generator(device=dev)
      g.manual_seed(8627169 + r)
      xr = (torch.rand((B, T, hw, hw, 2), device=dev, generator=g) < p_spike).to(torch.uint8)
      assert torch.equal(out[r * B:(r + 1) * B], apply_fn(xr)), "gathered rows of rank %d" % r

  # every rank's own account of the timed region: seconds, per-layer launch times (HIP events on
  # its own stream) and fallback counters -- a straggler or a rank that fell off the fast kernels
  # shows in rank 0's line, not only in the maximum
  mine = {"rank": rank, "seconds": dt,
          "kernels": {tag: round(ms / max(n, 1), 5) for tag, (n, ms) in (prof or {}).items()}}
  if full:
    mine["fallbacks"] = dict(ops.fallback_counts(), **ops.workqueue_stats())
    mine["device_status"] = ops.device_status(dev)
  if collective:
    rank_detail = [None] * world
    torch.distributed.all_gather_object(rank_detail, mine)
  else:
    rank_detail = [mine]
  tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
  rank_dt = [dt]
  if collective:
    every = torch.zeros(world, device=dev, dtype=torch.float64)
    torch.distributed.all_gather_into_tensor(every, tmax)
    rank_dt = [float(v) for v in every.tolist()]
    torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
  dt = float(tmax.item())

  # the same steps on resident uint8 frames (the format of rounds 1 and 2's headline), when the
  # line itself is on bit-packed frames
  alt = None
  if (gpu and full and frames_u8 is not None and args.input == "ev1"
      and args.feed == "resident" and not args.no_fed_leg and not args.graph):
    for _ in range(2):
      parallel.all_gather_rows(apply_fn(frames_u8))
    fence()
    ta = time.perf_counter()
    for _ in range(args.steps):
      ops.forget_inputs()
      parallel.all_gather_rows(apply_fn(frames_u8))
    fence()
    tb = torch.tensor([time.perf_counter() - ta], device=dev, dtype=torch.float64)
    if collective:
      torch.distributed.all_reduce(tb, op=torch.distributed.ReduceOp.MAX)
    alt = {"format": "u8 (uint8 frames, 655 360 B per sample)", "steps": args.steps,
           "ms_per_step": float(tb.item()) / args.steps * 1e3,
           "samples_per_s": world * B * args.steps / float(tb.item())}
  # the same steps as ONE graph launch each (the product's nn.capture; the reference's step is
  # jit-compiled, examples/eval.py:108-116): the conv kernels keep their work queues inside a
  # capture, and the launches lose the per-launch memset / event / Python between them.  One
  # process only: a capture that failed on some rank of a multi-GPU job would take the whole
  # line with it, and the figure is a per-GPU one anyway (--graph runs it on every rank).
  cap_leg = None
  # (Every input format captures: float32 frames are checked on the device since round 5.)
  if (gpu and full and not args.stand_in and not args.graph and args.feed == "resident"
      and not args.no_fed_leg and world == 1):
    captured = nn.capture(model, variables, x, trgt=None, train=False, rng=None)
    for _ in range(2):
      parallel.all_gather_rows(captured()[0])
    fence()
    tc0 = time.perf_counter()
    for _ in range(args.steps):
      parallel.all_gather_rows(captured()[0])
    fence()
    tcv = torch.tensor([time.perf_counter() - tc0], device=dev, dtype=torch.float64)
    if collective:
      torch.distributed.all_reduce(tcv, op=torch.distributed.ReduceOp.MAX)
    cap_leg = {"api": "nn.capture: model.apply recorded into a hipGraph, one graph launch per step",
               "steps": args.steps, "ms_per_step": float(tcv.item()) / args.steps * 1e3,
               "samples_per_s": world * B * args.steps / float(tcv.item())}
    del captured
  # the host-fed leg (every rank runs it: the step holds a collective); binary frames only
  fed = None
  if (gpu and full and frames_u8 is not None and args.feed == "resident"
      and not args.no_fed_leg and not args.counts and not args.graph):
    fed = fed_leg(args, frames_u8, apply_fn, parallel, fence, dev, args.steps, min(args.warmup, 2))
    tf = torch.tensor([fed["ms_per_step"]], device=dev, dtype=torch.float64)
    if collective:
      torch.distributed.all_reduce(tf, op=torch.distributed.ReduceOp.MAX)
    fed["ms_per_step"] = float(tf.item())
    fed["samples_per_s_per_gpu"] = B / (fed["ms_per_step"] * 1e-3)

  # the general case beside the headline's best case (every rank runs it: the step holds a collective)
  general = None
  notes_main = dict(ops.PROFILE_NOTES) if ops is not None else {}
  if (gpu and full and args.model == "c3" and args.feed == "resident" and not args.no_fed_leg
      and not args.counts and not args.random_bn and not args.graph and args.input == "ev1"):
    general = general_leg(args, model, dev, B, T, parallel, fence, args.steps, min(args.warmup, 3))
    tg = torch.tensor([general["ms_per_step"]], device=dev, dtype=torch.float64)
    if collective:
      torch.distributed.all_reduce(tg, op=torch.distributed.ReduceOp.MAX)
    general["ms_per_step"] = float(tg.item())
    general["samples_per_s_per_gpu"] = B / (general["ms_per_step"] * 1e-3)
    general["vs_headline"] = general["samples_per_s_per_gpu"] / (B * args.steps / dt)

  if rank != 0:
    return
  value = world * B * args.steps / dt

  line = {
      "metric": metric_name(args),
      "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps,
      "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
      "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
      "dtype": issued_dtype(args, lb),
      "dtype_detail": "the operand formats the dominant kernel issues; the arithmetic is integer and "
                      "exact throughout: codes of magnitude <= 7 (DuQ up to 4 bits) as fp6 (e2m3) x "
                      "spikes as fp4 (e2m1) on v_mfma_scale_f32_32x32x64_f8f6f4, sums < 2^24 exact in the "
                      "f32 accumulator (conv1, conv2, read-out); wider codes and conv0 / the C2 head as "
                      "int8 x int8 (u8 counts as x - 128) -> int32 on v_mfma_i32_32x32x32_i8; membrane "
                      "potentials f32",
      "data": ("synthetic Poisson(%g) event counts" if args.counts else "synthetic Poisson(%g)>0 spikes")
              % args.lam + {"ev1": " as bit-packed frames (EV1, include/snnqp.h)", "ev4": " as nibble-packed "
                            "frames (EV4)", "u8": " as uint8 frames", "f32": " as float32 frames (staged in place, checked on the device)",
                            "bits": " as bit-packed rows"}[args.input] +
              ", N(0,1/fan_in) weights, " +
              ("random BatchNorm statistics" if args.random_bn else "BatchNorm as initialised") +
              ", random seeds fixed",
      "config": {"workload": ("%s: qdense(2048->512)+LIF -> qdense(512->%d)+LIF + vote, [B, T, 2048] "
                              "binary spikes, T=%d, %s"
                              % ("C1" if args.bits < 0 else "C2", args.classes * 10, T,
                                 ("float32 weights (no quantiser)" if args.bits < 0 else "%d-bit" % args.bits) + ", " +
                                 ("no pruning" if args.prune < 0 else "%.4g%% pruned" % (args.prune * 100))))
                             if args.model == "dense" else
                             ("CextNet (reference TCJA model): 5x qconv3x3 blocks + 2 TCJA gates + "
                              "qdense(2048->512->%d) + vote, " % (args.classes * 10)
                              if args.model == "cextnet" else
                              "C3 topology: 3x(qconv3x3+BN+LIF+pool2) + qdense(32768->%d)+LIF + vote, "
                              % (args.classes * 10)) +
                             "DVS128 128x128x2, T=%d, bits %s, %.4g%% pruned" %
                             (T, "/".join(str(b) for b in lb), args.prune * 100),
                 "batch_per_gpu": B, "global_batch": world * B, "frames": T,
                 "parallelism": "dp%d (batch-sharded, all-gather logits)" % world},
  }
  # the ranks the collective spanned: distinct devices (PCI addresses when the backend is RCCL)
  line["ranks_seen"] = len({(i.get("pci"), i.get("device"), i["rank"]) for i in ids})
  line["ranks"] = [{k: i.get(k) for k in ("rank", "device", "pci", "rccl", "pid") if k in i} for i in ids]
  line["rank_seconds"] = rank_dt
  line["rank_detail"] = rank_detail
  line["collective"] = ("%s process group of %d rank(s): all-gather of the logits every step, "
                        "barrier + all-reduce(MAX) around the timed region" % (args.backend, world)
                        ) if collective else "none (one process, no process group)"
  if full:
    line["fallbacks"] = ops.fallback_counts()      # blocks on the direct-form kernel (should be 0)
    line["fallbacks"].update(ops.workqueue_stats())   # static patch walks, arithmetic instead of table dequantisation
    line["device_status"] = ops.device_status()       # 0: no kernel reported a broken invariant
  if args.graph:
    line["config"]["launch"] = "hipGraph replay of model.apply (kernel times from an eager pass)"
  if build_flags or os.environ.get("SNNQP_DIAG_LIB"):
    line["DIAGNOSTIC_BUILD"] = build_flags or os.environ.get("SNNQP_DIAG_LIB")
  if args.stand_in:
    line["stand_in"] = True
    emit(args, line)
    return
  if args.feed == "host":
    line["pcie_inclusive"] = True
    line["feed"] = {"mode": "host", "format": args.input, "prefetch_depth": 2,
                    "h2d_GBps": fed_bytes / dt / 1e9, "bytes_per_sample": fed_bytes / (B * args.steps)}
  else:
    line["feed"] = {"mode": "resident", "format": args.input}
  if fed is not None:
    fed["vs_resident"] = fed["samples_per_s_per_gpu"] / (value / world)
    line["fed"] = fed
  if alt is not None:
    line["resident_u8"] = alt
  if cap_leg is not None:
    line["captured"] = cap_leg
  if general is not None:
    line["general"] = general
  if args.model != "dense":
    # which specialisations this line's `value` took: the `general` leg takes none
    line["config"]["specialisations"] = {
        "input": {"ev1": "binary frames, bit-packed (EV1), resident in HBM", "ev4": "count frames <= 15, "
                  "nibble-packed (EV4)", "u8": "uint8 frames", "f32": "float32 frames"}[args.input]
                 + (", event counts" if args.counts else ", binary events")
                 + (", fed from host memory" if args.feed == "host" else ""),
        "bn_flags": "random statistics: sub, mul, add" if args.random_bn else
                    "mean 0 / bias 0 / one multiplier for every channel (as initialised): no BatchNorm "
                    "instruction in conv1 / conv2 (the multiplier is folded into the shared table's entries)"}
    if full:
      line["config"]["specialisations"]["dequant_form"] = {t: v.get("dequant") for t, v in notes_main.items()}
  # the --full headline run measures the HBM bytes of its kernels itself (two counter passes of one
  # step each in child processes); any failure falls back to the committed figure, labelled
  default_headline = (world == 1 and args.model == "c3" and args.input == "ev1" and B == 1024 and T == 20
                      and not args.layer_bits and args.bits == 4 and not args.counts and not args.random_bn
                      and args.feed == "resident" and not args.no_fed_leg and not args.graph
                      and not args.no_legs and full)
  if default_headline and not args.no_live_traffic and not os.environ.get("SNNQP_BENCH_NO_PMC"):
    global LIVE_TRAFFIC
    try:
      tags, src = live_traffic([])
    except Exception as e:          # never at the price of the line
      tags, src = None, "%s: %s" % (type(e).__name__, e)
    if tags is not None:
      LIVE_TRAFFIC = (tags, src, (args.input, bool(args.counts), bool(args.random_bn)))
      args._live_traffic_ok = True
    else:
      line["traffic_live"] = "not measured: %s" % src
  if full:
    line.update(rooflines_of(args, prof, B, T, lb, notes_main))
    if os.path.exists(PARITY_VS_FLOAT):
      with open(PARITY_VS_FLOAT) as f:
        line["parity_vs_float"] = dict(json.load(f).get("summary") or {},
                                       source="committed %s (CPU, oracle int vs float mode; not "
                                              "measured in this run)" % os.path.relpath(PARITY_VS_FLOAT, ROOT))
  # the other single-GPU BASELINE configurations, timed in the same run: C2 as
  # BASELINE.json configs[1] names it (B = 256, T = 20, 8-bit, 50 % pruned; uint8 rows) and C5's
  # per-GPU share (B = 512, T = 50, mixed 2/4-bit, 95 % pruned, 10 classes; EV1 frames)
  if default_headline:
    del x, frames_u8
    torch.cuda.empty_cache()
    line["legs"] = {
        "c2": config_leg(args, dict(model="dense", batch=256, frames=20, bits=8, prune=0.5, input="u8",
                                    layer_bits=None, classes=11), dev, 200, 20, True),
        "c2_b4096": config_leg(args, dict(model="dense", batch=4096, frames=20, bits=8, prune=0.5,
                                          input="u8", layer_bits=None, classes=11), dev, 50, 5, False),
        "c5": config_leg(args, dict(model="c3", batch=512, frames=50, bits=4, prune=0.95, input="ev1",
                                    layer_bits=[2, 4, 2, 4], classes=10), dev, args.steps, 3, False),
        # the reference's own input format: float32 rows / frames staged in place and checked on
        # the device (flax_qdense.py:67, flax_qconv.py:101); the dense layer's HBM roofline is on
        # the bytes the kernel really reads
        "c2_b4096_f32": config_leg(args, dict(model="dense", batch=4096, frames=20, bits=8, prune=0.5,
                                              input="f32", layer_bits=None, classes=11), dev, 50, 5, True),
        "c2_b4096_bits": config_leg(args, dict(model="dense", batch=4096, frames=20, bits=8, prune=0.5,
                                               input="bits", layer_bits=None, classes=11), dev, 50, 5, False),
        "c2_f32": config_leg(args, dict(model="dense", batch=256, frames=20, bits=8, prune=0.5,
                                        input="f32", layer_bits=None, classes=11), dev, 200, 20, True),
        "c3_f32": config_leg(args, dict(model="c3", batch=1024, frames=20, bits=4, prune=0.9, input="f32",
                                        layer_bits=None, classes=11), dev, args.steps, 3, True),
    }
  if full and world == 1 and not args.no_cpu_baseline and args.model == "c3":
    line["cpu_baseline"] = cpu_baseline(args, variables_np)
  emit(args, line)


# the driver keeps the last 8 000 bytes of stdout and parses the final line out of them
# (BENCH_r05.json: a 29 KB line left `parsed: null`); tests/test_host_cpu.py holds the line to this
LINE_LIMIT = 6000
_ROOFLINE_KEYS = ("kernel", "launches_per_step", "avg_launch_ms", "algorithmic_bytes", "traffic", "bound",
                  "achieved", "peak", "unit", "frac")
_DENSE_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms",
               "algorithmic_bytes")
_CPU_KEYS = ("value", "unit", "cores", "kind", "cpu", "sample")


def compact(line):
  """The ONE stdout line: the contract's keys, the dominant kernel's roofline, the dense layer's,
  the CPU baseline and one {value, ms_per_step, frac} per leg.  Everything else (per-kernel and
  per-rank blocks, every leg's rooflines, the committed parity summary) is in the detail file."""
  def pick(d, keys):
    return {k: d[k] for k in keys if k in d}
  out = pick(line, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                    "scaling", "vs_baseline", "dtype", "data"))
  out["config"] = pick(line.get("config", {}), ("workload", "batch_per_gpu", "global_batch", "frames",
                                                "parallelism", "launch"))
  if line.get("roofline"):
    out["roofline"] = pick(line["roofline"], _ROOFLINE_KEYS)
    src = line["roofline"].get("traffic_source") or ""
    out["roofline"]["traffic_measured"] = "live" if src.startswith("measured in this run") else "committed file"
  if line.get("roofline_dense"):
    out["roofline_dense"] = pick(line["roofline_dense"], _DENSE_KEYS)
  if line.get("cpu_baseline"):
    out["cpu_baseline"] = pick(line["cpu_baseline"], _CPU_KEYS)
  out.update(pick(line, ("ranks_seen", "rank_seconds", "fallbacks", "device_status", "stand_in",
                         "pcie_inclusive", "DIAGNOSTIC_BUILD")))
  if line.get("kernels"):
    out["kernel_ms"] = {t: round(k["avg_ms"], 5) for t, k in line["kernels"].items()}

  def leg_of(d, value_key):
    r = d.get("roofline_dense") if (d.get("config") or {}).get("model") == "dense" else d.get("roofline")
    leg = {"value": d[value_key], "ms_per_step": d["ms_per_step"]}
    if r:
      leg.update(frac=r["frac"], bound=r["bound"])
    if d.get("captured"):
      leg["captured_value"] = d["captured"]["samples_per_s"]
    return leg
  legs = {}
  for name, key in (("fed", "samples_per_s_per_gpu"), ("resident_u8", "samples_per_s"),
                    ("captured", "samples_per_s"), ("general", "samples_per_s_per_gpu")):
    if line.get(name):
      legs[name] = leg_of(line[name], key)
  for name, d in (line.get("legs") or {}).items():
    legs[name] = leg_of(d, "samples_per_s")
  if legs:
    out["legs"] = legs
  if line.get("detail"):
    out["detail"] = line["detail"]
  return out


def emit(args, line):
  """Rank 0's output: the full record into the detail file(s), the compact line on stdout."""
  paths = [args.detail] if args.detail else [os.path.join(ROOT, "bench_detail.json")]
  if not args.detail and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
    paths.append(os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
  written = []
  for path in paths:
    try:
      with open(path, "w") as f:
        json.dump(line, f)
        f.write("\n")
      written.append(os.path.relpath(path, ROOT) if path.startswith(ROOT) else path)
    except OSError:
      pass
  line["detail"] = written[0] if written else None
  if args.full_line:
    print(json.dumps(line), flush=True)
    return
  short = compact(line)
  for drop in (None, "kernel_ms", "legs", "data", "rank_seconds"):     # never lose the line to its own length
    if drop:
      short.pop(drop, None)
    text = json.dumps(short)
    if len(text) < LINE_LIMIT:
      break
  print(text, flush=True)


LIVE_TRAFFIC = None      # {tag: HBM bytes per launch} measured by live_traffic() in this run, or None


def live_traffic(argv_model, timeout=150.0):
  """HBM bytes per launch of this run's kernels, MEASURED: two child runs of this script (one step
  each, no legs, no CPU baseline) under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` / `... WRITE_SIZE`
  -- separate passes, counters only, as MI355X_MICROARCH.md prescribes -- summed per kernel by
  tools/pmc_summary.py (bytes = 2 x FETCH_SIZE KiB + WRITE_SIZE KiB on gfx950).  Returns
  ({tag: bytes}, source) or (None, why).  The parent holds its batch in HBM meanwhile and is idle."""
  import shutil
  import tempfile
  prof = shutil.which("rocprofv3")
  if prof is None:
    return None, "rocprofv3 not on PATH"
  t0 = time.time()
  with tempfile.TemporaryDirectory(prefix="snnqp_pmc_", dir="/tmp") as tmp:
    env = dict(os.environ, TMPDIR="/tmp")
    for name in ("FETCH_SIZE", "WRITE_SIZE"):
      cmd = [prof, "--kernel-trace", "--pmc", name, "--output-format", "csv", "-d", os.path.join(tmp, name.lower()),
             "--", sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
             "--no-fed-leg", "--no-legs", "--no-live-traffic", "--full", "--detail", os.devnull] + list(argv_model)
      try:
        p = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           timeout=max(10.0, timeout - (time.time() - t0)))
      except (subprocess.TimeoutExpired, OSError) as e:
        return None, "rocprofv3 pass %s: %s" % (name, type(e).__name__)
      if p.returncode != 0:
        return None, "rocprofv3 pass %s exited with %d" % (name, p.returncode)
    out = os.path.join(tmp, "traffic.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_summary.py"), tmp, "--steps", "3",
                        "--traffic", out, "--input-format", "live"], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, cwd=ROOT)
    if p.returncode != 0 or not os.path.exists(out):
      return None, "tools/pmc_summary.py failed"
    with open(out) as f:
      tags = json.load(f).get("bytes_per_launch", {})
  if not tags:
    return None, "no library kernel in the counter files"
  return tags, ("measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE, two child runs of one "
                "step each (%.0f s), bytes = 2 x FETCH_SIZE KiB + WRITE_SIZE KiB" % (time.time() - t0))


def rooflines_of(args, prof, B, T, lb, notes=None):
  """Per-kernel rooflines from the HIP events recorded on the launch stream inside the timed
  region: {roofline (dominant kernel), roofline_dense, rooflines, kernels}."""
  kern = {}
  for tag, (n, ms) in prof.items():
    kern[tag] = {"launches": n, "avg_ms": ms / max(n, 1)}
  nout = args.classes * 10

  def conv_peak(bits):      # codes of magnitude <= 7: fp4 x fp6 MFMA kernel for conv1/conv2
    return FP6_MFMA_PEAK_TOPS if bits <= 4 else INT8_MFMA_PEAK_TOPS
  # tag: (MACs per launch, algorithmic HBM bytes per launch in the formats the kernels
  #       really read / write, matrix peak of the instruction the kernel issues)
  # bytes of one input frame as conv0 reads it (ev4 frames are unpacked to uint8 first)
  in_bytes = {"f32": 128 * 128 * 2 * 4, "u8": 128 * 128 * 2, "ev4": 128 * 128 * 2,
              "ev1": 128 * 128 * 2 // 8, "bits": 0}[args.input]
  # bytes of one [2048] row as the dense head reads it: uint8 in place, float32 in place (the
  # reference's own format, flax_qdense.py:67), or bit-packed
  row_bytes = {"u8": 2048, "f32": 8192}.get(args.input, 256)
  spec = {
      "conv3x3[128x128x2->128]": (B * T * 128 * 128 * 128 * 18,
                                  B * T * (in_bytes + 64 * 64 * 16), INT8_MFMA_PEAK_TOPS),
      "conv3x3[64x64x128->128]": (B * T * 64 * 64 * 128 * 1152,
                                  B * T * (64 * 64 * 16 + 32 * 32 * 16), conv_peak(lb[1])),
      "conv3x3[32x32x128->128]": (B * T * 32 * 32 * 128 * 1152,
                                  B * T * (32 * 32 * 16 + 16 * 16 * 16), conv_peak(lb[2])),
      # read-out: bit-packed rows in, spike words out, the codes once per launch -- 6-bit packed
      # (fp6 tiles, f8f6f4 MFMA) when they fit, else int8
      "dense[32768->%d]" % nout: (B * T * 32768 * nout,
                                  B * T * (4096 + 16) + 32768 * 128 * (3 if lb[3] <= 4 else 4) // 4,
                                  conv_peak(lb[3])),
      # config C2 (bit-packed spikes in and out, int8 codes once per launch)
      # (uint8 rows are read in place: 2048 B per sample-step, not the 256 B of a bit-packed row)
      "dense[2048->512]": (B * T * 2048 * 512, B * T * (row_bytes + 64) + 2048 * 512,
                           INT8_MFMA_PEAK_TOPS),
      "dense[512->%d]" % nout: (B * T * 512 * nout, B * T * (64 + 16) + 512 * 128, INT8_MFMA_PEAK_TOPS),
      # config C2 as ONE launch (snnqp_dense_head_forward): the uint8 rows as the kernel reads them
      # (2048 B per sample-step, in place), both code matrices once, the logits; the hidden
      # raster never leaves the CU
      # unquantised dense blocks (config C1): float32 connection on the f32 MFMA + the scan; rows in
      # the format they arrive in, float32 currents out and back, float32 kernels once
      "dense[f32 1x1x2048->512]": (B * T * 2048 * 512, B * T * (row_bytes + 2 * 512 * 4 + 64) + 2048 * 512 * 4,
                                   F32_MFMA_PEAK_TOPS),
      "dense[f32 1x1x512->%d]" % nout: (B * T * 512 * nout, B * T * (64 + 2 * nout * 4 + 16) + 512 * nout * 4,
                                        F32_MFMA_PEAK_TOPS),
      "dense_head[2048->512->%d]" % nout: (B * T * (2048 * 512 + 512 * nout),
                                           B * T * row_bytes + 2048 * 512
                                           + 512 * 128 + B * 4 * args.classes, INT8_MFMA_PEAK_TOPS),
  }
  traffic, traffic_src, pmc, pmc_src = {}, None, {}, None
  headline = (B == 1024 and T == 20 and not args.layer_bits and args.bits == 4 and args.model == "c3")
  if (headline and LIVE_TRAFFIC is not None and getattr(args, "_live_traffic_ok", False)
      and LIVE_TRAFFIC[2] == (args.input, bool(args.counts), bool(args.random_bn))):
    traffic, traffic_src = LIVE_TRAFFIC[:2]      # (the legs on other formats keep their committed figures)
  elif headline:
    for path in PMC_TRAFFIC:
      if os.path.exists(path):
        with open(path) as f:
          tj = json.load(f)
        if tj.get("input", "u8") == args.input:
          traffic = tj.get("bytes_per_launch", {})
          traffic_src = "committed %s (rocprofv3 --pmc passes of this command; not measured in this run)" \
              % os.path.relpath(path, ROOT)
          break
  if headline:
    for path in PMC_SUMMARY:
      if os.path.exists(path):
        with open(path) as f:
          pmc = json.load(f)
        pmc_src = "committed %s (not measured in this run)" % os.path.relpath(path, ROOT)
        break

  c2_traffic = None
  if args.model == "dense" and T == 20 and args.bits == 8:
    c2_traffic = {(256, "u8"): "pmc_c2_traffic.json", (4096, "f32"): "pmc_c2_b4096_f32_traffic.json"}.get(
        (B, args.input))
  if c2_traffic:
    path = next((q for q in (os.path.join(ROOT, "profiles", r + "_" + c2_traffic) for r in ("r06", "r05"))
                 if os.path.exists(q)), "")
    if path:
      with open(path) as f:
        traffic = json.load(f).get("bytes_per_launch", {})
      traffic_src = "committed %s (rocprofv3 --pmc passes of this command; not measured in this run)" \
          % os.path.relpath(path, ROOT)

  def pmc_valu(prefix, which=0):
    """SQ_INSTS_VALU per launch of the `which`-th kernel whose name starts with `prefix`."""
    names = sorted(k for k in pmc if k.startswith(prefix))
    if which < len(names) and "SQ_INSTS_VALU" in pmc[names[which]]:
      return pmc[names[which]]["SQ_INSTS_VALU"]
    return None

  def roofline_of(tag):
    k = kern[tag]
    macs, nbytes, peak = spec[tag]
    sec = k["avg_ms"] * 1e-3
    tops, gbs = 2.0 * macs / sec / 1e12, nbytes / sec / 1e9
    hbm_frac, mfma_frac = gbs / HBM_PEAK_GBS, tops / peak
    r = {"kernel": tag, "avg_launch_ms": k["avg_ms"], "traffic": traffic.get(tag),
         "traffic_source": traffic_src if traffic.get(tag) is not None else None,
         "algorithmic_bytes": nbytes, "hbm_frac": hbm_frac, "mfma_frac": mfma_frac}
    if mfma_frac >= hbm_frac:
      r.update(bound="mfma", achieved=tops, peak=peak, unit="TFLOP/s", frac=mfma_frac)
    else:
      r.update(bound="hbm", achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s", frac=hbm_frac)
    return r

  rooflines = {tag: roofline_of(tag) for tag in kern if tag in spec}
  for tag, r in rooflines.items():
    kern[tag]["tops"] = 2.0 * spec[tag][0] / (kern[tag]["avg_ms"] * 1e-3) / 1e12
    kern[tag]["hbm_gbs"] = spec[tag][1] / (kern[tag]["avg_ms"] * 1e-3) / 1e9
  # dominant KERNEL = the device function with the largest share of the step, as
  # rocprofv3 --stats groups it (conv1 and conv2 are two launches of one kernel):
  # achieved = algorithmic ops (bytes) per launch / average launch duration
  conv_kernel = "conv3x3_bits_kernel"   # one device function, fp6 or int8 instruction inside
  dense_tag = "dense[2048->512]" if args.model == "dense" else "dense[32768->%d]" % nout
  if args.model == "dense" and "dense_head[2048->512->%d]" % nout in kern:
    dense_tag = "dense_head[2048->512->%d]" % nout
  groups = {conv_kernel: ["conv3x3[64x64x128->128]", "conv3x3[32x32x128->128]"],
            "conv3x3_u8c2_kernel": ["conv3x3[128x128x2->128]"],
            "dense kernel": [dense_tag] + (["dense[512->%d]" % nout] if args.model == "dense" else []),
            "fseq_gemm_kernel": ["dense[f32 1x1x2048->512]", "dense[f32 1x1x512->%d]" % nout]}
  gtime = {g: sum(kern[t]["avg_ms"] * kern[t]["launches"] for t in tags if t in kern)
           for g, tags in groups.items()}
  out = {"kernels": kern}
  if not any(gtime.values()):
    return out
  dom = max(gtime, key=gtime.get)
  tags = [t for t in groups[dom] if t in kern]
  nl = sum(kern[t]["launches"] for t in tags)
  avg_ms = gtime[dom] / nl
  nops = sum(2.0 * spec[t][0] * kern[t]["launches"] for t in tags) / nl
  nbytes = sum(spec[t][1] * kern[t]["launches"] for t in tags) / nl
  # launches of one device function may run on different instructions (mixed precision):
  # the peak is the time-weighted one of the launches
  peak = sum(spec[t][2] * kern[t]["avg_ms"] * kern[t]["launches"] for t in tags) / gtime[dom]
  tops, gbs = nops / (avg_ms * 1e-3) / 1e12, nbytes / (avg_ms * 1e-3) / 1e9
  tr = [traffic.get(t) for t in tags]
  roofline = {"kernel": dom, "launches_per_step": len(tags), "layers": tags,
              "avg_launch_ms": avg_ms, "algorithmic_bytes": nbytes,
              "traffic": (sum(tr) / len(tr)) if all(v is not None for v in tr) else None,
              "traffic_source": traffic_src if all(v is not None for v in tr) else None,
              "hbm_frac": gbs / HBM_PEAK_GBS, "mfma_frac": tops / peak,
              "share_of_step": gtime[dom] / sum(gtime.values())}
  if tops / peak >= gbs / HBM_PEAK_GBS:
    roofline.update(bound="mfma", achieved=tops, peak=peak, unit="TFLOP/s", frac=tops / peak)
  else:
    roofline.update(bound="hbm", achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s",
                    frac=gbs / HBM_PEAK_GBS)
  if dom == conv_kernel:
    # Beside the MFMAs the SIMD issues the neuron epilogue.  Per 32-pixel x
    # 32-channel tile-step a wave issues 18 MFMAs (32 cycles of the matrix pipe each: 576) and the
    # epilogue of 1024 neuron updates; that epilogue's vector instructions alone -- [dequantise 3,]
    # BatchNorm multiply, sub, fma, compare, select, half a v_writelane per update, no LDS, no
    # MFMA -- cost 466 SIMD cycles per tile-step at the kernel's two waves per SIMD with the
    # arithmetic dequantisation and 318 with the table form, which reads the current from LDS
    # instead (tools/ubench/threshold_forms.hip, profiles/r03_threshold_forms.txt).
    forms = sorted({(notes or {}).get(t, {}).get("dequant", "arith") for t in tags})
    mix_cycles = 318.0 if forms == ["table"] else 466.0
    updates = sum(B * T * hw * hw * 128 * kern[t]["launches"]
                  for t, hw in (("conv3x3[64x64x128->128]", 64), ("conv3x3[32x32x128->128]", 32))
                  if t in kern) / nl
    tiles_per_simd = updates / 1024.0 / 1024.0
    mix_ms = tiles_per_simd * mix_cycles / 2.4e9 * 1e3
    mfma_ms = tiles_per_simd * 576.0 / 2.4e9 * 1e3
    vi = {"updates_per_launch": updates, "dequant": "/".join(forms),
          "measured_mix_cycles_per_tile": mix_cycles,
          "mfma_cycles_per_tile": 576.0, "measured_mix_ms": mix_ms, "mfma_only_ms": mfma_ms,
          "measured_mix_frac": mix_ms / avg_ms,
          "note": "epilogue vector instructions alone / launch time; they share the issue port "
                  "with the MFMAs (8 issue cycles each) and the staging"}
    v1, v2 = pmc_valu("snnqp::conv3x3_bits_kernel", 0), pmc_valu("snnqp::conv3x3_bits_kernel", 1)
    if v1 is not None and v2 is not None and len(tags) == 2:
      vi["instr_per_update"] = (v1 + v2) / 2.0 / (updates / 64.0)
      vi["instr_per_update_source"] = pmc_src
    roofline["valu_issue"] = vi
  c0 = rooflines.get("conv3x3[128x128x2->128]")
  if c0 is not None:
    # third, stated ceiling of conv0: VALU issue of the per-neuron epilogue.  updates per
    # launch x wave-instructions per update (3.5 in the table variant on binary
    # events) / 64 lanes, against one wave-instruction per SIMD every 4 cycles
    updates = B * T * 128 * 128 * 128
    instr_per_update = 3.5
    ceiling_ms = updates * instr_per_update / 64.0 / (VALU_PEAK_GINSTR * 1e9) * 1e3
    # the same ceiling from a measurement instead of a count: the tile's vector instructions
    # alone (8 x {v_pk_add, v_pk_fma, 2 v_cmp, 2 v_cndmask, v_writelane}, 4 waves per SIMD, no
    # LDS, no MFMA: tools/ubench/u8c2_epilogue_rate.hip) take 245 SIMD cycles per 32-pixel x
    # 32-channel tile-step at 2.4 GHz -- compare / select / min / max issue every 4.2 cycles,
    # add / mul / fma / and every 2.3 (tools/ubench/pk_f32_rate.hip)
    tiles_per_simd = updates / 1024.0 / 1024.0           # 1024 updates per tile-step, 1024 SIMDs
    mix_ms = tiles_per_simd * 245.0 / 2.4e9 * 1e3
    v0 = pmc_valu("snnqp::conv3x3_u8c2_kernel")
    if v0 is not None:
      c0_counted = {"instr_per_update_counted": v0 / (updates / 64.0), "counted_source": pmc_src}
    else:
      c0_counted = {}
    c0["valu_issue"] = {**c0_counted, "updates": updates, "instr_per_update": instr_per_update,
                        "peak_ginstr_per_s": VALU_PEAK_GINSTR, "ceiling_ms": ceiling_ms,
                        "frac": ceiling_ms / c0["avg_launch_ms"],
                        "measured_mix_cycles_per_tile": 245.0, "measured_mix_ms": mix_ms,
                        "measured_mix_frac": mix_ms / c0["avg_launch_ms"]}
    c0["note"] = ("conv0 does 18 MACs and 0.3 HBM bytes per neuron update; it is bound by VALU "
                  "issue of the neuron epilogue (valu_issue.frac of that ceiling), neither roofline")
  dn = rooflines.get(dense_tag)
  roofline_dense = None
  if dn is not None:
    # the read-out cannot reach the HBM roof in a dense-MFMA formulation: at the int8 MFMA
    # peak the launch would take ops / peak seconds, which caps the HBM fraction at
    # ceiling_hbm_frac whatever the kernel does
    macs, nbytes, peak = spec[dense_tag]
    t_mfma = 2.0 * macs / (peak * 1e12)
    roofline_dense = {"kernel": dn["kernel"], "bound": "hbm",
                      "achieved": kern[dn["kernel"]]["hbm_gbs"], "peak": HBM_PEAK_GBS,
                      "unit": "GB/s", "frac": dn["hbm_frac"], "traffic": dn["traffic"],
                      "avg_launch_ms": dn["avg_launch_ms"], "mfma_frac": dn["mfma_frac"],
                      "ceiling_hbm_frac": nbytes / t_mfma / 1e9 / HBM_PEAK_GBS,
                      "ceiling": "%s MFMA peak: %.3f ms per launch; in practice the code stream "
                                 "through each CU's vector L1 (64 B/clk) binds first, DESIGN.md 4.4"
                                 % ("fp6" if peak == FP6_MFMA_PEAK_TOPS else "int8", t_mfma * 1e3)}
  out.update(roofline=roofline, roofline_dense=roofline_dense,
             rooflines=[rooflines[k] for k in sorted(rooflines)])
  return out


if __name__ == "__main__":
  try:
    main()
  finally:
    td = sys.modules.get("torch.distributed")
    if td is not None and td.is_available() and td.is_initialized():
      td.destroy_process_group()
