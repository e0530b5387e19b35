"""Batch-chunk co-run A/B: the event layer (conv0) on batch chunk c + 1 beside the
first bit-input block (conv1) on chunk c, two streams, against the same launches one after the other
on one stream -- product library, the headline's weights, plan and batch (C3, B = 1024, T = 20, EV1),
one process, alternating, medians.

The two blocks are the model's own: one apply() of ConvDenseSNN with ops.conv_lif_forward wrapped
hands over the geometry, packed weights, BatchNorm and neuron of its first two blocks exactly as the
model launches them (the compacted 96-channel event layer on the spread instance and the CIN = 80
bit-input instance; ops.PROFILE_NOTES is checked for both).  A chunk is a slice of the batch: conv0
reads samples [b0, b0 + Bc) of the resident frames and writes a raster of its own, conv1 reads that
raster -- the same kernels, instances and work per sample as one launch over the whole batch, in K
launches each.

Schedules per K:
  serial     conv0(0), then conv1(c), conv0(c + 1) for every chunk, one stream
  corun      the same launches, conv1 on a second stream of higher priority that waits on conv0(c)'s
             event; conv0(c + 1) goes on the caller's stream; the second stream is joined at the end
  corun_swap the same with conv0(c + 1) enqueued before conv1(c)
and `whole`: one launch of each block over the whole batch (what the model runs); each block alone.
A last pass puts an event pair around every launch (`per_launch_ms`) and gives, chunk against chunk,
r = a conv0 launch's time in the serial schedule over its time in the co-running one and s = the
same ratio inverted for conv1.  They are ratios of whole launch times: a launch whose workgroups
wait for room on the CUs, or that has company for a part of its run only, counts in full.  What
one state of the device is worth comes from `--cap 1` and the kernel trace.

  python tools/corun_ab.py [--B 1024] [--T 20] [--K 2 4 8] [--reps 5] [--out FILE.json]

conv0's persistent grid is six workgroups per CU; beside two conv1 workgroups a CU holds one.  With
  python tools/diag_build.py event_grid_cap --patch tools/diag/event_grid_cap.patch
  SNNQP_DIAG_LIB=diag_build/event_grid_cap/libsnnqp.so python tools/corun_ab.py --cap 1 ...
the schedule corun_cap1 launches the co-running conv0 chunks on one workgroup per CU, so that none
of conv0's workgroups waits for the CU that a draining conv1 chunk frees.

What the device did (do the launches overlap?) comes from a kernel trace of ONE schedule:
  rocprofv3 --kernel-trace -d DIR -o NAME --output-format csv -- python tools/corun_ab.py --K 4 --only corun_K4
  python tools/corun_ab.py --K 4 --overlap DIR/NAME_kernel_trace.csv
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from snnquantprune_amd import _lib as L, linen as nn, models, ops, synthetic as syn  # noqa: E402


def headline_blocks(B, T, dev):
  """((args, kwargs) of the first two ops.conv_lif_forward calls of the headline apply, the notes)."""
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(syn.conv_net_variables(prune_p=0.9, out=110), dev)
  gen = torch.Generator(device=dev)
  gen.manual_seed(8627169)
  x = (torch.rand((B, T, 128, 128, 2), device=dev, generator=gen) < 1.0 - np.exp(-0.1)).to(torch.uint8)
  x = ops.pack_frames(x, L.EV1)
  calls = []
  real = ops.conv_lif_forward

  def spy(*args, **kwargs):
    calls.append((args, kwargs))
    return real(*args, **kwargs)

  ops.conv_lif_forward = spy
  try:
    model.apply(variables, x, trgt=None, train=False, rng=None)      # packs, caches, the queue pool
    del calls[:]
    ops.profile_start()
    model.apply(variables, x, trgt=None, train=False, rng=None)
    ops.profile_stop()
  finally:
    ops.conv_lif_forward = real
  notes = {t: dict(v) for t, v in ops.PROFILE_NOTES.items()}
  assert len(calls) >= 2, len(calls)
  return calls[0], calls[1], notes


def check_instances(c0, c1, notes):
  """The facts that make these the headline's two instances; raises if one does not hold."""
  g0, g1 = c0[0][1], c1[0][1]
  n0 = [v for t, v in notes.items() if "x2->" in t and "channels" in v]
  n1 = [v for t, v in notes.items() if "x2->" not in t and "channels" in v]
  assert isinstance(c0[0][0], ops.PackedFrames) and c0[0][0].fmt == L.EV1, "conv0 must read EV1 frames"
  assert n0 and n0[0]["channels"].get("wave_spread") and n0[0]["channels"].get("half_group"), n0
  assert (g0.Cin, g0.Cout) == (2, 96), g0
  assert g1.Cin == 80 and n1 and n1[0].get("dequant") == "table", (g1, n1)
  return {"conv0": {"cout": g0.Cout, **n0[0]["channels"]}, "conv1": {"cin": g1.Cin, "cout": g1.Cout, **n1[0]}}


def batch_chunks(B, K):
  """[(b0, Bc)] of K chunks that tile [0, B) in order, the first B % K one sample longer."""
  assert 1 <= K <= B, (B, K)
  base, rem = divmod(B, K)
  out, b0 = [], 0
  for c in range(K):
    bc = base + (1 if c < rem else 0)
    out.append((b0, bc))
    b0 += bc
  return out


def trace_overlap(path, last):
  """The last `last` conv0 and conv1 launches of a rocprofv3 --kernel-trace CSV (those of the one
  schedule `--only` ran after its warm-up): their intervals from the first start, in ms, and the
  time a conv0 and a conv1 launch were on the device together."""
  import csv
  rows = {"conv0": [], "conv1": []}
  with open(path) as f:
    for r in csv.DictReader(f):
      n = r["Kernel_Name"]
      k = "conv0" if "conv3x3_u8c2_kernel" in n else "conv1" if "conv3x3_bits_kernel" in n else None
      if k:
        rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), int(r["Grid_Size_X"])))
  rows = {k: sorted(v)[-last:] for k, v in rows.items()}
  t0 = min(v[0][0] for v in rows.values())
  both = sum(max(0, min(a[1], b[1]) - max(a[0], b[0])) for a in rows["conv0"] for b in rows["conv1"])
  return {"intervals_ms": {k: [[(s - t0) / 1e6, (e - t0) / 1e6] for s, e, _ in v] for k, v in rows.items()},
          "grid_x": {k: [g for _, _, g in v] for k, v in rows.items()},
          "side_by_side_ms": both / 1e6,
          "span_ms": (max(v[-1][1] for v in rows.values()) - t0) / 1e6}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--B", type=int, default=1024)
  ap.add_argument("--T", type=int, default=20)
  ap.add_argument("--K", type=int, nargs="+", default=[2, 4, 8])
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--out", default=None)
  ap.add_argument("--cap", type=int, default=0,
                  help="also: conv0's co-running launches on this many workgroups per CU (needs the diagnostic "
                       "build of tools/diag/event_grid_cap.patch, SNNQP_DIAG_LIB)")
  ap.add_argument("--only", default=None, help="warm up, then run this one schedule once (under a kernel trace)")
  ap.add_argument("--overlap", default=None, metavar="KERNEL_TRACE_CSV",
                  help="no GPU work: time conv0 and conv1 launches of a rocprofv3 kernel trace ran side by side")
  args = ap.parse_args()
  if args.overlap:
    print(json.dumps(trace_overlap(args.overlap, args.K[0]), sort_keys=True))
    return
  if args.cap:
    assert "event_grid_cap" in L.build_flags(), "--cap needs the event_grid_cap diagnostic build"
  dev = torch.device("cuda:0")
  B = args.B
  c0, c1, notes = headline_blocks(B, args.T, dev)
  instances = check_instances(c0, c1, notes)
  x0 = c0[0][0]
  assert not c0[1].get("time_major", True), "the event layer reads the batch-major frames in place"
  hi = -1                                                     # (lower numbers are higher priorities)
  side = torch.cuda.Stream(device=dev, priority=hi)           # conv1's: the higher priority
  keep = []                                                   # rasters stay referenced until the fence
  marks = {"on": False, "conv0": [], "conv1": []}             # the detail pass: an event pair per launch

  def launch(which, fn):
    if not marks["on"]:
      return fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    marks[which].append((a, b))
    return out

  def conv0(b0, bc, cap=0):
    if cap:
      os.environ["SNNQP_DIAG_EVENT_WGS_PER_CU"] = str(cap)
    try:
      out = launch("conv0", lambda: ops.conv_lif_forward(x0[b0:b0 + bc], *c0[0][1:], **c0[1])[1])
    finally:
      os.environ.pop("SNNQP_DIAG_EVENT_WGS_PER_CU", None)
    keep.append(out)
    return out

  def conv1(s):
    keep.append(launch("conv1", lambda: ops.conv_lif_forward(s, *c1[0][1:], **c1[1])[1]))

  def chunks(K):
    return batch_chunks(B, K)

  def whole():
    conv1(conv0(0, B))

  def serial(K):
    for b0, bc in chunks(K):
      conv1(conv0(b0, bc))

  def corun(K, swap=False, cap=0):
    cur = torch.cuda.current_stream(dev)
    ch = chunks(K)
    fork = torch.cuda.Event()
    fork.record(cur)
    side.wait_event(fork)
    s = conv0(*ch[0])
    for c in range(K):
      done = torch.cuda.Event()
      done.record(cur)                      # conv0(c) is the last thing on the caller's stream

      def consumer(s=s, done=done):
        side.wait_event(done)
        with torch.cuda.stream(side):
          conv1(s)

      def producer():
        return conv0(*ch[c + 1], cap=cap) if c + 1 < K else None

      if swap:
        nxt = producer()
        consumer()
      else:
        consumer()
        nxt = producer()
      s = nxt
    join = torch.cuda.Event()
    join.record(side)
    cur.wait_event(join)

  variants = [("whole", whole)]
  for K in args.K:
    variants += [("serial_K%d" % K, lambda K=K: serial(K)),
                 ("corun_K%d" % K, lambda K=K: corun(K)),
                 ("corun_swap_K%d" % K, lambda K=K: corun(K, True))]
    if args.cap:
      variants.append(("corun_cap%d_K%d" % (args.cap, K), lambda K=K: corun(K, cap=args.cap)))
  if args.cap:                              # conv0 alone on the capped grid: its rate at that occupancy
    variants.append(("conv0_cap%d_alone" % args.cap, lambda: conv0(0, B, cap=args.cap)))
  variants += [("conv0_alone", lambda: conv0(0, B)),
               ("conv1_alone", lambda s=conv0(0, B): conv1(s))]
  torch.cuda.synchronize()

  def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    del keep[:]
    return a.elapsed_time(b)

  for _, fn in variants:                    # every chunk shape once: allocator pools, occupancy cache
    timed(fn)
  if args.only:
    print("%s once: %.3f ms" % (args.only, timed(dict(variants)[args.only])))
    return
  ops.workqueue_stats(reset=True)
  ms = {name: [] for name, _ in variants}
  for _ in range(args.reps):
    for name, fn in variants:
      ms[name].append(timed(fn))
  med = {name: float(np.median(v)) for name, v in ms.items()}
  # one more pass with an event pair around every launch, on the launch's own stream: how long each
  # chunk's launch took in the serial and in the co-running schedule, waiting for room included.
  # r = conv0's serial time over its co-running time, s = conv1's co-running time over its serial
  # time (conv0's chunks 1 .. K - 1 and conv1's chunks 0 .. K - 2 are the ones that may have company)
  detail, rs = {}, {}
  for name, fn in variants:
    if name.startswith(("serial", "corun")):
      marks.update(on=True, conv0=[], conv1=[])
      timed(fn)
      marks["on"] = False
      detail[name] = {k: [a.elapsed_time(b) for a, b in marks[k]] for k in ("conv0", "conv1")}
  for name, d in detail.items():
    if name.startswith("corun"):
      K = int(name.rsplit("K", 1)[1])
      alone = detail["serial_K%d" % K]
      rs[name] = {"r": float(np.median(alone["conv0"][1:]) / np.median(d["conv0"][1:])),
                  "s": float(np.median(d["conv1"][:K - 1]) / np.median(alone["conv1"][:K - 1]))}
  res = {"B": B, "T": args.T, "reps": args.reps, "device": torch.cuda.get_device_name(0),
         "library": L.build_flags() or "product", "stream_priorities": {"conv0": 0, "conv1": hi},
         "instances": instances, "conv0_plus_conv1_ms_median": med, "conv0_plus_conv1_ms": ms,
         "per_launch_ms": detail, "r_s": rs,
         "gain_vs_whole_ms": {n: med["whole"] - v for n, v in med.items() if n.startswith(("serial", "corun"))},
         "workqueue_stats": ops.workqueue_stats(), "device_status": ops.device_status(),
         "fallback_counts": ops.fallback_counts()}
  for name, _ in variants:
    print("%-16s %.3f ms  (%s)" % (name, med[name], " ".join("%.3f" % v for v in ms[name])), flush=True)
  for name, v in rs.items():
    print("%-16s r %.2f  s %.2f" % (name, v["r"], v["s"]))
  print("workqueue_stats", res["workqueue_stats"], "device_status", res["device_status"])
  if args.out:
    with open(args.out, "w") as f:
      json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
  main()
