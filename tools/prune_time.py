"""Times one global prune event (prune_utils.prune_event, csrc/prune.hip) against the
host path it stands beside -- prune_utils.update_global_prune_mask: every kernel `.cpu()`,
np.argpartition, the masks copied back into the leaves -- at the weight counts of config C3
(ConvDenseSNN) and of CextNet, from masks of ones to 90 % sparsity (the most a single event can
have to do: every radix pass sees every weight).

Both sides start a call by resetting the masks to ones (timed alone as `reset_ms`, the same
launches for both).  The pairs are timed alternately, --reps rounds of --steps calls, after --warmup
calls: the device path between HIP events (it never synchronises), the host path, which ends in
host-to-device copies, with a host clock around calls closed by a device synchronise.  The median
and the spread (min, max) of the rounds are reported per call, in milliseconds.  These are whole
calls, host share included, not kernel times.  Before timing, the device masks are compared with
the host path's at the zero counts (the selections differ only inside ties at the cut, where
argpartition's choice is unspecified).

Prints one JSON line and writes it to --out (default profiles/prune_time.json).

  python tools/prune_time.py [--steps 10] [--warmup 3] [--reps 5] [--out profiles/prune_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SPARSITY = 0.9


def _stats(v):
  return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def _time_events(fn, steps, warmup):
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


def _time_host(fn, steps, warmup):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  t = time.perf_counter()
  for _ in range(steps):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) * 1e3 / steps


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_time.json"))
  args = ap.parse_args(argv)
  assert torch.cuda.is_available(), "prune_time.py needs the GPU"
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import prune_utils as pu
  from snnquantprune_amd import synthetic as syn
  dev = torch.device("cuda:0")
  result = {"tool": "prune_time", "steps": args.steps, "warmup": args.warmup, "reps": args.reps, "sparsity": SPARSITY,
            "timing": "whole calls, ms per call: device path between HIP events, host path by a host clock closed "
                      "with a device synchronise", "models": {}}
  for name, variables in (("c3", syn.conv_net_variables(prune_p=-1.0)), ("cextnet", syn.cextnet_variables(prune_p=-1.0))):
    params = pu.ones_masks(nn.tree_from_numpy(variables["params"], dev))
    layers = pu._layers(params)
    masks = [l["prune_0"]["mask"] for l in layers]
    total = sum(m.numel() for m in masks)

    def reset():
      for m in masks:
        m.fill_(1.0)

    def device_path():
      reset()
      pu.prune_event(params, SPARSITY, True)

    def host_path():
      reset()
      new = pu.update_global_prune_mask(params, SPARSITY)
      for old, upd in zip(layers, pu._layers(new)):
        old["prune_0"]["mask"].copy_(upd["prune_0"]["mask"])

    device_path()
    zd = int(pu.mask_zeros(params)[0])
    kept_d = torch.cat([(m != 0).reshape(-1) for m in masks]).cpu().numpy()
    host_path()
    zh = int(pu.mask_zeros(params)[0])
    kept_h = torch.cat([(m != 0).reshape(-1) for m in masks]).cpu().numpy()
    assert zd == zh == int(total * SPARSITY), (name, zd, zh, total)
    differ = int((kept_d != kept_h).sum())
    mags = np.abs(np.concatenate([l["kernel"].cpu().numpy().reshape(-1) for l in layers]))
    if differ:                                                      # only inside the ties at the cut
      assert np.unique(mags[kept_d != kept_h]).size == 1, name
    ms = {"device": [], "host": [], "reset": []}
    for _ in range(args.reps):                                      # alternating
      ms["device"].append(_time_events(device_path, args.steps, args.warmup))
      ms["host"].append(_time_host(host_path, args.steps, args.warmup))
      ms["reset"].append(_time_events(reset, args.steps, args.warmup))
    d, h = _stats(ms["device"]), _stats(ms["host"])
    result["models"][name] = {"layers": len(layers), "weights": total, "zeros": zd, "differ_inside_ties": differ,
                              "device_ms": d, "host_ms": h, "reset_ms": _stats(ms["reset"]),
                              "host_over_device": round(h["median"] / d["median"], 2)}
  line = json.dumps(result)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
  main()
