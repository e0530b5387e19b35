"""Conv K packing A/B: the same model, weights and batch with nn.set_conv_kpack off
(codes of the bit-input convs padded to 64 / 128 input channels) and on (to a multiple of 32), in
one process, alternating; per-kernel device time from the HIP-event profile and the whole apply.
Checks that logits are bit-equal.  --ab k16: the same A/B of nn.set_conv_k16 (off =
the kernel walks whole 32-channel groups, on = it leaves the empty upper half of the last group
out), K packing on in both.  --ab half: the same A/B of nn.set_event_half_group (off =
the event layer computes the whole last channel group and masks its silent half, on = it computes
that group in a 16-channel half); the C5 and 8-bit legs run identical instances both ways, so their
ratios are the session's noise.  --ab spread: the same A/B of nn.set_event_wave_spread (DESIGN.md 4.2:
off = wave w of the event layer computes channel group w, on = every wave one (group, tile) unit and a
quarter of the half group), the half group on in both.  --ab quarter: the same A/B of
nn.set_event_quarter16 (off = a spread wave takes its quarter out of the half group's whole
32x32x32 product, on = from one 16x16x64 product), half group and spread on in both; here the C5 leg
(64 channels: no quarter) and the 8-bit leg run identical instances both ways.

  python tools/kpack_ab.py [--ab kpack|k16|half|spread|quarter] [--B 1024] [--T 20] [--reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from snnquantprune_amd import _lib as L, linen as nn, models, ops, synthetic as syn  # noqa: E402

LEGS = [  # name, bits, prune, layer_bits, input
    ("C3", 4, 0.9, None, "ev1"),
    ("C3", 4, 0.9, None, "u8"),
    ("C5", 4, 0.95, (2, 4, 2, 4), "ev1"),
    ("8bit_30", 8, 0.3, None, "ev1"),
]


def leg(name, bits, prune, lb, inp, B, T, reps, dev, switch=nn.set_conv_kpack):
  cfg = syn.make_config(bits=bits, prune_percentage=prune)
  if lb:
    cfg.quant.layer_bits = tuple(lb)
  model = models.ConvDenseSNN(num_classes=11, config=cfg)
  variables = nn.tree_from_numpy(syn.conv_net_variables(prune_p=prune, out=110), dev)
  gen = torch.Generator(device=dev)
  gen.manual_seed(8627169)
  x = (torch.rand((B, T, 128, 128, 2), device=dev, generator=gen) < 1.0 - np.exp(-0.1)).to(torch.uint8)
  if inp == "ev1":
    x = ops.pack_frames(x, L.EV1)

  def run(kpack):
    switch(kpack)
    return model.apply(variables, x, trgt=None, train=False, rng=None)[0]

  out = {}
  ref = {}
  for kpack in (False, True):
    ref[kpack] = run(kpack).cpu().numpy()
    run(kpack)
  torch.cuda.synchronize()
  sums = {False: {}, True: {}}
  steps = {False: [], True: []}
  for _ in range(reps):
    for kpack in (False, True):
      run(kpack)
      torch.cuda.synchronize()
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      ops.profile_start()
      a.record()
      run(kpack)
      b.record()
      prof = ops.profile_stop()
      steps[kpack].append(a.elapsed_time(b))
      for tag, (n, ms) in prof.items():
        sums[kpack].setdefault(tag, []).append(ms / max(n, 1))
      if kpack:
        out["notes"] = {t: v for t, v in ops.PROFILE_NOTES.items() if "channels" in v}
  for kpack in (False, True):
    key = "on" if kpack else "off"
    out[key] = {"step_ms_median": float(np.median(steps[kpack])),
                "kernel_ms_median": {t: float(np.median(v)) for t, v in sorted(sums[kpack].items())}}
  out["ratio_on_off"] = {t: out["on"]["kernel_ms_median"][t] / out["off"]["kernel_ms_median"][t]
                         for t in out["on"]["kernel_ms_median"] if t in out["off"]["kernel_ms_median"]}
  out["step_ratio_on_off"] = out["on"]["step_ms_median"] / out["off"]["step_ms_median"]
  out["logits_bit_equal"] = bool(np.array_equal(ref[False], ref[True]))
  switch(True)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--B", type=int, default=1024)
  ap.add_argument("--T", type=int, default=20)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--out", default=None)
  ap.add_argument("--ab", choices=["kpack", "k16", "half", "spread", "quarter"], default="kpack")
  args = ap.parse_args()
  dev = torch.device("cuda:0")
  switch = {"k16": nn.set_conv_k16, "half": nn.set_event_half_group,
            "spread": nn.set_event_wave_spread, "quarter": nn.set_event_quarter16}.get(args.ab, nn.set_conv_kpack)
  res = {"ab": args.ab, "B": args.B, "T": args.T, "reps": args.reps, "device": torch.cuda.get_device_name(0), "legs": {}}
  for name, bits, prune, lb, inp in LEGS:
    r = leg(name, bits, prune, lb, inp, args.B, args.T, args.reps, dev, switch)
    res["legs"]["%s_%s" % (name, inp)] = r
    print("%-8s %-4s step %.2f -> %.2f ms (x%.3f)  %s  bit-equal %s" % (
        name, inp, r["off"]["step_ms_median"], r["on"]["step_ms_median"], r["step_ratio_on_off"],
        " ".join("%s %.3f->%.3f x%.3f" % (t, r["off"]["kernel_ms_median"][t], r["on"]["kernel_ms_median"][t], v)
                 for t, v in r["ratio_on_off"].items() if t.startswith("conv3x3")),
        r["logits_bit_equal"]), flush=True)
    torch.cuda.empty_cache()
  res["fallback_counts"] = ops.fallback_counts()
  res["workqueue_stats"] = ops.workqueue_stats()
  res["device_status"] = ops.device_status()
  if args.out:
    with open(args.out, "w") as f:
      json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
  main()
