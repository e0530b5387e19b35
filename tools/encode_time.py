"""Times the rate encoder (ops.rate_encode, csrc/encode.hip) against the torch path it stands in
for, at MNIST's shape -- B = 256, T = 32, K = 784 -- and config C2's -- B = 256 and 4096, T = 20,
K = 2048 --, both kinds and both formats:

  poisson / u8     torch.poisson on the gathered float32 rate tensor [B, T, K], clamp to 15, cast
  bernoulli / u8   torch.bernoulli on it, cast
  bernoulli / bits the same, then ops.pack_bits

The torch path is handed the rates of the same table (RateTable.rates, already on the device as
float32) and the row indices already on the device; the launch validates and uploads its rows per
call, as the input pipeline calls it.  The two draw different spikes -- torch's generator against the
counter hash -- so nothing is compared but the shapes and, loosely, the mean rates.  Each pair is
timed alternately, --reps rounds of --steps calls between HIP events, after --warmup calls; the
median and the spread (min, max) of the rounds are reported per call, in milliseconds.  These are
whole calls (host share included), not kernel times: take those from a kernel trace.

Prints one JSON line and writes it to --out (default profiles/encode_time.json).

  python tools/encode_time.py [--steps 20] [--warmup 5] [--reps 5] [--out profiles/encode_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = (("mnist", 256, 32, 784), ("c2", 256, 20, 2048), ("c2_4096", 4096, 20, 2048))
COUNT_MAX = 15


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


def _stats(v):
  return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--reps", type=int, default=5)
  ap.add_argument("--images", type=int, default=8192, help="images in the resident set")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_time.json"))
  args = ap.parse_args(argv)
  assert torch.cuda.is_available(), "encode_time.py needs the GPU"
  from snnquantprune_amd import ops
  dev = torch.device("cuda:0")
  rng = np.random.Generator(np.random.PCG64(7))
  tables = {"poisson": ops.RateTable("poisson"), "bernoulli": ops.RateTable("bernoulli")}
  result = {"tool": "encode_time", "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
            "timing": "HIP events around whole calls (host share included), ms per call",
            "shapes": {}}
  for name, B, T, K in SHAPES:
    images = ops.ImageSet(rng.integers(0, 256, (args.images, K)).astype(np.uint8), device=dev)
    rows = rng.integers(0, args.images, B)
    rows_d = torch.from_numpy(rows).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    lut = {k: torch.from_numpy(t.rates.astype(np.float32)).to(dev) for k, t in tables.items()}

    def rates(kind):
      r = lut[kind][images.data[rows_d].long()]                       # [B, K] float32
      return r.unsqueeze(1).expand(B, T, K).contiguous()                # the rate tensor torch draws from

    def torch_path(kind, fmt):
      if kind == "poisson":
        return torch.poisson(rates(kind), generator=gen).clamp_(max=COUNT_MAX).to(torch.uint8)
      s = torch.bernoulli(rates(kind).clamp(max=1.0), generator=gen).to(torch.uint8)
      return ops.pack_bits(s) if fmt == "bits" else s

    def launch(kind, fmt):
      return ops.rate_encode(images, rows, T, tables[kind], seed=7, draw=1, fmt=fmt)

    entry = result["shapes"][name] = {"B": B, "T": T, "K": K, "pairs": {}}
    for kind, fmt in (("poisson", "u8"), ("bernoulli", "u8"), ("bernoulli", "bits")):
      a, b = torch_path(kind, fmt), launch(kind, fmt)
      assert tuple(a.shape) == tuple(b.shape) == (B, T, K), (name, kind, fmt)
      da, db = (a.to_dense(), b.to_dense()) if fmt == "bits" else (a, b)
      ma, mb = float(da.float().mean()), float(db.float().mean())
      assert abs(ma - mb) < 0.01 * max(ma, mb) + 1e-3, (name, kind, fmt, ma, mb)   # the same rates, loosely
      ms = {"torch": [], "launch": []}
      for _ in range(args.reps):                                      # alternating
        ms["torch"].append(_time(lambda: torch_path(kind, fmt), args.steps, args.warmup))
        ms["launch"].append(_time(lambda: launch(kind, fmt), args.steps, args.warmup))
      t, l = _stats(ms["torch"]), _stats(ms["launch"])
      out_bytes = B * T * ((K + 31) // 32 * 4 if fmt == "bits" else K)
      entry["pairs"]["%s_%s" % (kind, fmt)] = {
          "torch_ms": t, "launch_ms": l, "torch_over_launch": round(t["median"] / l["median"], 2),
          "mean_value": {"torch": round(ma, 4), "launch": round(mb, 4)},
          "write_bytes": out_bytes, "launch_call_gb_per_s": round(out_bytes / l["median"] / 1e6, 1)}
    del images
  line = json.dumps(result)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
  main()
