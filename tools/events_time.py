"""Times the batched event front end (ops.events_bin, csrc/events.hip) at DVS128-Gesture's shape --
128 x 128, T = 20, B = 64, 2^18 uniformly random events per sample -- one launch per output
format in both modes, against the path it replaces for the same frames: B calls of
ops.events_to_frames (zero + scatter + narrow each) followed by ops.pack_frames.  The candidates
alternate in one process, --reps timings each, HIP events around --steps calls.  Checks first that
the loop and the launch give the same bytes.  Prints one JSON line: milliseconds per batch, the bytes
a launch has to read and write, and that traffic over the CALL's time (host validation and upload
included: a lower bound on the kernel's rate) as a fraction of --hbm-gbs.

--augment times the augmenting launch (ops.events_bin(augment=...), snnqp_events_bin_aug) beside the
plain one instead of the loop: every augmentation on, per-row records drawn once -- flips and
polarity swap with probability 1/2, shifts of up to 8 pixels, a drop probability uniform on
[0, 0.5], a cutout of up to a quarter of a side, up to two emptied frames.  Checks first that an
identity record gives the plain launch's bytes.

--mix times the mixing launch (ops.events_bin(mix=...), snnqp_events_bin_mix) with
half the rows mixed with the next row and everything of --augment on for both, against the
composition that gives the same uint8 frames without it: two augmenting launches (the rows, the
partners), a box mask over [B, T, H, W] and a saturating add.  Checks first that both give the same
bytes on the rows without a saturated count, and writes the JSON line to
profiles/events_mix_time.json as well (--out names another file; the other modes write one only
when --out is given).

  python tools/events_time.py [--batch 64] [--frames 20] [--hw 128] [--events 262144]
                              [--steps 10] [--warmup 3] [--reps 3] [--hbm-gbs 8000] [--augment | --mix]
                              [--out profiles/events_mix_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def main(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument("--batch", type=int, default=64)
  ap.add_argument("--frames", type=int, default=20)
  ap.add_argument("--hw", type=int, default=128)
  ap.add_argument("--events", type=int, default=1 << 18)
  ap.add_argument("--steps", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--reps", type=int, default=3)
  ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate the traffic is set against")
  ap.add_argument("--augment", action="store_true", help="time the augmenting launch beside the plain one")
  ap.add_argument("--mix", action="store_true", help="time the mixing launch beside two augmenting ones, a mask and an add")
  ap.add_argument("--out", default=None, help="also write the JSON line to this file (--mix: "
                  "profiles/events_mix_time.json unless given)")
  args = ap.parse_args(argv)
  if args.mix and args.out is None:
    args.out = os.path.join(ROOT, "profiles", "events_mix_time.json")
  assert not (args.augment and args.mix), "--augment and --mix are two runs"
  assert torch.cuda.is_available(), "events_time.py needs the GPU"
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  dev = torch.device("cuda:0")
  B, T, HW, N = args.batch, args.frames, args.hw, args.events
  rng = np.random.Generator(np.random.PCG64(7))
  addrs = np.stack([rng.integers(0, HW, B * N), rng.integers(0, HW, B * N), rng.integers(0, 2, B * N)], 1)
  span = T * 1000                                       # 1 ms windows over a recording of T ms
  times = np.sort(rng.integers(0, span, (B, N)), axis=1).reshape(-1)
  es = ops.EventSet(addrs, times, np.arange(B + 1, dtype=np.int64) * N, (HW, HW), device=dev)
  xyz = [torch.from_numpy(addrs[:, k].astype(np.int32)).to(dev) for k in range(3)]
  rows = list(range(B))
  starts = [-1] * B                                     # windows (-1, 999), (999, 1999), ...: all but the edges

  def loop(fmt):
    frames = torch.stack([ops.events_to_frames(xyz[0][b * N:(b + 1) * N], xyz[1][b * N:(b + 1) * N],
                                               xyz[2][b * N:(b + 1) * N], T, HW, HW) for b in range(B)], 0)
    return frames if fmt is None else ops.pack_frames(frames, fmt)

  def launch(fmt, mode):
    return ops.events_bin(es, rows, T, HW, HW, mode=mode, start=starts, step_us=1000, fmt=fmt)

  def draw_augment():
    w, h = rng.integers(0, HW // 4 + 1, B), rng.integers(0, HW // 4 + 1, B)
    x0, y0 = rng.integers(0, HW - w + 1), rng.integers(0, HW - h + 1)
    n = rng.integers(0, min(2, T) + 1, B)
    f0 = rng.integers(0, T - n + 1)
    return ops.EventAugment(B, flip_x=rng.integers(0, 2, B), flip_y=rng.integers(0, 2, B),
                            swap_polarity=rng.integers(0, 2, B), dx=rng.integers(-8, 9, B), dy=rng.integers(-8, 9, B),
                            cutout=np.stack([x0, y0, x0 + w, y0 + h], 1), frames=np.stack([f0, f0 + n], 1),
                            drop_below=np.floor(rng.random(B) * 0.5 * 2.0 ** 32).astype(np.int64),
                            seed=rng.integers(0, 1 << 32, B))

  def launch_aug(fmt, mode, aug):
    return ops.events_bin(es, rows, T, HW, HW, mode=mode, start=starts, step_us=1000, fmt=fmt, augment=aug)

  if args.mix:
    return _mix(args, ops, es, rows, starts, draw_augment, rng)
  formats = (("u8", None), ("ev4", L.EV4), ("ev1", L.EV1))
  cands = {}
  if args.augment:
    aug, ident = draw_augment(), ops.EventAugment(B)
    for name, fmt in formats:                           # an identity record: the plain launch's bytes
      for mode in ("number", "time"):
        a, b = launch_aug(fmt, mode, ident), launch(fmt, mode)
        assert torch.equal(a.data if fmt else a, b.data if fmt else b), (name, mode)
    for name, fmt in formats:
      for mode in ("number", "time"):
        cands["bin_%s_%s" % (mode, name)] = lambda fmt=fmt, mode=mode: launch(fmt, mode)
        cands["aug_%s_%s" % (mode, name)] = lambda fmt=fmt, mode=mode: launch_aug(fmt, mode, aug)
  else:
    for name, fmt in formats:                           # the same frames, before any timing
      a, b = loop(fmt), launch(fmt, "number")
      assert torch.equal(a.data if fmt else a, b.data if fmt else b), name
    for name, fmt in formats:
      cands["loop_%s" % name] = lambda fmt=fmt: loop(fmt)
      cands["bin_number_%s" % name] = lambda fmt=fmt: launch(fmt, "number")
      cands["bin_time_%s" % name] = lambda fmt=fmt: launch(fmt, "time")
  ms = {k: [] for k in cands}
  for _ in range(args.reps):                            # alternating: every candidate once per round
    for k, fn in cands.items():
      ms[k].append(_time(fn, args.steps, args.warmup))
  out_bytes = {"u8": B * T * HW * HW * 2, "ev4": B * T * HW * HW, "ev1": B * T * ops.frame_units(HW, HW, L.EV1) * 4}
  # The timings are those of a whole ops.events_bin CALL (host validation and upload included), so the
  # rates below are call-level lower bounds, not the kernel's: take the kernel's time from a kernel trace.
  result = {"tool": "events_time", "batch": B, "frames": T, "hw": HW, "events_per_sample": N,
            "timing": "HIP events around whole calls (host share included)",
            "ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}, "per_call": {}}
  rounds, span_n = 0, max(N, 1)                         # rounds of a 64-ary search over N sorted times
  while span_n > 0:
    span_n, rounds = (span_n + 63) // 64 - 1, rounds + 1
  for name, _ in formats:
    for mode in ("number", "time"):
      k = "bin_%s_%s" % (mode, name)
      rd = B * N * 4                                    # the address words ...
      if mode == "time":
        rd += B * T * 2 * rounds * 64 * 4               # ... and the times both searches of a frame probe
      best = min(ms[k])
      result["per_call"][k] = {"read_bytes": rd, "write_bytes": out_bytes[name],
                               "call_gb_per_s": round((rd + out_bytes[name]) / best / 1e6, 1),
                               "call_fraction_of_hbm": round((rd + out_bytes[name]) / best / 1e6 / args.hbm_gbs, 4),
                               "call_events_per_us": round(B * N / best / 1e3, 1)}
    if args.augment:
      for mode in ("number", "time"):
        result.setdefault("augmented_over_plain", {})["%s_%s" % (mode, name)] = round(
            min(ms["aug_%s_%s" % (mode, name)]) / min(ms["bin_%s_%s" % (mode, name)]), 3)
    else:
      result.setdefault("speedup_over_loop", {})[name] = round(min(ms["loop_%s" % name]) / min(ms["bin_number_%s" % name]), 2)
  _emit(result, args.out)


def _emit(result, path):
  line = json.dumps(result)
  print(line)
  if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
      f.write(line + "\n")


def _mix(args, ops, es, rows, starts, draw_augment, rng):
  """--mix: the mixing launch against two augmenting launches, a box mask and a saturating add."""
  B, T, HW = args.batch, args.frames, args.hw
  dev = es.device
  aug, aug2 = draw_augment(), draw_augment()
  partner = np.where(np.arange(B) % 2 == 0, (np.arange(B) + 1) % B, -1)           # half the rows
  w, h = rng.integers(0, HW // 2 + 1, B), rng.integers(0, HW // 2 + 1, B)
  x0, y0 = rng.integers(0, HW - w + 1), rng.integers(0, HW - h + 1)
  n = rng.integers(0, T + 1, B)
  g0 = rng.integers(0, T - n + 1)
  box = np.stack([x0, y0, x0 + w, y0 + h, g0, g0 + n], 1)
  starts2 = [-1] * B
  rows2 = np.where(partner >= 0, partner, 0).tolist()
  box_d = torch.from_numpy(box).to(dev)
  mixed_d = torch.from_numpy(partner >= 0).to(dev)
  ax, at = torch.arange(HW, device=dev), torch.arange(T, device=dev)

  def launch_mix(mode):
    m = ops.EventMix(B, partner=partner, start=starts2 if mode == "time" else None, box=box, augment=aug2)
    return ops.events_bin(es, rows, T, HW, HW, mode=mode, start=starts, step_us=1000, augment=aug, mix=m)

  def composed(mode):
    a = ops.events_bin(es, rows, T, HW, HW, mode=mode, start=starts, step_us=1000, augment=aug)
    b = ops.events_bin(es, rows2, T, HW, HW, mode=mode, start=starts2, step_us=1000, augment=aug2)
    inx = (ax[None] >= box_d[:, 0, None]) & (ax[None] < box_d[:, 2, None])                     # [B, W]
    iny = (ax[None] >= box_d[:, 1, None]) & (ax[None] < box_d[:, 3, None])                     # [B, H]
    inf = (at[None] >= box_d[:, 4, None]) & (at[None] < box_d[:, 5, None]) & mixed_d[:, None]  # [B, T]
    mask = (inf[:, :, None, None] & iny[:, None, :, None] & inx[:, None, None, :])[..., None]
    total = a.masked_fill(mask, 0).to(torch.int16) + b.masked_fill(~mask, 0)
    return total.clamp_(max=255).to(torch.uint8)

  cands = {}
  for mode in ("number", "time"):                       # the same bytes, before any timing
    got, counts = launch_mix(mode)
    want = composed(mode)
    clear = got.reshape(B, -1).amax(1) < 255
    assert bool(clear.any()) and torch.equal(got[clear], want[clear]), mode
    assert bool((counts[mixed_d][:, 1] > 0).any()) and bool((counts[~mixed_d][:, 1] == 0).all())
    cands["mix_%s_u8" % mode] = lambda mode=mode: launch_mix(mode)
    cands["composed_%s_u8" % mode] = lambda mode=mode: composed(mode)
  ms = {k: [] for k in cands}
  for _ in range(args.reps):                            # alternating: every candidate once per round
    for k, fn in cands.items():
      ms[k].append(_time(fn, args.steps, args.warmup))
  result = {"tool": "events_time --mix", "batch": B, "frames": T, "hw": HW, "events_per_sample": args.events,
            "rows_mixed": int((partner >= 0).sum()), "steps": args.steps, "reps": args.reps,
            "timing": "HIP events around whole calls (host share included)",
            "ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
            "mix_over_composed": {mode: round(min(ms["mix_%s_u8" % mode]) / min(ms["composed_%s_u8" % mode]), 3)
                                  for mode in ("number", "time")}}
  _emit(result, args.out)


if __name__ == "__main__":
  main()
