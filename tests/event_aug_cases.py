"""Plain numpy restatement of snnqp_events_bin_aug's per-event rules (include/snnqp.h) as a
`frame=` callable for event_cases.decode_number / decode_time, and the record layout the C entry
reads.  The event's index within its sample rides along as a fourth address column: the decoders
slice rows, so it survives.  Nothing here imports the package under test."""
import numpy as np

from tests import event_cases as ec

M32 = np.uint64(0xFFFFFFFF)
IDENTITY = dict(flip_x=0, flip_y=0, swap=0, dx=0, dy=0, cut=(0, 0, 0, 0), frames=(0, 0), drop_below=0, seed=0)


def params(**kw):
  """IDENTITY with some rules set."""
  assert set(kw) <= set(IDENTITY), kw
  return dict(IDENTITY, **kw)


def fmix32(h):
  """The murmur3 finaliser on uint32 values (held in uint64, masked after every product)."""
  h = np.asarray(h).astype(np.uint64) & M32
  h = h ^ (h >> np.uint64(16))
  h = (h * np.uint64(0x85EBCA6B)) & M32
  h = h ^ (h >> np.uint64(13))
  h = (h * np.uint64(0xC2B2AE35)) & M32
  return h ^ (h >> np.uint64(16))


def dropped(index, seed, drop_below):
  """Which events (by index within the sample) rule 5 drops."""
  h = fmix32(fmix32(np.uint64(seed)) ^ (np.asarray(index).astype(np.uint64) & M32))
  return h < np.uint64(drop_below)


def with_index(addrs):
  """addrs [n, 3] -> [n, 4]: the index within the sample as the fourth column."""
  return np.concatenate([addrs, np.arange(addrs.shape[0], dtype=np.int64)[:, None]], 1)


def frame_aug(p):
  """Rules 1-7 for one frame's events (addrs [n, 4], see with_index) under the parameters p."""
  def frame(addrs, H, W, scale):
    out = np.zeros((H, W, 2), np.int64)
    xs, ys = ec.scaled(addrs[:, 0], scale), ec.scaled(addrs[:, 1], scale)
    keep = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)                       # 1
    if p["flip_x"]:
      xs = W - 1 - xs                                                        # 2
    if p["flip_y"]:
      ys = H - 1 - ys
    xs, ys = xs + int(p["dx"]), ys + int(p["dy"])                            # 3
    keep &= (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    x0, y0, x1, y1 = (int(v) for v in p["cut"])
    keep &= ~((xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1))               # 4
    keep &= ~dropped(addrs[:, 3], p["seed"], p["drop_below"])                # 5
    pol = (addrs[:, 2] != 0).astype(np.int64) ^ (1 if p["swap"] else 0)      # 6
    np.add.at(out, (ys[keep], xs[keep], pol[keep]), 1)                       # 7
    return out
  return frame


def decode_aug(addrs, times, p, T, H, W, mode, start=None, step_us=None, scale=1.0):
  """Counts int64 [T, H, W, 2] of one sample under p: the slices are those of the untouched sample,
  frames [f0, f1) come out empty."""
  a4 = with_index(addrs)
  out = ec.decode_number(a4, T, H, W, scale, frame=frame_aug(p)) if mode == "number" else \
      ec.decode_time(a4, times, start, step_us, T, H, W, scale, frame=frame_aug(p))
  out[max(int(p["frames"][0]), 0):max(int(p["frames"][1]), 0)] = 0
  return out


def decode_batch_aug(ev, sample, plist, T, H, W, mode, start=None, step_us=None, scale=1.0):
  """Counts int64 [B, T, H, W, 2]: row b decodes sample[b] of the set `ev` under plist[b]."""
  out = np.zeros((len(sample), T, H, W, 2), np.int64)
  off = ev["offsets"]
  for b, s in enumerate(sample):
    a, t = ev["addrs"][off[s]:off[s + 1]], ev["times"][off[s]:off[s + 1]]
    out[b] = decode_aug(a, t, plist[b], T, H, W, mode, None if start is None else start[b], step_us, scale)
  return out


def columns(plist):
  """The parameter dicts of a batch as per-row arrays, named as ops.EventAugment names them."""
  col = lambda k: np.array([int(p[k]) for p in plist], np.int64)
  return dict(flip_x=col("flip_x"), flip_y=col("flip_y"), swap_polarity=col("swap"), dx=col("dx"), dy=col("dy"),
              cutout=np.array([p["cut"] for p in plist], np.int64).reshape(len(plist), 4),
              frames=np.array([p["frames"] for p in plist], np.int64).reshape(len(plist), 2),
              drop_below=col("drop_below"), seed=col("seed"))


def from_columns(c):
  """The inverse of columns(), from anything with those attributes or keys (an ops.EventAugment)."""
  get = (lambda k: np.asarray(c[k])) if isinstance(c, dict) else (lambda k: np.asarray(getattr(c, k)))
  n = get("dx").shape[0]
  return [dict(flip_x=int(get("flip_x")[b]), flip_y=int(get("flip_y")[b]), swap=int(get("swap_polarity")[b]),
               dx=int(get("dx")[b]), dy=int(get("dy")[b]), cut=tuple(int(v) for v in get("cutout")[b]),
               frames=tuple(int(v) for v in get("frames")[b]), drop_below=int(get("drop_below")[b]),
               seed=int(get("seed")[b])) for b in range(n)]


def records(plist):
  """snnqp_event_aug_t records, int32 [B, 12] (unsigned fields as bit patterns), written from the
  header's layout: flags, dx, dy, cut_x0, cut_y0, cut_x1, cut_y1, f0, f1, drop_below, seed, reserved."""
  r = np.zeros((len(plist), 12), np.int64)
  for b, p in enumerate(plist):
    r[b] = [int(bool(p["flip_x"])) | int(bool(p["flip_y"])) << 1 | int(bool(p["swap"])) << 2, p["dx"], p["dy"],
            *p["cut"], *p["frames"], p["drop_below"], p["seed"], 0]
  return (r & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
