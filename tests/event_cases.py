"""Plain numpy restatement of the two event decoders of examples/input_pipeline.py (split_by =
"number", :142-219, and "time", :63-131) as snnqp_events_bin's contract states them
(include/snnqp.h), one loop per frame, and the streams the event tests share.  Nothing here
imports the package under test."""
import numpy as np

F32 = np.float32
U8, EV1, EV4 = 1, 3, 4                        # include/snnqp.h
FLAG_GT_ONE, FLAG_GT_15 = 8, 32
POLARITIES = (0, 1, 2, 255)                   # anything non-zero is channel 1


def scaled(coord, scale):
  return np.floor(np.asarray(coord).astype(F32) / F32(scale)).astype(np.int64)


def frame_of(addrs, H, W, scale):
  """Counts [H, W, 2] of the given events: out-of-range ones dropped, channel 1 = polarity != 0."""
  out = np.zeros((H, W, 2), np.int64)
  xs, ys = scaled(addrs[:, 0], scale), scaled(addrs[:, 1], scale)
  for x, y, p in zip(xs, ys, addrs[:, 2]):
    if 0 <= x < W and 0 <= y < H:
      out[y, x, 0 if p == 0 else 1] += 1
  return out


def frame_of_fast(addrs, H, W, scale):
  """frame_of for the long streams (np.add.at instead of the Python loop; test_events_cpu checks
  that the two agree)."""
  out = np.zeros((H, W, 2), np.int64)
  xs, ys = scaled(addrs[:, 0], scale), scaled(addrs[:, 1], scale)
  keep = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
  np.add.at(out, (ys[keep], xs[keep], (addrs[keep, 2] != 0).astype(np.int64)), 1)
  return out


def decode_number(addrs, T, H, W, scale=1.0, frame=frame_of_fast):
  n = addrs.shape[0]
  di = n // T
  out = np.zeros((T, H, W, 2), np.int64)
  for f in range(T):
    lo = f * di
    hi = lo + di if f < T - 1 else n
    out[f] = frame(addrs[lo:hi], H, W, scale)
  return out


def decode_time(addrs, times, start, step_us, T, H, W, scale=1.0, frame=frame_of_fast):
  t = np.asarray(times).astype(np.int64)
  out = np.zeros((T, H, W, 2), np.int64)
  for f in range(T):
    lo = int(start) + f * int(step_us)
    inside = (t > lo) & (t < lo + int(step_us))
    out[f] = frame(addrs[inside], H, W, scale)
  return out


def decode_batch(ev, sample, T, H, W, mode, start=None, step_us=None, scale=1.0):
  """Counts int64 [B, T, H, W, 2]: row b decodes sample[b] of the set `ev` (make_set)."""
  out = np.zeros((len(sample), T, H, W, 2), np.int64)
  off = ev["offsets"]
  for b, s in enumerate(sample):
    a, t = ev["addrs"][off[s]:off[s + 1]], ev["times"][off[s]:off[s + 1]]
    out[b] = decode_number(a, T, H, W, scale) if mode == "number" else \
        decode_time(a, t, start[b], step_us, T, H, W, scale)
  return out


def wire(counts, fmt):
  """(array, flag word) of counts [..., H, W, 2] in an output format: uint8 [..., H, W, 2] saturated
  at 255; EV4 uint8 [..., H * W] saturated at 15; EV1 int32 [..., ceil(H * W * 2 / 32)] of bits
  (count != 0), little-endian bit order, frames word-aligned."""
  counts = np.asarray(counts)
  lead, (H, W) = counts.shape[:-3], counts.shape[-3:-1]
  if fmt in (None, U8):
    return np.minimum(counts, 255).astype(np.uint8), 0
  if fmt == EV4:
    c = np.minimum(counts, 15).astype(np.uint8)
    return (c[..., 0] | (c[..., 1] << 4)).reshape(lead + (H * W,)), FLAG_GT_15 if counts.max(initial=0) > 15 else 0
  bits = np.packbits((counts != 0).reshape(lead + (H * W * 2,)), axis=-1, bitorder="little")
  nbytes = (H * W * 2 + 31) // 32 * 4
  bits = np.concatenate([bits, np.zeros(lead + (nbytes - bits.shape[-1],), np.uint8)], -1)
  return np.ascontiguousarray(bits).view(np.int32), FLAG_GT_ONE if counts.max(initial=0) > 1 else 0


# ---- streams -----------------------------------------------------------------------------------

def make_sample(rng, n, H, W, scale=1.0, t_lo=0, t_hi=1000, outside=True, unique=False):
  """n events (addrs int64 [n, 3], times int64 [n], sorted).  Sensor coordinates run a little past
  the scaled frame when `outside` (those events are dropped); `unique`: every (pixel, polarity) at
  most once and polarities 0 / 1 -- a stream that fits EV1 whatever the frames are."""
  if unique:
    assert n <= H * W * 2 and scale == int(scale)
    e = rng.permutation(H * W * 2)[:n]
    addrs = np.stack([(e // 2 % W) * int(scale), (e // 2 // W) * int(scale), e % 2], 1).astype(np.int64)
  else:
    xmax = int(np.ceil(W * scale)) + (2 if outside else 0)
    ymax = int(np.ceil(H * scale)) + (2 if outside else 0)
    addrs = np.stack([rng.integers(0, xmax, n), rng.integers(0, ymax, n),
                      np.asarray(POLARITIES)[rng.integers(0, len(POLARITIES), n)]], 1).astype(np.int64)
  times = np.sort(rng.integers(t_lo, max(t_hi, t_lo + 1), n)).astype(np.int64)
  return addrs, times


def make_set(samples):
  """{addrs [N, 3], times [N], offsets [S + 1]} of a list of (addrs, times) samples."""
  off = np.zeros(len(samples) + 1, np.int64)
  off[1:] = np.cumsum([a.shape[0] for a, _ in samples])
  addrs = np.concatenate([a for a, _ in samples] + [np.zeros((0, 3), np.int64)], 0)
  times = np.concatenate([t for _, t in samples] + [np.zeros((0,), np.int64)], 0)
  return {"addrs": addrs, "times": times, "offsets": off}


def edge_sample(rng, n, H, W, T, start, step_us, scale=1.0):
  """A sample for time mode whose times straddle the T windows from `start` (some before, some
  after) and put events exactly on window edges: on `start` (a lower edge), on every inner edge
  (upper and lower at once) and on start + T * step_us (an upper edge)."""
  addrs, _ = make_sample(rng, n, H, W, scale)
  times = rng.integers(start - step_us // 2 - 1, start + T * step_us + step_us // 2 + 2, n).astype(np.int64)
  edges = start + step_us * np.arange(T + 1)
  k = min(n, T + 1)
  times[:k] = edges[np.r_[0, T, 1:T][:k]] if T > 0 else times[:k]
  order = np.argsort(times, kind="stable")
  return addrs[order], times[order]


def ragged_counts(T):
  """Events per sample the GPU tests cover: none, one, T - 1, T, many."""
  return [0, 1, max(T - 1, 0), T, 1000]


def ragged_set(seed, H, W, T, start, step_us, scale=1.0):
  """One sample per count of ragged_counts(T), each with events on the window edges of
  (start, step_us) as far as it has events."""
  rng = np.random.Generator(np.random.PCG64(seed))
  return make_set([edge_sample(rng, n, H, W, T, start, step_us, scale) for n in ragged_counts(T)])


HOT_N, HOT_COUNT = 70000, 66000
# (count, polarity) of the hot pixel.  Two 16-bit counters packed into a word fail differently by half:
# an overflow of the low half (polarity 0) carries into polarity 1 of the same pixel, an overflow
# of the high half (polarity 1) is lost and leaves count mod 65536 -- which at 66 000 is 464 and
# still saturates every format, so 65 539 (residue 3) stands beside it.  wrapped_halves() models that
# failure and test_events_cpu shows which case exposes it.
HOT_CASES = [(HOT_COUNT, 0), (HOT_COUNT, 1), (65539, 0), (65539, 1)]


def wrapped_halves(counts):
  """What counts [..., 2] read as after passing through two 16-bit halves of one 32-bit word with
  nothing done about overflow (the failure the hot-pixel cases are there to catch)."""
  word = (counts[..., 0] + (counts[..., 1] << 16)) & 0xFFFFFFFF
  return np.stack([word & 0xFFFF, word >> 16], -1)


def hot_sample(rng, H, W, step_us, T=3, count=HOT_COUNT, polarity=1):
  """70 000 events, `count` of them on one pixel and polarity (0, or 255 for channel 1) in the first
  window from origin 0 (and in the first count + 1000 of the stream); no other event touches that
  pixel, so its other polarity stays silent and the hot count is exact."""
  hx, hy = W // 2, H // 3
  hot = np.tile(np.array([[hx, hy, 255 if polarity else 0]], np.int64), (count, 1))
  rest, _ = make_sample(rng, HOT_N - count, H, W, outside=False)
  rest = rest[~((rest[:, 0] == hx) & (rest[:, 1] == hy))]
  rest = np.concatenate([rest, np.tile(rest[:1], (HOT_N - count - rest.shape[0], 1))], 0)
  first = np.concatenate([hot, rest[:1000]], 0)
  first = first[rng.permutation(first.shape[0])]
  addrs = np.concatenate([first, rest[1000:]], 0)
  times = np.concatenate([np.sort(rng.integers(1, step_us, first.shape[0])),
                          np.sort(rng.integers(step_us + 1, T * step_us, rest.shape[0] - 1000))]).astype(np.int64)
  return addrs, times, (hx, hy)
