"""Input pipeline -- mirror of examples/input_pipeline.py for three kinds of source (there is no
tfds and no network on the boxes this runs on):

  * a FRAME source: event-count frames in host memory (a `.npz` with `dvs_matrix`
    [N, T, H, W, 2] uint8 and `label` [N], e.g. synthetic Poisson frames), eval only, fed
    through the host ring of feed.py;
  * an EVENT source: the raw recordings (`addrs` [E, 3] x, y, polarity; `times` [E]
    microseconds; `offsets` [N + 1]; `label` [N]; `sensor_size`), eval and training.  The
    rank's slice goes resident on the device as an `ops.EventSet` and every batch is one
    `ops.events_bin` launch (preprocess_data_number, :142-219, or preprocess_data_time,
    :63-139): nothing crosses PCIe per batch, so there is no host ring;
  * an IMAGE source: static images (`image` [N, ...] uint8 and `label` [N], no `dvs_matrix`),
    eval and training -- the `mnist` branch of :286-296, which Poisson-encodes each image into
    `num_frames` count frames.  The rank's slice goes resident as an `ops.ImageSet` and every
    batch is one `ops.rate_encode` launch into [B, T, K] (`config.encoding`, `feed_format`
    "u8" | "bits", `image_layout` "flat" | "frames": ImagePlan); no host ring either.

What is kept from the reference:
  * every PROCESS takes a contiguous slice of the split, `split_size = N // processes`,
    `start = process_index * split_size` (input_pipeline.py:245-254) -- one process per
    GPU here, so that slice is also the device shard (:38-46);
  * eval batches of `config.eval_batch_size // processes`, remainder dropped, repeated
    (:321-329);
  * two batches prefetched towards the device (:17-27) -- `feed.DeviceFeeder` (frame sources).
What is new: `config.feed_format` ("u8" | "ev1" | "ev4") picks the wire format of the
frames (include/snnqp.h); with `cache` the slice is packed once into page-locked memory.
"""

from __future__ import annotations

from typing import Any, Dict, Iterator

import numpy as np
import torch

from . import _lib as L
from . import feed, ops

FEED_FORMATS = {"u8": None, "ev1": L.EV1, "ev4": L.EV4}
EVENT_KEYS = ("addrs", "times", "offsets", "label", "sensor_size")


def is_event_source(source) -> bool:
  return all(k in source for k in EVENT_KEYS)


def is_image_source(source) -> bool:
  return "image" in source and "label" in source and "dvs_matrix" not in source and not is_event_source(source)


def _open_source(source):
  """The arrays of a source as a dict, unvalidated (a `.npz` path is read)."""
  if isinstance(source, str):
    with np.load(source) as z:
      return {k: z[k] for k in z.files}
  return source


def load_source(source) -> Dict[str, np.ndarray]:
  source = _open_source(source)
  if is_event_source(source):
    off, y = np.asarray(source["offsets"]).reshape(-1), np.asarray(source["label"]).reshape(-1)
    if off.shape[0] != y.shape[0] + 1:
      raise ValueError("an event source needs offsets [N + 1] for its N labels, got %s / %s"
                       % (off.shape, y.shape))
    hw = np.asarray(source["sensor_size"]).reshape(-1)
    return {"addrs": np.asarray(source["addrs"]), "times": np.asarray(source["times"]),
            "offsets": off.astype(np.int64), "label": y.astype(np.int8),
            "sensor_size": np.array([int(hw[0]), int(hw[-1])], np.int64)}
  if is_image_source(source):
    x, y = np.asarray(source["image"]), np.asarray(source["label"]).reshape(-1)
    if x.dtype != np.uint8:
      raise ValueError("an image source holds uint8 images, got %s" % (x.dtype,))
    if x.ndim < 1 or x.shape[0] != y.shape[0]:
      raise ValueError("image must be [N, ...] with one label per image, got %s / %s" % (x.shape, y.shape))
    return {"image": x, "label": y.astype(np.int8)}
  x, y =np.asarray(source["dvs_matrix"]), np.asarray(source["label"])
  if x.ndim != 5 or x.shape[-1] != 2 or x.shape[0] != y.shape[0]:
    raise ValueError("dvs_matrix must be [N, T, H, W, 2] with one label per sample, got %s / %s"
                     % (x.shape, y.shape))
  return {"dvs_matrix": x, "label": y.astype(np.int8)}            # :271 casts labels to int8


def _cfg(config, key, default=None):
  if hasattr(config, "get"):
    return config.get(key, default)
  return getattr(config, key, default)


class EventPlan:
  """Everything about an event split that is decided on the host, without a device: the frame
  geometry, the decoder's constants and, per batch, which samples are decoded and from which
  window origin.  Config keys are the reference's: split_by, num_frames, resolution_scale,
  time_step (ms), input_scale, train_chunk_size / test_chunk_size (ms), batch_size /
  eval_batch_size, seed, feed_format.

  Where this differs from the reference, knowingly:
    * the window origin of split_by = "time" is uniform on [t_min, max(t_min, t_max - 2 * chunk *
      1000)] as there (:76-85) -- a 62-bit draw reduced modulo the range --, but from a
      torch.Generator seeded with config.seed (+ rank); the reference draws it with TensorFlow's
      global generator, at eval as well (:268-275, shuffle=True), which cannot be reproduced.
      The eval split re-seeds at the start of every pass, so an eval is reproducible;
    * the train split takes a fresh permutation of the rank's slice per epoch from the same
      generator; the reference shuffles through a buffer of 16 batches with seed 0 (:323), an
      order that depends on the buffer and is not reproduced either;
    * counts saturate at 255 (uint8), as ops.events_to_frames' do; the reference keeps int32.

  Augmentation (train split only; the reference has none).  `config.augment` is a mapping of the
  keys below; the eval split ignores it, and absent or with every value 0 the plan draws nothing
  for it: its generator stream and its batches are those of a plan without the key.  Otherwise
  every batch -- a skipped one too -- draws from `plan.gen`, after the batch's origins, one array
  of `per` values per line, in this order, a key whose value is 0 drawing nothing:
    flip_x         probability: 1 draw (float64 uniform < p)
    flip_y         probability: 1 draw
    swap_polarity  probability: 1 draw
    shift          whole pixels: dx, then dy, uniform on [-shift, shift]
    drop_event     probability: u (float64 uniform), the row's p = u * drop_event and drop_below =
                   floor(p * 2^32) in float64; then seed, 32 bits
    cutout         largest side as a fraction of the frame: width uniform on 0 .. floor(cutout * W),
                   height on 0 .. floor(cutout * H), then x0 on 0 .. W - width, y0 on 0 .. H - height
    drop_frames    whole frames: n uniform on 0 .. drop_frames, then f0 on 0 .. T - n
  Integers are 62-bit draws reduced modulo the range, as the origins are.  `augmented_batches`
  yields the batch's ops.EventAugment beside the indices and origins; `batches` yields the pairs.

  Mixing (train split only).  `config.mix = dict(prob=p, size=s[, frames=m])` mixes
  row b of a batch with row (b + 1) mod per of the same batch -- no second permutation --, which
  keeps its own origin and its own augmentation record: inside the row's box the partner's events
  are counted, outside it the row's own.  p and s lie in [0, 1], m is a whole number in 0..T, and
  the per-rank batch must hold at least 2 rows.  The eval split ignores the key and an absent key
  draws nothing.  Otherwise every batch -- a skipped one too -- draws after its augmentation, one
  array of `per` values per line:
    mixed          1 draw (float64 uniform < p)
    box            width uniform on 0 .. floor(s * W), height on 0 .. floor(s * H), then x0 on
                   0 .. W - width, y0 on 0 .. H - height (the cutout's draws)
    frames         with `frames` only: n uniform on 0 .. m, then g0 on 0 .. T - n; without it the
                   box spans all T frames
  `mixed_batches` yields the batch's ops.EventMix as a fourth element.
  """

  AUGMENT_KEYS = ("flip_x", "flip_y", "swap_polarity", "shift", "drop_event", "cutout", "drop_frames")
  MIX_KEYS = ("prob", "size", "frames")

  def __init__(self, config, sensor_size, counts_per_rank: int, train: bool, rank: int = 0, world: int = 1):
    self.train = bool(train)
    self.split_by = _cfg(config, "split_by", "number")
    if self.split_by not in ("number", "time"):
      raise ValueError("split_by must be 'number' or 'time', got %r" % (self.split_by,))
    self.T = int(_cfg(config, "num_frames"))
    self.scale = float(_cfg(config, "resolution_scale", 1))
    hw = np.asarray(sensor_size).reshape(-1)
    self.H, self.W = int(int(hw[0]) // self.scale), int(int(hw[-1]) // self.scale)   # :87, :156
    name = _cfg(config, "feed_format", "u8")
    if name not in FEED_FORMATS:
      raise ValueError("feed_format must be one of %s, got %r" % (sorted(FEED_FORMATS), name))
    self.fmt = FEED_FORMATS[name]
    self.divisor = None                                            # float32 batches: counts / divisor
    self.step_us = self.chunk_ms = None
    if self.split_by == "time":
      time_step = _cfg(config, "time_step")
      if time_step != int(time_step) or int(time_step) <= 0:
        raise ValueError("time_step must be a positive whole number of ms, got %r" % (time_step,))
      self.step_us = int(time_step) * 1000                         # :93-94
      self.chunk_ms = int(_cfg(config, "train_chunk_size" if train else "test_chunk_size"))  # :264, :273
      product = float(time_step) * float(_cfg(config, "input_scale", 1))                     # :137
      if product != 1.0:
        self.divisor = np.float32(product)
    if self.fmt is not None and (self.divisor is not None or train):
      raise ValueError("feed_format %r holds integer counts: %s needs feed_format 'u8'"
                       % (name, "the training split" if train else "time_step * input_scale != 1"))
    total = int(_cfg(config, "batch_size" if train else "eval_batch_size"))
    self.per = total // world                                      # :333, :337
    self.n = int(counts_per_rank)
    if self.per < 1 or self.n < self.per:
      raise ValueError("%s %d over %d processes needs at least %d samples per process, the split has %d"
                       % ("batch_size" if train else "eval_batch_size", total, world, max(self.per, 1), self.n))
    self.nb = self.n // self.per                                   # drop_remainder=True
    self.seed = int(_cfg(config, "seed", 0)) + int(rank)
    self.gen = torch.Generator()
    self.gen.manual_seed(self.seed)
    aug = self._augment_config(_cfg(config, "augment"))            # validated for either split
    self.augment = {k: v for k, v in aug.items() if v} if self.train else {}
    mix = self._mix_config(_cfg(config, "mix"))                    # validated for either split
    self.mix = mix if self.train else None
    if self.mix is not None and self.per < 2:
      raise ValueError("mix pairs every row with the next row of its batch: batch_size %d over %d processes "
                       "leaves %d row per process, it needs at least 2" % (total, world, self.per))

  def _mix_config(self, mix):
    if mix is None:
      return None
    form = "mix must be a mapping of prob, size and optionally frames"
    if not hasattr(mix, "keys"):
      raise ValueError("%s, got %r" % (form, mix))
    keys = set(mix.keys())
    if not {"prob", "size"} <= keys <= set(self.MIX_KEYS):
      raise ValueError("%s, got the keys %s" % (form, sorted(keys, key=str)))
    out = {}
    for k in ("prob", "size"):
      v = mix[k]
      try:
        ok = not isinstance(v, bool) and 0.0 <= float(v) <= 1.0      # (a NaN fails both comparisons)
      except (TypeError, ValueError):
        ok = False
      if not ok:
        raise ValueError("mix.%s must lie in [0, 1], got %r" % (k, v))
      out[k] = float(v)
    if "frames" in keys:
      v = mix["frames"]
      try:
        ok = not isinstance(v, bool) and v == int(v) and 0 <= int(v) <= self.T
      except (TypeError, ValueError, OverflowError):
        ok = False
      if not ok:
        raise ValueError("mix.frames must be a whole number in 0..%d, got %r" % (self.T, v))
      out["frames"] = int(v)
    return out

  def _augment_config(self, aug) -> Dict[str, Any]:
    if aug is None:
      return {}
    if not hasattr(aug, "keys"):
      raise ValueError("augment must be a mapping of %s, got %r" % (list(self.AUGMENT_KEYS), aug))
    unknown = sorted(set(aug.keys()) - set(self.AUGMENT_KEYS))
    if unknown:
      raise ValueError("augment has unknown keys %s (known: %s)" % (unknown, list(self.AUGMENT_KEYS)))
    out = {}
    for k in self.AUGMENT_KEYS:
      if k not in aug.keys():
        continue
      v = aug[k]
      if k in ("shift", "drop_frames"):
        limit = ops.EVENT_SHIFT_MAX if k == "shift" else self.T
        if isinstance(v, bool) or v != int(v) or not 0 <= int(v) <= limit:
          raise ValueError("augment.%s must be a whole number in 0..%d, got %r" % (k, limit, v))
        out[k] = int(v)
      else:
        if isinstance(v, bool) or not 0.0 <= float(v) <= 1.0:        # (a NaN fails both comparisons)
          raise ValueError("augment.%s must lie in [0, 1], got %r" % (k, v))
        out[k] = float(v)
    return out

  def _uniform_int(self, lo, hi) -> np.ndarray:
    """One integer per row, uniform on [lo, hi] (arrays or scalars), as draw_starts draws."""
    lo = np.broadcast_to(np.asarray(lo, np.int64), (self.per,))
    hi = np.broadcast_to(np.asarray(hi, np.int64), (self.per,))
    r = torch.randint(0, 1 << 62, (self.per,), generator=self.gen, dtype=torch.int64).numpy()
    return (lo + r % (hi - lo + 1)).astype(np.int64)

  def _uniform(self) -> np.ndarray:
    return torch.rand(self.per, generator=self.gen, dtype=torch.float64).numpy()

  def draw_augment(self):
    """The batch's ops.EventAugment in the order the class docstring fixes, or None for a plan that
    does not augment (nothing is drawn then)."""
    a = self.augment
    if not a:
      return None
    kw = {}
    for k in ("flip_x", "flip_y", "swap_polarity"):
      if k in a:
        kw[k] = self._uniform() < a[k]
    if "shift" in a:
      kw["dx"] = self._uniform_int(-a["shift"], a["shift"])
      kw["dy"] = self._uniform_int(-a["shift"], a["shift"])
    if "drop_event" in a:
      p = self._uniform() * a["drop_event"]
      kw["drop_below"] = np.minimum(np.floor(p * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.int64)
      kw["seed"] = torch.randint(0, 1 << 32, (self.per,), generator=self.gen, dtype=torch.int64).numpy()
    if "cutout" in a:
      w = self._uniform_int(0, int(np.floor(a["cutout"] * self.W)))
      h = self._uniform_int(0, int(np.floor(a["cutout"] * self.H)))
      x0, y0 = self._uniform_int(0, self.W - w), self._uniform_int(0, self.H - h)
      kw["cutout"] = np.stack([x0, y0, x0 + w, y0 + h], 1)
    if "drop_frames" in a:
      n = self._uniform_int(0, a["drop_frames"])
      f0 = self._uniform_int(0, self.T - n)
      kw["frames"] = np.stack([f0, f0 + n], 1)
    return ops.EventAugment(self.per, **kw)

  def draw_mix(self, idx, starts, aug):
    """The batch's ops.EventMix in the order the class docstring fixes, or None for a plan that does
    not mix (nothing is drawn then).  The partner of row b is row (b + 1) mod per: its index, its
    origin and its record of `aug` are the batch's own, rolled by one."""
    m = self.mix
    if m is None:
      return None
    mixed = self._uniform() < m["prob"]
    w = self._uniform_int(0, int(np.floor(m["size"] * self.W)))
    h = self._uniform_int(0, int(np.floor(m["size"] * self.H)))
    x0, y0 = self._uniform_int(0, self.W - w), self._uniform_int(0, self.H - h)
    if "frames" in m:
      n = self._uniform_int(0, m["frames"])
      g0 = self._uniform_int(0, self.T - n)
      g1 = g0 + n
    else:
      g0, g1 = np.zeros(self.per, np.int64), np.full(self.per, self.T, np.int64)
    roll = lambda a: np.roll(np.asarray(a), -1, axis=0)                           # noqa: E731
    aug2 = None if aug is None else ops.EventAugment(
        self.per, flip_x=roll(aug.flip_x), flip_y=roll(aug.flip_y), swap_polarity=roll(aug.swap_polarity),
        dx=roll(aug.dx), dy=roll(aug.dy), cutout=roll(aug.cutout), frames=roll(aug.frames),
        drop_below=roll(aug.drop_below), seed=roll(aug.seed))
    return ops.EventMix(self.per, partner=np.where(mixed, roll(idx), -1), start=None if starts is None else roll(starts),
                        box=np.stack([x0, y0, x0 + w, y0 + h, g0, g1], 1), augment=aug2)

  def start_range(self, t_min, t_max):
    """[tbegin, tend] of the window origin, both inclusive (:76-77)."""
    t_min, t_max = np.asarray(t_min, np.int64), np.asarray(t_max, np.int64)
    return t_min, np.maximum(t_min, t_max - 2 * self.chunk_ms * 1000)

  def draw_starts(self, t_min, t_max) -> np.ndarray:
    """One origin per row, uniform on start_range (tf.random.uniform(minval=tbegin, maxval=tend + 1))."""
    lo, hi = self.start_range(t_min, t_max)
    r = torch.randint(0, 1 << 62, (lo.shape[0],), generator=self.gen, dtype=torch.int64).numpy()
    return (lo + r % (hi - lo + 1)).astype(np.int64)

  def batches(self, t_min=None, t_max=None, skip: int = 0):
    """Endless (indices, starts) pairs: int64 sample indices within the rank's slice, and the
    window origins of those rows (None for split_by = "number").  `skip`: the first `skip` pairs
    are drawn -- permutations and origins alike, so the generator ends up where a consumer of them
    leaves it -- and not yielded: what follows is what a fresh plan yields from its skip-th pair
    on.  (An eval pass re-seeds, so only skip modulo the pass is drawn there.)"""
    for idx, starts, _ in self.augmented_batches(t_min, t_max, skip):
      yield idx, starts

  def augmented_batches(self, t_min=None, t_max=None, skip: int = 0):
    """`batches` with each batch's ops.EventAugment as a third element (None when the plan does not
    augment), drawn after the batch's origins -- for a skipped batch too."""
    for idx, starts, aug, _ in self.mixed_batches(t_min, t_max, skip):
      yield idx, starts, aug

  def mixed_batches(self, t_min=None, t_max=None, skip: int = 0):
    """`augmented_batches` with each batch's ops.EventMix as a fourth element (None when the plan
    does not mix), drawn after the batch's augmentation -- for a skipped batch too."""
    skip = int(skip)
    if skip < 0:
      raise ValueError("skip must be >= 0, got %d" % skip)
    if not self.train:
      skip %= self.nb
    while True:
      if self.train:
        order = torch.randperm(self.n, generator=self.gen).numpy()
      else:
        order = np.arange(self.n)
        self.gen.manual_seed(self.seed)                            # every eval pass draws the same origins
      for i in range(self.nb):
        idx = order[i * self.per:(i + 1) * self.per]
        starts = self.draw_starts(np.asarray(t_min)[idx], np.asarray(t_max)[idx]) \
            if self.split_by == "time" else None
        aug = self.draw_augment()
        mix = self.draw_mix(idx, starts, aug)
        if skip > 0:
          skip -= 1
          continue
        yield idx, starts, aug, mix


def create_event_split(data, config, train: bool, rank: int = 0, world: int = 1,
                       device=None, skip: int = 0) -> Iterator[Dict[str, Any]]:
  """The batches of an event source, decoded on `device` (see EventPlan for the rules), from the
  `skip`-th on: the plan is advanced on the host and nothing is launched for a skipped batch."""
  device = torch.device("cuda" if device is None else device)
  n = data["label"].shape[0]
  split = n // world                                               # :245-254
  lo = rank * split
  plan = EventPlan(config, data["sensor_size"], split, train, rank, world)
  off = data["offsets"]
  e0, e1 = int(off[lo]), int(off[lo + split])
  events = ops.EventSet(data["addrs"][e0:e1], data["times"][e0:e1], off[lo:lo + split + 1] - e0,
                        data["sensor_size"], device=device)
  labels = torch.from_numpy(np.ascontiguousarray(data["label"][lo:lo + split])).to(device)

  # a device divisor: torch turns a division by a host scalar into a multiplication by its reciprocal
  divisor = None if plan.divisor is None else torch.full((), float(plan.divisor), dtype=torch.float32, device=device)

  def gen():
    for idx, starts, aug, mix in plan.mixed_batches(events.t_min, events.t_max, skip):
      x = ops.events_bin(events, idx, plan.T, plan.H, plan.W, mode=plan.split_by, start=starts,
                         step_us=plan.step_us, scale=plan.scale, fmt=plan.fmt, augment=aug, mix=mix)
      if mix is not None:
        x, counts = x
      if plan.divisor is not None:
        x = x.to(torch.float32) / divisor                          # :134-137
      batch = {"dvs_matrix": x, "label": labels[torch.from_numpy(idx).to(device)]}
      if mix is not None:
        # the partner's label (an unmixed row: its own) and the share of the row's own events among
        # those counted, nA / (nA + nB) in float64, rounded once; 1 where nothing was counted
        batch["label_mix"] = labels[torch.from_numpy(np.where(mix.partner >= 0, mix.partner, idx)).to(device)]
        n = counts.to(torch.float64)
        total = n.sum(1)
        batch["mix_weight"] = torch.where(total > 0, n[:, 0] / total, torch.ones_like(total)).to(torch.float32)
      yield batch
  return gen()


class ImagePlan:
  """Everything about an image split that is decided on the host, without a device: the encoder,
  the batch's format and layout and, per batch, which images are encoded, under which ids and with
  which draw.  Config keys: num_frames (T), seed, batch_size / eval_batch_size, encoding (a mapping
  of kind, gain, mean, std: ops.RateTable; default kind "poisson", the reference's encoder),
  feed_format ("u8" | "bits"), image_layout ("flat" | "frames").

    * eval: the batches in order, remainder dropped, repeated; draw = 0 always, so every
      evaluation of a sample sees the same spikes;
    * train: a fresh permutation of the rank's slice per epoch from a torch.Generator seeded
      `seed + rank`, as EventPlan draws it; draw = 1 + the epoch's index, so every epoch sees fresh
      spikes and never the evaluation's;
    * the id that goes into the hash is `lo + index`, the sample's index in the whole source
      (lo = rank * counts_per_rank): what a sample is encoded as does not depend on the world size.

  The reference encodes with tf.random.poisson under TensorFlow's global generator (and shuffles
  through a buffer with seed 0), which cannot be reproduced; see DESIGN.md 16."""

  FORMATS = ("u8", "bits")
  LAYOUTS = ("flat", "frames")
  ENCODING_KEYS = ("kind", "gain", "mean", "std")

  def __init__(self, config, item_shape, counts_per_rank: int, train: bool, rank: int = 0, world: int = 1):
    self.train = bool(train)
    self.T = int(_cfg(config, "num_frames"))
    self.item_shape = tuple(int(d) for d in item_shape)
    self.K = int(np.prod(self.item_shape, dtype=np.int64)) if self.item_shape else 1
    enc = _cfg(config, "encoding")
    if enc is None:
      enc = {}
    if not hasattr(enc, "keys"):
      raise ValueError("encoding must be a mapping of %s, got %r" % (list(self.ENCODING_KEYS), enc))
    unknown = sorted(set(enc.keys()) - set(self.ENCODING_KEYS))
    if unknown:
      raise ValueError("encoding has unknown keys %s (known: %s)" % (unknown, list(self.ENCODING_KEYS)))
    self.table = ops.RateTable(enc.get("kind", "poisson"), gain=enc.get("gain", 1.0), mean=enc.get("mean", 0.0),
                               std=enc.get("std", 1.0))
    self.fmt = _cfg(config, "feed_format", "u8")
    if self.fmt not in self.FORMATS:
      raise ValueError("feed_format must be one of %s, got %r" % (sorted(self.FORMATS), self.fmt))
    if self.fmt == "bits" and (self.table.kind != "bernoulli" or train):
      raise ValueError("feed_format %r holds spikes: %s needs feed_format 'u8'"
                       % (self.fmt, "the training split" if train else "encoding kind %r" % (self.table.kind,)))
    self.layout = _cfg(config, "image_layout", "flat")
    if self.layout not in self.LAYOUTS:
      raise ValueError("image_layout must be one of %s, got %r" % (sorted(self.LAYOUTS), self.layout))
    if self.layout == "frames":
      if len(self.item_shape) != 3 or self.item_shape[-1] != 2:
        raise ValueError("image_layout 'frames' needs images of [N, H, W, 2], got items of %s" % (self.item_shape,))
      if self.fmt != "u8":
        raise ValueError("image_layout 'frames' yields uint8 [B, T, H, W, 2] batches: it needs feed_format 'u8'")
    aug = _cfg(config, "augment")
    if aug is not None and not (hasattr(aug, "keys") and len(aug.keys()) == 0):
      raise ValueError("augment is for event sources: an image source has no event to flip, shift or drop")
    if _cfg(config, "mix") is not None:
      raise ValueError("mix is for event sources: an image source has no events of two recordings to mix")
    total = int(_cfg(config, "batch_size" if train else "eval_batch_size"))
    self.per = total // world
    self.n = int(counts_per_rank)
    if self.per < 1 or self.n < self.per:
      raise ValueError("%s %d over %d processes needs at least %d samples per process, the split has %d"
                       % ("batch_size" if train else "eval_batch_size", total, world, max(self.per, 1), self.n))
    self.nb = self.n // self.per                                   # drop_remainder=True
    self.lo = int(rank) * self.n
    self.seed = int(_cfg(config, "seed", 0))                       # the encoder's: the same on every rank
    self.gen = torch.Generator()
    self.gen.manual_seed(self.seed + int(rank))

  @property
  def batch_shape(self):
    """The shape of a yielded batch (PackedSpikes: the logical one)."""
    return (self.per, self.T) + (self.item_shape if self.layout == "frames" else (self.K,))

  def batches(self, skip: int = 0):
    """Endless (indices, ids, draw) triples: int64 sample indices within the rank's slice, their
    ids in the whole source and the batch's draw.  `skip`: the first `skip` triples are drawn --
    the permutations, so the generator ends up where a consumer of them leaves it -- and not
    yielded: what follows is what a fresh plan yields from its skip-th triple on.  (An eval pass
    draws nothing, so only skip modulo the pass counts there.)"""
    skip = int(skip)
    if skip < 0:
      raise ValueError("skip must be >= 0, got %d" % skip)
    if not self.train:
      skip %= self.nb
    epoch = 0
    while True:
      order = torch.randperm(self.n, generator=self.gen).numpy() if self.train else np.arange(self.n)
      draw = 1 + epoch if self.train else 0
      for i in range(self.nb):
        if skip > 0:
          skip -= 1
          continue
        idx = order[i * self.per:(i + 1) * self.per].astype(np.int64)
        yield idx, self.lo + idx, draw
      epoch += 1


def create_image_split(data, config, train: bool, rank: int = 0, world: int = 1,
                       device=None, skip: int = 0) -> Iterator[Dict[str, Any]]:
  """The batches of an image source, rate-encoded on `device` (see ImagePlan for the rules), from
  the `skip`-th on: the plan is advanced on the host and nothing is launched for a skipped batch.
  The rank's slice goes resident as an ops.ImageSet and every batch is one ops.rate_encode launch:
  uint8 [B, T, K] ("flat"), the same memory seen as [B, T, H, W, 2] ("frames"), or batch-major
  PackedSpikes [B, T, K] (feed_format "bits": the layout DenseSNN's packed input takes)."""
  device = torch.device("cuda" if device is None else device)
  x = data["image"]
  n = data["label"].shape[0]
  split = n // world                                               # :245-254
  lo = rank * split
  plan = ImagePlan(config, x.shape[1:], split, train, rank, world)
  images = ops.ImageSet(x[lo:lo + split], device=device)
  labels = torch.from_numpy(np.ascontiguousarray(data["label"][lo:lo + split])).to(device)

  def gen():
    for idx, ids, draw in plan.batches(skip):
      b = ops.rate_encode(images, idx, plan.T, plan.table, seed=plan.seed, draw=draw, sample_id=ids, fmt=plan.fmt)
      if plan.layout == "frames":
        b = b.view(plan.batch_shape)
      yield {"dvs_matrix": b, "label": labels[torch.from_numpy(idx).to(device)]}
  return gen()


def image_input_shape(data, config):
  """The dummy input a model is initialised from for an image source: [1, T, K] ("flat") or
  [1, T, H, W, 2] ("frames")."""
  item = tuple(int(d) for d in data["image"].shape[1:])
  if _cfg(config, "image_layout", "flat") == "frames":
    return (1, int(_cfg(config, "num_frames"))) + item
  return (1, int(_cfg(config, "num_frames")), int(np.prod(item, dtype=np.int64)) if item else 1)


def create_split(source, config, train: bool, cache: bool, rank: int = 0, world: int = 1,
                 pin: bool = False, device=None, skip: int = 0) -> Iterator[Dict[str, Any]]:
  """Iterator of this process's batches (input_pipeline.py:222-345), from the `skip`-th on: host
  batches of a frame source, device batches of an event or image source."""
  source = _open_source(source)
  if is_event_source(source):
    return create_event_split(load_source(source), config, train, rank, world, device, skip)
  if is_image_source(source):
    return create_image_split(load_source(source), config, train, rank, world, device, skip)
  if _cfg(config, "mix") is not None:
    raise ValueError("mix is for event sources: a frame source holds counts, which no longer know their events")
  if train:
    raise NotImplementedError("the training split (shuffle, augmentation) is out of scope")
  data = load_source(source)
  n = data["label"].shape[0]
  split = n // world                                               # :250-254
  lo = rank * split
  x, y = data["dvs_matrix"][lo:lo + split], data["label"][lo:lo + split]
  per = config.eval_batch_size // world                            # :326
  if per < 1 or split < per:
    raise ValueError("eval_batch_size %d over %d processes needs at least %d samples per "
                     "process, the split has %d" % (config.eval_batch_size, world, max(per, 1), split))
  fmt = FEED_FORMATS[config.get("feed_format", "u8") if hasattr(config, "get") else "u8"]

  def wire(frames):
    if fmt is None:
      return torch.from_numpy(np.ascontiguousarray(frames))
    return ops.pack_frames_host(frames.astype(np.uint8, copy=False), fmt)

  nb = split // per                                                # drop_remainder=True
  if cache:                 # ds.cache(): decode (here: pack) the slice once
    wx = wire(x[:nb * per])
    wy = torch.from_numpy(np.ascontiguousarray(y[:nb * per]))
    if pin:
      wx, wy = feed.pinned_like(wx), feed.pinned_like(wy)

  def gen():
    first = int(skip) % nb
    while True:                                                    # ds.repeat()
      for i in range(first, nb):
        if cache:
          bx = wx.narrow(0, i * per, per) if isinstance(wx, ops.PackedFrames) else wx[i * per:(i + 1) * per]
          by = wy[i * per:(i + 1) * per]
        else:
          bx = wire(x[i * per:(i + 1) * per])
          by = torch.from_numpy(np.ascontiguousarray(y[i * per:(i + 1) * per]))
        yield {"dvs_matrix": bx, "label": by}
      first = 0
  return gen()


def create_input_iter(source, config, train: bool, cache: bool, rank: int = 0, world: int = 1,
                      device=None, skip: int = 0):
  """create_input_iter of input_pipeline.py:17-27: the split, prefetched two batches deep
  to this process's device.  `skip`: start at the skip-th batch of the stream (a resumed run)."""
  device = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device is None else device
  source = _open_source(source)
  if is_event_source(source):       # decoded on the device: nothing to prefetch
    return create_event_split(load_source(source), config, train, rank, world, device, skip)
  if is_image_source(source):       # encoded on the device, one launch per batch: the same
    return create_image_split(load_source(source), config, train, rank, world, device, skip)
  ds = create_split(source, config, train=train, cache=cache, rank=rank, world=world,
                    pin=torch.device(device).type == "cuda", skip=skip)
  return feed.DeviceFeeder(ds, device, 2)
