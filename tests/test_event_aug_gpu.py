"""ops.events_bin(augment=...) (snnqp_events_bin_aug, csrc/events.hip) on the GPU, bit for bit
against the numpy restatement of tests/event_aug_cases.py: every output format with its flag word,
both modes, an odd frame with the byte-loop output, a scaled frame and a frame of two bands; each
rule alone and all together, shifts across the band boundary and out of every edge, whole and
empty cutouts, drop bounds 0 and 2^32 - 1, emptied frames, an empty sample, a sample named twice,
the identity record against the plain launch, a hot pixel under a drop, records full of extreme
values through the C entry, and the train split of the pipeline with an `augment` config."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_train_reference as cr
from tests import event_aug_cases as ea
from tests import event_cases as ec
from tests import train_loop_cases as tlc

pytestmark = pytest.mark.gpu

# (H, W) -> scale: 13 x 17 is odd in both and ends in the byte loops; 32 x 32 decodes a 64 x 64
# sensor; 130 x 128 is 16 640 pixels, two bands whose boundary is the line between rows 127 and 128
SHAPES = {(13, 17): 1.0, (32, 32): 2.0, (130, 128): 1.0}
T, START, STEP = 3, 5000, 300
SENTINEL = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A}
I32_MIN, I32_MAX, U32_MAX = -2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _np(t):
  return t.detach().cpu().numpy()


_sets = {}


def _set(dev, hw):
  """Three samples of a shape (shared, never modified): 3000 events, none, 2200 events, with events
  on the window edges of (START, STEP) and a little outside the scaled frame."""
  from snnquantprune_amd import ops
  if hw not in _sets:
    H, W = hw
    scale = SHAPES[hw]
    rng = np.random.Generator(np.random.PCG64(1000 * H + W))
    ev = ec.make_set([ec.edge_sample(rng, n, H, W, T, START, STEP, scale) for n in (3000, 0, 2200)])
    es = ops.EventSet(ev["addrs"], ev["times"], ev["offsets"], (int(H * scale), int(W * scale)), device=dev)
    _sets[hw] = (ev, es, scale)
  return _sets[hw]


def _bin_guarded(es, sample, plist, H, W, fmt, dev, frames=T, guard=64, **kw):
  """The augmented events_bin into the middle of a sentinel-filled buffer -> (array, flag word);
  asserts that nothing outside the result was written."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  packed = fmt in (L.EV1, L.EV4)
  shape = (len(sample), frames, ops.frame_units(H, W, fmt)) if packed else (len(sample), frames, H, W, 2)
  dtype = torch.int32 if fmt == L.EV1 else torch.uint8
  n = int(np.prod(shape))
  buf = torch.full((guard + n + guard,), SENTINEL[dtype], dtype=dtype, device=dev)
  flags = torch.zeros(1, dtype=torch.int32, device=dev)
  aug = None if plist is None else ops.EventAugment(len(sample), **ea.columns(plist))
  got = ops.events_bin(es, sample, frames, H, W, fmt=fmt, flags=flags, out=buf[guard:guard + n].view(shape),
                       augment=aug, **kw)
  data = got.data if packed else got
  assert data.data_ptr() == buf.data_ptr() + guard * buf.element_size()
  torch.cuda.synchronize()
  assert bool((buf[:guard] == SENTINEL[dtype]).all()) and bool((buf[guard + n:] == SENTINEL[dtype]).all())
  return _np(data), int(flags.item())


def _check_all_formats(es, ev, sample, plist, H, W, mode, dev, scale=1.0, start=None, frames=T, guard=64):
  """Every format against the restatement (the flag word included); returns the counts."""
  from snnquantprune_amd import _lib as L
  kw = dict(mode=mode, scale=scale)
  if mode == "time":
    kw.update(start=start, step_us=STEP)
  want = ea.decode_batch_aug(ev, sample, plist, frames, H, W, mode, start, STEP, scale)
  for fmt in (None, L.EV4, L.EV1):
    exp, exp_flag = ec.wire(want, fmt)
    got, flag = _bin_guarded(es, sample, plist, H, W, fmt, dev, frames=frames, guard=guard, **kw)
    assert got.shape == exp.shape and got.dtype == exp.dtype
    np.testing.assert_array_equal(got, exp, err_msg="format %r" % (fmt,))
    assert flag == exp_flag, (fmt, flag, exp_flag)
  return want


def _all_together(H, W, seed, sign=1):
  return ea.params(flip_x=1, flip_y=1, swap=1, dx=sign * 3, dy=-sign * 2, cut=(W // 3, H // 4, W // 3 + 5, H // 4 + 4),
                   frames=(1, 2), drop_below=2 ** 30, seed=seed)


def _groups(H, W):
  """name -> (rows' samples, rows' parameters, rows whose frames must come out all zero)."""
  P = ea.params
  return {
      # each rule alone
      "alone": ([0, 2, 0, 2, 0, 2],
                [P(flip_x=1), P(flip_y=1), P(swap=1), P(dx=4, dy=3), P(cut=(2, 3, W - 4, H - 2)),
                 P(drop_below=2 ** 31, seed=9)], []),
      # across the band boundary (130 x 128: rows 127 | 128) and out of every edge; a whole frame
      # width or height drops everything
      "shifts": ([0, 0, 2, 2, 0, 2],
                 [P(dx=W - 2), P(dx=-(W - 2), dy=-3), P(dy=H - 2, dx=1), P(dy=-(H - 2)), P(dx=W), P(dy=-H, dx=-1)],
                 [4, 5]),
      # a cutout over the whole frame and an empty one, the two ends of drop_below, one frame and all
      "bounds": ([0, 2, 0, 2, 0, 2],
                 [P(cut=(0, 0, W, H)), P(cut=(5, 5, 5, 9)), P(drop_below=0, seed=123), P(drop_below=U32_MAX, seed=123),
                  P(frames=(1, 2)), P(frames=(0, T))], [0, 3, 5]),
      # an empty frame range, everything at once -- one sample in two rows with two seeds --, the
      # empty sample, the identity beside them
      "together": ([2, 0, 0, 1, 2, 2],
                   [P(frames=(1, 1)), _all_together(H, W, 1), _all_together(H, W, 2), _all_together(H, W, 3),
                    P(), _all_together(H, W, 4, -1)], [3]),
  }


@pytest.mark.parametrize("mode", ["number", "time"])
@pytest.mark.parametrize("group", ["alone", "shifts", "bounds", "together"])
@pytest.mark.parametrize("hw", list(SHAPES), ids=["%dx%d" % s for s in SHAPES])
def test_rules_every_format(dev, hw, group, mode):
  H, W = hw
  ev, es, scale = _set(dev, hw)
  sample, plist, empty = _groups(H, W)[group]
  start = [START, START + 7, START, START - 20, START, START + 1]
  want = _check_all_formats(es, ev, sample, plist, H, W, mode, dev, scale, start)
  plain = ec.decode_batch(ev, sample, T, H, W, mode, start, STEP, scale)
  # the cases are not vacuous
  for b in range(len(sample)):
    assert (want[b].sum() == 0) == (b in empty), (group, b)
    assert plain[b].sum() > 0 or sample[b] == 1
  if group == "alone":
    assert all(not np.array_equal(want[b], plain[b]) for b in range(6))
    assert 0.3 * plain[5].sum() < want[5].sum() < 0.7 * plain[5].sum()
    if hw == (130, 128):                                # dy = 3 carries rows 125, 126 over the band boundary
      assert want[3, :, 128:].sum() == plain[3, :, 125:127, :W - 4].sum() > 0
  if group == "shifts" and hw == (130, 128):
    # events cross the band boundary in both directions: rows that start in one band end in the other
    assert plain[2, :, :2].sum() > 0 and want[2, :, 128:].sum() > 0               # dy = H - 2
    assert plain[3, :, 128:].sum() > 0 and want[3, :, :2].sum() > 0               # dy = -(H - 2)
  if group == "bounds":
    np.testing.assert_array_equal(want[1], plain[1])
    np.testing.assert_array_equal(want[2], plain[2])
    assert ea.dropped(np.arange(2200), 123, U32_MAX).all()                        # (only a hash of 2^32 - 1 survives)
    assert want[4, 1].sum() == 0 and want[4, 0].sum() > 0 and want[4, 2].sum() > 0
  if group == "together":
    np.testing.assert_array_equal(want[0], plain[0])
    np.testing.assert_array_equal(want[4], plain[4])
    assert not np.array_equal(want[1], want[2]) and want[1, 1].sum() == 0 and want[1, 0].sum() > 0


@pytest.mark.parametrize("hw", [(13, 17), (130, 128)], ids=["13x17", "130x128"])
def test_output_at_an_odd_address(dev, hw):
  """Frames that begin on no 8- or 4-byte boundary: the byte path of the uint8 / EV4 epilogues."""
  H, W = hw
  ev, es, scale = _set(dev, hw)
  plist = [_all_together(H, W, 5), ea.params(dx=-2, dy=1, swap=1), _all_together(H, W, 6, -1)]
  for mode in ("number", "time"):
    _check_all_formats(es, ev, [0, 2, 0], plist, H, W, mode, dev, scale, start=[START] * 3, guard=3)


@pytest.mark.parametrize("hw", list(SHAPES), ids=["%dx%d" % s for s in SHAPES])
def test_identity_record_gives_the_plain_launch_bytes(dev, hw):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  H, W = hw
  ev, es, scale = _set(dev, hw)
  sample, start = [0, 1, 2, 0], [START, START, START + 5, START - 9]
  ident = ops.EventAugment(4)
  seeded = ops.EventAugment(4, seed=[1, 2, 3, U32_MAX], cutout=[[3, 3, 3, 9]] * 4, frames=[[2, 2]] * 4)
  for mode in ("number", "time"):
    for fmt in (None, L.EV4, L.EV1):
      kw = dict(mode=mode, start=start, step_us=STEP, scale=scale, fmt=fmt)
      fp, fa, fs = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
      plain = ops.events_bin(es, sample, T, H, W, flags=fp, **kw)
      a = ops.events_bin(es, sample, T, H, W, flags=fa, augment=ident, **kw)
      s = ops.events_bin(es, sample, T, H, W, flags=fs, augment=seeded, **kw)
      again = ops.events_bin(es, sample, T, H, W, augment=seeded, **kw)
      data = lambda t: t.data if fmt else t
      assert torch.equal(data(a), data(plain)) and torch.equal(data(s), data(plain)) and torch.equal(data(again), data(s))
      assert int(fa.item()) == int(fp.item()) == int(fs.item())
      assert bool(data(plain).any())
  empty = ops.events_bin(es, [], T, H, W, mode="number", augment=ops.EventAugment(0))
  assert tuple(empty.shape) == (0, T, H, W, 2)


@pytest.mark.parametrize("mode,frames", [("time", 3), ("number", 1)])
def test_hot_pixel_under_a_drop(dev, mode, frames):
  """66 000 events on one pixel, polarity 0, half of the sample dropped by hash: some 33 000 remain
  there -- past every format's ceiling -- while 70 000 events are walked, more than one chunk: the
  halves are clamped between chunks and no carry reaches polarity 1."""
  from snnquantprune_amd import ops
  H = W = 34
  rng = np.random.Generator(np.random.PCG64(43))
  addrs, times, (hx, hy) = ec.hot_sample(rng, H, W, STEP, count=ec.HOT_COUNT, polarity=0)
  quiet = ec.make_sample(rng, 40, H, W, unique=True, t_lo=1, t_hi=3 * STEP)
  ev = ec.make_set([(addrs, times), quiet])
  es = ops.EventSet(ev["addrs"], ev["times"], ev["offsets"], (H, W), device=dev)
  plist = [ea.params(), ea.params(drop_below=2 ** 31, seed=77)]
  want = _check_all_formats(es, ev, [1, 0], plist, H, W, mode, dev, start=[0, 0], frames=frames)
  assert 30000 < want[1, 0, hy, hx, 0] < 36000 and want[1, 0, hy, hx, 1] == 0 and want[0].max() <= 1


def test_records_of_extreme_values_write_only_out(dev):
  """The C entry with records no host check would pass -- INT32_MIN / INT32_MAX in every field,
  all-ones flags and reserved words -- inside guarded buffers: every store of the kernel is guarded
  by the band's pixel count, so the launch completes, writes `out` alone, leaves the records and
  the guards as they were, and still computes what the header says such values do."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  H, W = 130, 128
  ev, es, scale = _set(dev, (H, W))
  sample = [0, 0, 2, 2, 0, 2]
  r = np.array([
      [-1] * 12,                                                          # every bit of the record set
      [-1, I32_MAX, I32_MIN, I32_MIN, I32_MIN, I32_MAX, I32_MAX, I32_MIN, I32_MAX, 0, 0, -1],
      [I32_MIN | 8, I32_MIN, I32_MAX, I32_MAX, I32_MAX, I32_MIN, I32_MIN, I32_MAX, I32_MIN, 0, -1, -1],
      [-8, 0, 0, I32_MIN, I32_MIN, 0, 0, I32_MAX, I32_MAX, 0, -1, I32_MIN],  # ignored bits only: the identity
      [0, 0, 0, I32_MIN, I32_MIN, I32_MAX, I32_MAX, 0, 0, 0, 0, 0],           # a cutout over everything
      [1, 0, 0, 0, 0, 0, 0, I32_MIN, 1, 0, 0, 0],                             # frames from far below 0: frame 0
  ], np.int64)
  plist = [ea.params(flip_x=row[0] & 1, flip_y=row[0] >> 1 & 1, swap=row[0] >> 2 & 1, dx=row[1], dy=row[2],
                     cut=tuple(row[3:7]), frames=tuple(row[7:9]), drop_below=row[9] & U32_MAX, seed=row[10] & U32_MAX)
           for row in r.tolist()]
  rec_host = (r & U32_MAX).astype(np.uint32).view(np.int32)
  guard = 16
  rec = torch.full((guard + 6 * 12 + guard,), SENTINEL[torch.int32], dtype=torch.int32, device=dev)
  rec[guard:guard + 72] = torch.from_numpy(rec_host.reshape(-1)).to(dev)
  rec_before = rec.clone()
  rows = torch.tensor(sample, dtype=torch.int32, device=dev)
  start = torch.full((6,), START, dtype=torch.int32, device=dev)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  for mode in (0, 1):
    want = ea.decode_batch_aug(ev, sample, plist, T, H, W, "number" if mode == 0 else "time", [START] * 6, STEP, scale)
    plain = ec.decode_batch(ev, sample, T, H, W, "number" if mode == 0 else "time", [START] * 6, STEP, scale)
    np.testing.assert_array_equal(want[3], plain[3])
    assert plain[3].sum() > 0 and all(want[b].sum() == 0 for b in (0, 1, 2, 4))
    np.testing.assert_array_equal(want[5, 1:], plain[5, 1:, :, ::-1])
    assert want[5, 0].sum() == 0 and plain[5, 0].sum() > 0 and want[5, 1:].sum() > 0
    for fmt in (L.U8, L.EV4, L.EV1):
      dtype = torch.int32 if fmt == L.EV1 else torch.uint8
      units = ops.frame_units(H, W, fmt) if fmt != L.U8 else H * W * 2
      n = 6 * T * units
      buf = torch.full((64 + n + 64,), SENTINEL[dtype], dtype=dtype, device=dev)
      flags = torch.zeros(3, dtype=torch.int32, device=dev)
      L.check(L.lib().snnqp_events_bin_aug(p(es.addr), p(es.times), p(es.offsets), es.num_samples, p(rows), p(start), 6,
                                           mode, T, STEP, H, W, scale, p(rec[guard:]), p(buf[64:]), fmt, p(flags[1:]),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
      torch.cuda.synchronize()
      assert ops.device_status() == 0
      assert bool((buf[:64] == SENTINEL[dtype]).all()) and bool((buf[64 + n:] == SENTINEL[dtype]).all())
      assert torch.equal(rec, rec_before)
      exp, exp_flag = ec.wire(want, None if fmt == L.U8 else fmt)
      np.testing.assert_array_equal(_np(buf[64:64 + n]).reshape(exp.shape), exp)
      assert _np(flags).tolist() == [0, exp_flag, 0]


# ---- the pipeline with config.augment ------------------------------------------------------------

AUGMENT = dict(flip_x=0.5, flip_y=0.5, swap_polarity=0.5, shift=2, drop_event=0.5, cutout=0.5, drop_frames=1)


def _t_range(src):
  off, n = src["offsets"], src["label"].shape[0]
  return (np.array([src["times"][off[i]] for i in range(n)], np.int64),
          np.array([src["times"][off[i + 1] - 1] for i in range(n)], np.int64))


@pytest.mark.parametrize("split_by", ["number", "time"])
def test_train_split_batches_equal_the_reference_and_resume(dev, split_by):
  """create_input_iter(train=True) with an `augment` config: every batch is the restatement's under
  the parameters a plan of the same seed draws; a stream resumed at its third batch is the tail of
  the uninterrupted one; the eval split of the same config is the plain decode."""
  from snnquantprune_amd import input_pipeline as ip
  src, test = tlc.sources()
  cfg = tlc.make_config(split_by=split_by, augment=AUGMENT)
  n = src["label"].shape[0]
  it = ip.create_input_iter(src, cfg, train=True, cache=False, device=dev)
  plan = ip.EventPlan(cfg, src["sensor_size"], n, train=True)      # the same seed: the same draws
  drawn = plan.augmented_batches(*_t_range(src))
  seen, moved = [], 0
  for _ in range(5):                                               # an epoch is four batches
    batch = next(it)
    idx, starts, aug = next(drawn)
    plist = ea.from_columns(aug)
    want = ea.decode_batch_aug(src, idx, plist, tlc.T, tlc.H, tlc.W, split_by, starts, plan.step_us)
    plain = ec.decode_batch(src, idx, tlc.T, tlc.H, tlc.W, split_by, starts, plan.step_us)
    moved += int(not np.array_equal(want, plain))
    assert batch["dvs_matrix"].dtype == torch.uint8 and want.sum() > 0
    np.testing.assert_array_equal(_np(batch["dvs_matrix"]), np.minimum(want, 255).astype(np.uint8))
    np.testing.assert_array_equal(_np(batch["label"]), src["label"][idx])
    seen.append(batch)
  assert moved == 5
  resumed = ip.create_input_iter(src, cfg, train=True, cache=False, device=dev, skip=2)
  for k in range(2, 5):
    batch = next(resumed)
    assert torch.equal(batch["dvs_matrix"], seen[k]["dvs_matrix"]) and torch.equal(batch["label"], seen[k]["label"])
  # eval never augments, whatever the config holds
  ev_it = ip.create_input_iter(test, cfg, train=False, cache=False, device=dev)
  ev_plan = ip.EventPlan(cfg, test["sensor_size"], test["label"].shape[0], train=False)
  idx, starts = next(ev_plan.batches(*_t_range(test)))
  want = ec.decode_batch(test, idx, tlc.T, tlc.H, tlc.W, split_by, starts, ev_plan.step_us)
  np.testing.assert_array_equal(_np(next(ev_it)["dvs_matrix"]), np.minimum(want, 255).astype(np.uint8))


def test_two_train_steps_from_an_augmented_split(dev):
  """Two train_steps of the tiny ConvDenseSNN on augmented batches: a finite loss, moved parameters."""
  from snnquantprune_amd import input_pipeline as ip
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models
  from snnquantprune_amd import train_utils as tu
  src, _ = tlc.sources()
  cfg = tlc.make_config(split_by="time", augment=AUGMENT)
  v, _ = cr.fixture(True)
  model = models.ConvDenseSNN(num_classes=cr.CLASSES, config=cfg)
  state = tu.create_train_state(nn.tree_from_numpy(v, dev), cfg, model)
  before = [p.clone() for _, p in tu._flatten(state.params["params"])]
  it = ip.create_input_iter(src, cfg, train=True, cache=False, device=dev)
  for step in range(2):
    batch = next(it)
    assert batch["dvs_matrix"].dtype == torch.uint8 and bool(batch["dvs_matrix"].any())
    state, m = tu.train_step(state, batch, step, lambda s: 1e-2, 0.0, 0.0, tu.mse_loss)
    assert bool(torch.isfinite(m["loss"]))
  after = [p for _, p in tu._flatten(state.params["params"])]
  assert state.step == 2 and any(not torch.equal(a, b) for a, b in zip(after, before))
