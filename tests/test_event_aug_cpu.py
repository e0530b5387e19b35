"""Event augmentation without a GPU: the numpy restatement of tests/event_aug_cases.py against the
plain one and against array moves of its counts, the drop hash's statistics, the plan's draws
(input_pipeline.EventPlan with config.augment), ops.EventAugment / ops.events_bin's host
validation, and snnqp_events_bin_aug's argument checks."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import event_aug_cases as ea
from tests import event_cases as ec

RNG = lambda seed: np.random.Generator(np.random.PCG64(seed))
H, W, T, START, STEP = 9, 13, 4, 700, 90


@pytest.fixture(scope="module")
def streams():
  rng = RNG(21)
  ev = ec.make_set([ec.edge_sample(rng, n, H, W, T, START, STEP, 2.0) for n in (600, 0, 350)])
  return ev, [2, 0, 1, 0], [START, START + 11, START, START - 40]


def _both_modes(ev, sample, start, plist, scale=2.0):
  return [ea.decode_batch_aug(ev, sample, plist, T, H, W, "number", scale=scale),
          ea.decode_batch_aug(ev, sample, plist, T, H, W, "time", start, STEP, scale)]


# ---- the restatement ----------------------------------------------------------------------------

def test_identity_parameters_equal_the_plain_restatement(streams):
  ev, sample, start = streams
  num, tim = _both_modes(ev, sample, start, [ea.params()] * 4)
  np.testing.assert_array_equal(num, ec.decode_batch(ev, sample, T, H, W, "number", scale=2.0))
  np.testing.assert_array_equal(tim, ec.decode_batch(ev, sample, T, H, W, "time", start, STEP, 2.0))
  assert num[0].sum() > 0 and tim[0].sum() > 0 and num[2].sum() == 0
  # a seed alone drops nothing, and a hash is never below 0
  for got, want in zip(_both_modes(ev, sample, start, [ea.params(seed=77)] * 4), (num, tim)):
    np.testing.assert_array_equal(got, want)


def test_flips_reverse_an_axis_and_two_flips_are_the_identity(streams):
  ev, sample, start = streams
  plain = _both_modes(ev, sample, start, [ea.params()] * 4)
  fx = _both_modes(ev, sample, start, [ea.params(flip_x=1)] * 4)
  fy = _both_modes(ev, sample, start, [ea.params(flip_y=1)] * 4)
  fxy = _both_modes(ev, sample, start, [ea.params(flip_x=1, flip_y=1)] * 4)
  for p, x, y, xy in zip(plain, fx, fy, fxy):
    assert not np.array_equal(x, p) and not np.array_equal(y, p)
    np.testing.assert_array_equal(x[:, :, :, ::-1], p)              # flipping the flipped frames: the identity
    np.testing.assert_array_equal(y[:, :, ::-1], p)
    np.testing.assert_array_equal(xy[:, :, ::-1, ::-1], p)
  # the same on the events: the stream mirrored in the sensor, decoded with the flip, is the stream
  a, t = ev["addrs"][:600].copy(), ev["times"][:600]
  inside = (a[:, 0] < W) & (a[:, 1] < H)
  a, t = a[inside], t[inside]
  m = a.copy()
  m[:, 0] = W - 1 - m[:, 0]
  np.testing.assert_array_equal(ea.decode_aug(m, t, ea.params(flip_x=1), T, H, W, "number"),
                                ea.decode_aug(a, t, ea.params(), T, H, W, "number"))


@pytest.mark.parametrize("dx,dy", [(3, 0), (-3, 0), (0, 2), (0, -2), (5, -4), (-12, 8), (W, 0), (0, -H), (16384, -16384)])
def test_a_shift_is_a_zero_filled_move_of_the_counts(streams, dx, dy):
  ev, sample, start = streams
  plain = _both_modes(ev, sample, start, [ea.params()] * 4)
  moved = _both_modes(ev, sample, start, [ea.params(dx=dx, dy=dy)] * 4)
  for p, m in zip(plain, moved):
    want = np.zeros_like(p)
    if abs(dx) < W and abs(dy) < H:
      want[:, :, max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = \
          p[:, :, max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
      assert want.sum() > 0
    np.testing.assert_array_equal(m, want)


def test_cutout_and_frame_drops_zero_their_region_and_nothing_else(streams):
  ev, sample, start = streams
  plain = _both_modes(ev, sample, start, [ea.params()] * 4)
  for cut in ((2, 1, 7, 5), (0, 0, W, H), (-5, -5, 3, 3), (4, 4, 4, 9), (6, 3, 2, 8), (W - 1, H - 1, W + 9, H + 9)):
    for p, c in zip(plain, _both_modes(ev, sample, start, [ea.params(cut=cut)] * 4)):
      want = p.copy()
      x0, y0, x1, y1 = (max(v, 0) for v in cut)
      want[:, :, y0:max(y1, y0), x0:max(x1, x0)] = 0
      np.testing.assert_array_equal(c, want)
      assert (c.sum() == p.sum()) == (cut[2] <= cut[0] or cut[3] <= cut[1])
  for frames in ((0, 0), (2, 2), (1, 2), (0, T), (T - 1, T), (1, 3)):
    for p, c in zip(plain, _both_modes(ev, sample, start, [ea.params(frames=frames)] * 4)):
      want = p.copy()
      want[:, frames[0]:frames[1]] = 0
      np.testing.assert_array_equal(c, want)
  assert plain[0][0, 1].sum() > 0 and plain[1][0, 1].sum() > 0


def test_polarity_swap_exchanges_the_channels(streams):
  ev, sample, start = streams
  plain = _both_modes(ev, sample, start, [ea.params()] * 4)
  for p, s in zip(plain, _both_modes(ev, sample, start, [ea.params(swap=1)] * 4)):
    np.testing.assert_array_equal(s, p[..., ::-1])
    assert not np.array_equal(s, p)


def test_drops_take_events_by_their_index_within_the_sample(streams):
  """The random drop of a row keeps exactly the events whose hash is not below the bound, whatever
  frame they fall in and whichever row names the sample; rows differ per record."""
  ev, sample, start = streams
  a, t = ev["addrs"][:600], ev["times"][:600]
  gone = ea.dropped(np.arange(600), 5, 2 ** 31)
  assert 200 < gone.sum() < 400
  for mode in ("number", "time"):
    got = ea.decode_aug(a, t, ea.params(seed=5, drop_below=2 ** 31), T, H, W, mode, START, STEP, 2.0)
    if mode == "time":
      np.testing.assert_array_equal(got, ec.decode_time(a[~gone], t[~gone], START, STEP, T, H, W, 2.0))
    else:                                               # number mode's slices count the dropped events too
      di = 600 // T
      for f in range(T):
        lo, hi = f * di, (f + 1) * di if f < T - 1 else 600
        np.testing.assert_array_equal(got[f], ec.frame_of(a[lo:hi][~gone[lo:hi]], H, W, 2.0))
  every = ea.decode_aug(a, t, ea.params(seed=5, drop_below=2 ** 32 - 1), T, H, W, "number", scale=2.0)
  assert every.sum() == 0
  rows = ea.decode_batch_aug(ev, [0, 0], [ea.params(seed=1, drop_below=2 ** 31), ea.params(seed=2, drop_below=2 ** 31)],
                             T, H, W, "number", scale=2.0)
  assert not np.array_equal(rows[0], rows[1])


def test_records_follow_the_header_layout():
  p = ea.params(flip_y=1, swap=1, dx=-3, dy=16384, cut=(-1, 2, 3, 2 ** 31 - 1), frames=(1, 4), drop_below=2 ** 32 - 1,
                seed=0x80000000)
  r = ea.records([ea.params(), p])
  assert r.shape == (2, 12) and r.dtype == np.int32 and r.nbytes == 2 * 48 and not r[0].any()
  assert r[1].tolist() == [6, -3, 16384, -1, 2, 3, 2 ** 31 - 1, 1, 4, -1, -2 ** 31, 0]
  assert ea.from_columns(ea.columns([ea.params(), p])) == [ea.params(), p]


# ---- the hash -----------------------------------------------------------------------------------

HASH_SEEDS = [0, 1, 2, 3, 0x80000000, 0xFFFFFFFF, 12344, 12345, 0xDEADBEEF]


def test_fmix32_is_the_murmur3_finaliser():
  # h = 0 is its fixed point; the others by the definition, one value at a time in Python integers
  def one(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    return h ^ (h >> 16)
  vals = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF, 65535, 65536]
  assert ea.fmix32(np.array(vals)).tolist() == [one(v) for v in vals] and one(0) == 0 and one(1) == 0x514E28B7


@pytest.mark.parametrize("p", [1 / 16, 1 / 2, 0.9])
def test_drop_hash_counts_and_independence_of_seeds(p):
  """N = 65536 indices: the number dropped lies within 6 sigma of N p for every seed, and the overlap
  of any two seeds' dropped sets within 6 sigma of N p^2 (binomial sigmas)."""
  N = 65536
  below = int(np.floor(p * 2.0 ** 32))
  sets = [ea.dropped(np.arange(N), s, below) for s in HASH_SEEDS]
  for s, d in zip(HASH_SEEDS, sets):
    assert abs(int(d.sum()) - N * p) <= 6 * np.sqrt(N * p * (1 - p)), (hex(s), int(d.sum()))
  for (s, a), (r, b) in itertools.combinations(zip(HASH_SEEDS, sets), 2):
    both = int((a & b).sum())
    assert abs(both - N * p * p) <= 6 * np.sqrt(N * p * p * (1 - p * p)), (hex(s), hex(r), both)


# ---- the plan -----------------------------------------------------------------------------------

ALL = dict(flip_x=0.5, flip_y=0.3, swap_polarity=0.5, shift=3, drop_event=0.4, cutout=0.5, drop_frames=2)
N_SAMPLES = 10
T_MIN = np.array([1000 + 10 * i for i in range(N_SAMPLES)], np.int64)
T_MAX = T_MIN + 30000


def _config(**kw):
  from snnquantprune_amd import synthetic as syn
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  cfg.split_by, cfg.num_frames, cfg.resolution_scale = "time", 3, 2
  cfg.time_step, cfg.input_scale, cfg.train_chunk_size, cfg.test_chunk_size = 1, 1, 4, 7
  cfg.batch_size, cfg.eval_batch_size, cfg.seed, cfg.feed_format = 4, 2, 11, "u8"
  for k, v in kw.items():
    setattr(cfg, k, v)
  return cfg


def _plan(train=True, sensor=(16, 24), **kw):
  from snnquantprune_amd import input_pipeline as ip
  return ip.EventPlan(_config(**kw), sensor, N_SAMPLES, train=train)


def _take(plan, k, skip=0):
  it = plan.augmented_batches(T_MIN, T_MAX, skip)
  return [next(it) for _ in range(k)]


def _same(a, b):
  ok = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[2] is None) == (b[2] is None)
  if ok and a[2] is not None:
    ok = ea.from_columns(a[2]) == ea.from_columns(b[2])
  return ok


def test_plan_draws_every_parameter_in_its_range():
  plan = _plan(augment=ALL)                           # frames of 8 x 12, T = 3
  assert (plan.H, plan.W, plan.T, plan.per) == (8, 12, 3, 4)
  rows = []
  for idx, starts, aug in _take(plan, 60):
    assert aug.rows == 4 and idx.shape == (4,) and starts.shape == (4,)
    rows += ea.from_columns(aug)
  col = lambda k: np.array([r[k] for r in rows])
  for k, p in (("flip_x", 0.5), ("flip_y", 0.3), ("swap", 0.5)):
    assert set(col(k)) == {0, 1} and abs(col(k).mean() - p) < 6 * np.sqrt(p * (1 - p) / len(rows))
  for k in ("dx", "dy"):
    assert set(col(k)) == set(range(-3, 4))
  below = col("drop_below")
  assert below.min() >= 0 and below.max() < 0.4 * 2 ** 32 and below.max() > 0.3 * 2 ** 32 and below.min() < 0.1 * 2 ** 32
  seeds = col("seed")
  assert seeds.min() >= 0 and seeds.max() < 2 ** 32 and seeds.max() >= 2 ** 31 and len(set(seeds)) == len(rows)
  cut = col("cut")
  w, h = cut[:, 2] - cut[:, 0], cut[:, 3] - cut[:, 1]
  assert set(w) == set(range(0, 7)) and set(h) == set(range(0, 5))            # floor(0.5 * 12), floor(0.5 * 8)
  assert cut[:, 0].min() == 0 and cut[:, 1].min() == 0 and cut[:, 2].max() == 12 and cut[:, 3].max() == 8
  fr = col("frames")
  assert set(fr[:, 1] - fr[:, 0]) == {0, 1, 2} and fr[:, 0].min() == 0 and fr[:, 1].max() == 3
  # drop_below is floor(p * 2^32) of a float64 p <= drop_event: certain at the top of the range
  top = _plan(augment=dict(drop_event=1.0))
  b = np.concatenate([a.drop_below for _, _, a in _take(top, 40)])
  assert b.max() <= 2 ** 32 - 1 and b.max() > 0.9 * 2 ** 32


@pytest.mark.parametrize("key", sorted(ALL))
def test_each_key_alone_leaves_the_others_at_identity(key):
  plan = _plan(augment={key: ALL[key]})
  rows = [r for _, _, aug in _take(plan, 12) for r in ea.from_columns(aug)]
  mine = {"swap_polarity": ("swap",), "shift": ("dx", "dy"), "drop_event": ("drop_below", "seed"), "cutout": ("cut",),
          "drop_frames": ("frames",)}.get(key, (key,))
  for k, ident in ea.IDENTITY.items():
    vals = [r[k] for r in rows]
    if k in mine:
      assert any(v != ident for v in vals), k
    else:
      assert all(v == ident for v in vals), k
  # the indices and origins in front of the first augmentation draw are the plain plan's
  a, b = _take(_plan(augment={key: ALL[key]}), 1)[0], _take(_plan(), 1)[0]
  assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_same_seed_gives_the_same_stream_and_skip_equals_consuming():
  a, b = _take(_plan(augment=ALL), 7), _take(_plan(augment=ALL), 7)
  assert all(_same(x, y) for x, y in zip(a, b))
  other = _take(_plan(augment=ALL, seed=12), 7)
  assert not any(_same(x, y) for x, y in zip(a, other))
  for k in (1, 2, 5):                                  # (an epoch is two batches)
    tail = _take(_plan(augment=ALL), 7 - k, skip=k)
    assert all(_same(x, y) for x, y in zip(a[k:], tail)), k
  # batches() is the same stream without the records
  plain = _plan(augment=ALL).batches(T_MIN, T_MAX, 2)
  for x in a[2:5]:
    idx, starts = next(plain)
    assert np.array_equal(idx, x[0]) and np.array_equal(starts, x[1])
  # number mode: no origins, the same draws otherwise
  num = _take(_plan(augment=ALL, split_by="number"), 2)
  assert num[0][1] is None and num[0][2].rows == 4


def test_no_key_and_an_all_zero_key_are_todays_stream():
  zero = {k: 0 for k in ALL}
  plans = [_plan(), _plan(augment={}), _plan(augment=zero), _plan(augment=dict(shift=0, flip_x=0.0))]
  streams = [_take(p, 6) for p in plans]
  for s in streams:
    assert all(aug is None for _, _, aug in s)
    assert all(_same(x, y) for x, y in zip(s, streams[0]))
  # ... which is what batches() of a plan without the key yields, generator state included
  gens = [p.gen.get_state() for p in plans]
  assert all(torch.equal(g, gens[0]) for g in gens)
  it = _plan().batches(T_MIN, T_MAX)
  for x in streams[0]:
    idx, starts = next(it)
    assert np.array_equal(idx, x[0]) and np.array_equal(starts, x[1])
  busy = _plan(augment=ALL)
  _take(busy, 6)
  assert not torch.equal(busy.gen.get_state(), gens[0])


def test_the_eval_split_ignores_the_key():
  a, b = _take(_plan(train=False, augment=ALL), 7), _take(_plan(train=False), 7)
  assert all(aug is None for _, _, aug in a) and all(_same(x, y) for x, y in zip(a, b))
  assert _plan(train=False, augment=ALL).augment == {}


def test_the_constructor_refuses_bad_augment_configs():
  for bad in (dict(flip=0.5), dict(flip_x=0.5, rotate=10), dict(flip_x=1.5), dict(flip_y=-0.1), dict(swap_polarity=2),
              dict(drop_event=1.01), dict(drop_event=float("nan")), dict(cutout=-0.5), dict(cutout=1.5),
              dict(shift=-1), dict(shift=1.5), dict(shift=16385), dict(drop_frames=-1), dict(drop_frames=4),
              dict(drop_frames=0.5)):
    for train in (True, False):
      with pytest.raises(ValueError, match="augment"):
        _plan(train=train, augment=bad)
  with pytest.raises(ValueError, match="augment"):
    _plan(augment=0.5)
  _plan(augment=dict(shift=16384, drop_frames=3, cutout=1.0, flip_x=1, drop_event=1.0))


# ---- ops.EventAugment and ops.events_bin on the host ---------------------------------------------

def test_event_augment_validates_on_the_host():
  from snnquantprune_amd import ops
  p = [ea.params(flip_x=1, dx=-16384, dy=16384, cut=(-2 ** 31, 0, 2 ** 31 - 1, 5), frames=(0, 3), drop_below=2 ** 32 - 1,
                 seed=2 ** 32 - 1), ea.params(swap=1, flip_y=1, frames=(2, 2))]
  aug = ops.EventAugment(2, **ea.columns(p))
  np.testing.assert_array_equal(aug.records(3), ea.records(p))
  assert ea.from_columns(aug) == p
  np.testing.assert_array_equal(ops.EventAugment(3).records(0), np.zeros((3, 12), np.int32))
  np.testing.assert_array_equal(ops.EventAugment(2, flip_x=np.array([True, False]), seed=torch.tensor([1, 2])).records(1),
                                ea.records([ea.params(flip_x=1, seed=1), ea.params(seed=2)]))
  with pytest.raises(ValueError, match="frames"):
    aug.records(2)                                    # f1 = 3 > T
  for bad in (dict(dx=[0]), dict(dx=[0, 16385]), dict(dy=[-16385, 0]), dict(flip_x=[0, 2]), dict(flip_y=[0, 0, 0]),
              dict(swap_polarity=[-1, 0]), dict(cutout=[[0, 0, 1, 1]]), dict(cutout=[[0, 0, 1, 2 ** 31]] * 2),
              dict(cutout=[0, 0]), dict(frames=[[1, 0], [0, 0]]), dict(frames=[[-1, 0], [0, 0]]), dict(frames=[0, 0]),
              dict(drop_below=[0, 2 ** 32]), dict(drop_below=[-1, 0]), dict(seed=[2 ** 32, 0]), dict(seed=[0, -1]),
              dict(seed=[0.5, 1.0])):
    with pytest.raises(ValueError, match=list(bad)[0]):
      ops.EventAugment(2, **bad)


def test_events_bin_validates_the_augment_before_any_upload():
  from snnquantprune_amd import ops
  rng = RNG(7)
  ev = ec.make_set([ec.make_sample(rng, n, 20, 30, t_lo=10, t_hi=500) for n in (50, 0, 7)])
  es = ops.EventSet(ev["addrs"], ev["times"], ev["offsets"], (20, 30))
  with pytest.raises(ValueError, match="augment"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="number", augment=ops.EventAugment(3))
  with pytest.raises(ValueError, match="augment"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="number", augment={"dx": [0, 0]})
  with pytest.raises(ValueError, match="frames"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="number", augment=ops.EventAugment(2, frames=[[0, 4], [0, 0]]))
  # a valid one reaches the same refusal as the plain call: CPU tensors
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="number", augment=ops.EventAugment(2, frames=[[0, 3], [0, 0]]))


# ---- the C entry point's argument checks --------------------------------------------------------

def test_events_bin_aug_argument_errors_without_a_gpu():
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  p = ctypes.c_void_p(64)                                  # never dereferenced: the checks come first

  for aug in (p, None):                                    # with and without records: the same checks
    def call(S=1, B=1, mode=1, T=1, step=10, H=4, W=4, scale=1.0, out_type=L.U8, times=p, start=p):
      return lib.snnqp_events_bin_aug(None, times, None, S, None, start, B, mode, T, step, H, W, scale, aug, None,
                                      out_type, None, None)

    for bad in (dict(S=-1), dict(B=-1), dict(T=-1), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385)):
      assert call(**bad) == L.EINVAL and b"shape" in lib.snnqp_last_error(), bad
    assert call(mode=2) == L.EINVAL and b"mode" in lib.snnqp_last_error()
    assert call(scale=0.0) == L.EINVAL and b"scale" in lib.snnqp_last_error()
    for t in (L.F32, L.BITS, 7):
      assert call(out_type=t) == L.EINVAL and b"out_type" in lib.snnqp_last_error()
    for s in (0, -5):
      assert call(step=s) == L.EINVAL and b"step_us" in lib.snnqp_last_error()
    assert call(times=None) == L.EINVAL and b"times" in lib.snnqp_last_error()
    assert call(start=None) == L.EINVAL and b"times" in lib.snnqp_last_error()
    assert call(mode=0, times=None, start=None, step=0) == L.EINVAL and b"null" in lib.snnqp_last_error()
    assert call() == L.EINVAL and b"null" in lib.snnqp_last_error()
    assert call(B=0) == L.OK and call(T=0) == L.OK and call(mode=0, B=0, times=None, start=None) == L.OK
    assert call(B=0, out_type=9) == L.EINVAL
