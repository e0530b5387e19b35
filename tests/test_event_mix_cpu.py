"""Event mixing without a GPU: the numpy restatement of tests/event_mix_cases.py against a
per-event loop and against its own corner cases, the fixtures' kept-event counts, the plan's draws
(input_pipeline.EventPlan with config.mix), ops.EventMix / ops.events_bin's host validation,
snnqp_events_bin_mix's argument checks, and the soft targets of train_utils."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_aug_cases as ea
from tests import event_cases as ec
from tests import event_mix_cases as em

RNG = lambda seed: np.random.Generator(np.random.PCG64(seed))                      # noqa: E731


# ---- the restatement ------------------------------------------------------------------------------

def _loop_row(addrs, times, p, T, H, W, mode, start, step_us, scale, box, keep_in):
  """Counts [T, H, W, 2] of one sample, one event at a time, in the header's words: the frame's slice
  of the untouched sample, rules 1-6 of the record, then the box -- dropped inside it
  (keep_in = False: the primary) or outside it (the partner) -- for frames in [g0, g1); a partner is
  read in those frames only."""
  out = np.zeros((T, H, W, 2), np.int64)
  n = addrs.shape[0]
  x0, y0, x1, y1, g0, g1 = (int(v) for v in box)
  for f in range(T):
    boxed = g0 <= f < g1
    if p["frames"][0] <= f < p["frames"][1] or (keep_in and not boxed):
      continue
    if mode == "number":
      di = n // T
      members = range(f * di, (f + 1) * di if f < T - 1 else n)
    else:
      lo = int(start) + f * int(step_us)
      members = [i for i in range(n) if lo < int(times[i]) < lo + int(step_us)]
    for i in members:
      x = int(np.floor(np.float32(addrs[i, 0]) / np.float32(scale)))
      y = int(np.floor(np.float32(addrs[i, 1]) / np.float32(scale)))
      if not (0 <= x < W and 0 <= y < H):
        continue
      x = W - 1 - x if p["flip_x"] else x
      y = H - 1 - y if p["flip_y"] else y
      x, y = x + p["dx"], y + p["dy"]
      if not (0 <= x < W and 0 <= y < H):
        continue
      if p["cut"][0] <= x < p["cut"][2] and p["cut"][1] <= y < p["cut"][3]:
        continue
      if bool(ea.dropped(i, p["seed"], p["drop_below"])):
        continue
      pol = int(addrs[i, 2] != 0) ^ int(bool(p["swap"]))
      inside = boxed and x0 <= x < x1 and y0 <= y < y1
      if inside != keep_in:
        continue
      out[f, y, x, pol] += 1
  return out


@pytest.mark.parametrize("mode", ["number", "time"])
@pytest.mark.parametrize("hw,T,group", [((13, 17), 3, "rules"), ((13, 17), 1, "box"), ((13, 17), 3, "frames"),
                                        ((13, 17), 3, "ragged"), ((32, 32), 3, "edges")])
def test_the_restatement_equals_a_per_event_loop(hw, T, group, mode):
  H, W = hw
  ev, scale = em.fixture_set(hw, T)
  rows = em.groups(H, W, T)[group]
  sample, partner, box, plist, plist2, start, start2 = em.columns_of(rows)
  want, kept = em.expected(hw, T, group, mode)
  off = ev["offsets"]
  for b, r in enumerate(rows):
    sl = lambda s: (ev["addrs"][off[s]:off[s + 1]], ev["times"][off[s]:off[s + 1]])       # noqa: E731
    none = em.NO_BOX if partner[b] < 0 else box[b]
    a = _loop_row(*sl(sample[b]), plist[b], T, H, W, mode, start[b], em.STEP, scale, none, False)
    got, n2 = a, 0
    if partner[b] >= 0:
      other = _loop_row(*sl(partner[b]), plist2[b], T, H, W, mode, start2[b], em.STEP, scale, box[b], True)
      got, n2 = a + other, other.sum()
    np.testing.assert_array_equal(got, want[b], err_msg="%s row %d" % (group, b))
    assert kept[b].tolist() == [a.sum(), n2], (group, b)


@pytest.mark.parametrize("mode", ["number", "time"])
@pytest.mark.parametrize("T", em.FRAMES)
@pytest.mark.parametrize("hw", list(em.SHAPES), ids=["%dx%d" % s for s in em.SHAPES])
def test_corner_cases_and_the_fixtures_kept_counts(hw, T, mode):
  """An empty box or a partner of -1 is event_aug_cases' result, a full box is the partner's
  frames, and every mixed fixture row keeps events of both samples except the rows built not to."""
  H, W = hw
  ev, scale = em.fixture_set(hw, T)
  for name, rows in em.groups(H, W, T).items():
    sample, partner, box, plist, plist2, start, start2 = em.columns_of(rows)
    want, kept = em.expected(hw, T, name, mode)
    own = ea.decode_batch_aug(ev, sample, plist, T, H, W, mode, start, em.STEP, scale)
    for b, r in enumerate(rows):
      x0, y0, x1, y1, g0, g1 = r["box"]
      if partner[b] < 0 or x1 <= x0 or y1 <= y0 or g1 <= g0:
        np.testing.assert_array_equal(want[b], own[b])
        assert kept[b].tolist() == [own[b].sum(), 0]
      if partner[b] >= 0 and r["box"] == (0, 0, W, H, 0, T):
        other = ea.decode_batch_aug(ev, [partner[b]], [plist2[b]], T, H, W, mode, [start2[b]], em.STEP, scale)[0]
        np.testing.assert_array_equal(want[b], other)
        assert kept[b].tolist() == [0, other.sum()] and other.sum() > 0
      assert want[b].sum() == kept[b].sum()
      if r["expect"] != "any":
        assert (kept[b, 0] > 0, kept[b, 1] > 0) == {"both": (True, True), "A": (True, False), "B": (False, True),
                                                    "none": (False, False)}[r["expect"]], (name, b, kept[b])
    if name == "edges" and hw == (130, 128):
      # the band box holds partner events on both sides of the line between rows 127 and 128
      assert (want[5] - own[5]).clip(0)[:, 120:128].sum() > 0 and (want[5] - own[5]).clip(0)[:, 128:129].sum() > 0
    if name == "box" and hw == (13, 17):
      assert want.max() > 1                             # EV1 does saturate (EV4, uint8: the hot-pixel tests)


def test_box_slices_clip_and_empty():
  assert em.box_slices((-5, 2, 40, 3, 1, 9), 3, 8, 12) == (slice(1, 3), slice(2, 3), slice(0, 12))
  f, y, x = em.box_slices((5, 6, 5, 2, 3, 3), 3, 8, 12)
  assert x.start == x.stop and y.start >= y.stop and f.start == f.stop
  lo, hi = -2 ** 31, 2 ** 31 - 1
  assert em.box_slices((lo, lo, hi, hi, lo, hi), 3, 8, 12) == (slice(0, 3), slice(0, 8), slice(0, 12))
  f, y, x = em.box_slices((hi, hi, lo, lo, hi, lo), 3, 8, 12)
  assert x.start >= x.stop and y.start >= y.stop and f.start >= f.stop


# ---- the plan -------------------------------------------------------------------------------------

AUG = dict(flip_x=0.5, shift=3, drop_event=0.4, cutout=0.5, drop_frames=2)
MIX = dict(prob=0.5, size=0.5, frames=2)
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
  it = plan.mixed_batches(T_MIN, T_MAX, skip)
  return [next(it) for _ in range(k)]


def _aug_same(a, b):
  return (a is None) == (b is None) and (a is None or ea.from_columns(a) == ea.from_columns(b))


def _same(a, b):
  ok = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _aug_same(a[2], b[2]) and (a[3] is None) == (b[3] is None)
  if ok and a[3] is not None:
    ok = (np.array_equal(a[3].partner, b[3].partner) and np.array_equal(a[3].box, b[3].box)
          and np.array_equal(a[3].start, b[3].start) and _aug_same(a[3].augment, b[3].augment))
  return ok


def test_plan_draws_the_mix_in_its_ranges_and_pairs_rows_with_the_next():
  plan = _plan(augment=AUG, mix=MIX)                  # frames of 8 x 12, T = 3
  assert (plan.H, plan.W, plan.T, plan.per) == (8, 12, 3, 4)
  boxes, mixed = [], []
  for idx, starts, aug, mix in _take(plan, 80):
    assert mix.rows == 4 and mix.box.shape == (4, 6)
    on = mix.partner >= 0
    np.testing.assert_array_equal(mix.partner[on], np.roll(idx, -1)[on])           # row (b + 1) mod per
    np.testing.assert_array_equal(mix.start, np.roll(starts, -1))                  # with its own origin
    assert ea.from_columns(mix.augment) == list(np.roll(np.array(ea.from_columns(aug), object), -1))   # and record
    boxes.append(mix.box)
    mixed.append(on)
  box, on = np.concatenate(boxes), np.concatenate(mixed)
  assert abs(on.mean() - 0.5) < 6 * np.sqrt(0.25 / on.size) and set(on) == {True, False}
  w, h, n = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1], box[:, 5] - box[:, 4]
  assert set(w) == set(range(0, 7)) and set(h) == set(range(0, 5))                 # floor(0.5 * 12), floor(0.5 * 8)
  assert box[:, 0].min() == 0 and box[:, 1].min() == 0 and box[:, 2].max() == 12 and box[:, 3].max() == 8
  assert set(n) == {0, 1, 2} and box[:, 4].min() == 0 and box[:, 5].max() == 3
  # without `frames` the box spans the recording; number mode has no origins
  for idx, starts, aug, mix in _take(_plan(mix=dict(prob=1.0, size=1.0), split_by="number"), 5):
    assert starts is None and mix.start is None and aug is None and mix.augment is None
    assert (mix.box[:, 4] == 0).all() and (mix.box[:, 5] == 3).all() and (mix.partner == np.roll(idx, -1)).all()


def test_the_draw_order_is_the_documented_one():
  """The mix's draws replayed from a generator in the state the batch's augmentation leaves: mixed,
  width, height, x0, y0, n, g0, one array of `per` values each."""
  plan, twin = _plan(augment=AUG, mix=MIX), _plan(augment=AUG)
  it, tw = plan.mixed_batches(T_MIN, T_MAX), twin.mixed_batches(T_MIN, T_MAX)
  idx, starts, aug, mix = next(it)
  tidx, tstarts, taug, none = next(tw)
  assert none is None and np.array_equal(idx, tidx) and np.array_equal(starts, tstarts) and _aug_same(aug, taug)
  g = twin.gen                                        # after draw_augment, before the mix's draws
  u = torch.rand(4, generator=g, dtype=torch.float64).numpy()
  draw = lambda lo, hi: lo + torch.randint(0, 1 << 62, (4,), generator=g, dtype=torch.int64).numpy() % (hi - lo + 1)  # noqa: E731
  w, h = draw(0, 6), draw(0, 4)
  x0, y0 = draw(0, 12 - w), draw(0, 8 - h)
  n = draw(0, 2)
  g0 = draw(0, 3 - n)
  np.testing.assert_array_equal(mix.partner >= 0, u < 0.5)
  np.testing.assert_array_equal(mix.box, np.stack([x0, y0, x0 + w, y0 + h, g0, g0 + n], 1))
  assert torch.equal(plan.gen.get_state(), g.get_state())


def test_the_same_seed_gives_the_same_stream_and_skip_equals_consuming():
  a, b = _take(_plan(augment=AUG, mix=MIX), 7), _take(_plan(augment=AUG, mix=MIX), 7)
  assert all(_same(x, y) for x, y in zip(a, b))
  other = _take(_plan(augment=AUG, mix=MIX, seed=12), 7)
  assert not any(_same(x, y) for x, y in zip(a, other))
  for k in (1, 2, 5):                                  # (an epoch is two batches)
    tail = _take(_plan(augment=AUG, mix=MIX), 7 - k, skip=k)
    assert all(_same(x, y) for x, y in zip(a[k:], tail)), k
  # augmented_batches() and batches() are the same stream without the mix
  three = _plan(augment=AUG, mix=MIX).augmented_batches(T_MIN, T_MAX, 2)
  two = _plan(augment=AUG, mix=MIX).batches(T_MIN, T_MAX, 2)
  for x in a[2:5]:
    idx, starts, aug = next(three)
    assert np.array_equal(idx, x[0]) and np.array_equal(starts, x[1]) and _aug_same(aug, x[2])
    idx, starts = next(two)
    assert np.array_equal(idx, x[0]) and np.array_equal(starts, x[1])


def test_an_absent_key_is_todays_stream_and_prob_0_differs_by_the_mix_draws_only():
  for aug in (None, AUG):
    plain, absent, zero = _plan(augment=aug), _plan(augment=aug, mix=None), _plan(augment=aug, mix=dict(prob=0.0, size=0.5))
    today = list(zip(range(6), plain.augmented_batches(T_MIN, T_MAX)))
    a = _take(absent, 6)
    assert all(x[3] is None for x in a) and all(_same(x, y + (None,)) for x, (_, y) in zip(a, today))
    assert torch.equal(absent.gen.get_state(), plain.gen.get_state()) and absent.mix is None
    # prob = 0: every row unmixed, but the draws are made -- the first batch (drawn in front of any
    # mix draw) is today's, the generator then stands elsewhere
    z = _take(zero, 6)
    assert all((x[3].partner == -1).all() for x in z)
    assert np.array_equal(z[0][0], a[0][0]) and np.array_equal(z[0][1], a[0][1]) and _aug_same(z[0][2], a[0][2])
    assert not torch.equal(zero.gen.get_state(), plain.gen.get_state())
    # replaying today's stream with the mix's five draws after each batch gives the prob = 0 stream
    replay = _plan(augment=aug)
    it = replay.augmented_batches(T_MIN, T_MAX)
    for x in z:
      idx, starts, ag = next(it)
      assert np.array_equal(idx, x[0]) and np.array_equal(starts, x[1]) and _aug_same(ag, x[2])
      replay._uniform()
      w, h = replay._uniform_int(0, 6), replay._uniform_int(0, 4)
      replay._uniform_int(0, 12 - w), replay._uniform_int(0, 8 - h)
    assert torch.equal(replay.gen.get_state(), zero.gen.get_state())


def test_the_eval_split_never_mixes():
  a, b = _take(_plan(train=False, mix=MIX), 7), _take(_plan(train=False), 7)
  assert all(x[3] is None for x in a) and all(_same(x, y) for x, y in zip(a, b))
  assert _plan(train=False, mix=MIX).mix is None
  _plan(train=False, mix=MIX, eval_batch_size=1)      # one row per eval batch is fine: nothing is paired


def test_refusals_of_the_config():
  from snnquantprune_amd import input_pipeline as ip
  for bad in (0.5, "cutmix", [0.5, 0.5], dict(), dict(prob=0.5), dict(size=0.5), dict(prob=0.5, size=0.5, alpha=1.0),
              dict(prob=1.5, size=0.5), dict(prob=-0.1, size=0.5), dict(prob=0.5, size=1.01), dict(prob=0.5, size=float("nan")),
              dict(prob=True, size=0.5), dict(prob="x", size=0.5), dict(prob=0.5, size=0.5, frames=-1),
              dict(prob=0.5, size=0.5, frames=4), dict(prob=0.5, size=0.5, frames=1.5), dict(prob=0.5, size=0.5, frames=True)):
    for train in (True, False):
      with pytest.raises(ValueError, match="mix"):
        _plan(train=train, mix=bad)
  _plan(mix=dict(prob=1, size=1, frames=3))
  _plan(mix=dict(prob=0, size=0, frames=0))
  with pytest.raises(ValueError, match="mix"):
    _plan(mix=MIX, batch_size=1)                      # a per-rank batch of one row has no partner
  with pytest.raises(ValueError, match="mix"):
    ip.EventPlan(_config(mix=MIX, batch_size=4), (16, 24), N_SAMPLES, train=True, world=4)
  # an image source and a frame source refuse the key
  images = {"image": np.zeros((8, 4, 4), np.uint8), "label": np.zeros(8, np.int64)}
  frames = {"dvs_matrix": np.zeros((8, 3, 4, 4, 2), np.uint8), "label": np.zeros(8, np.int64)}
  for train in (True, False):
    with pytest.raises(ValueError, match="mix"):
      ip.ImagePlan(_config(mix=MIX), (4, 4), 8, train=train)
    with pytest.raises(ValueError, match="mix"):
      ip.create_split(images, _config(mix=MIX), train=train, cache=False, device="cpu")
    with pytest.raises(ValueError, match="mix"):
      ip.create_split(frames, _config(mix=MIX), train=train, cache=False)
  next(ip.create_split(frames, _config(), train=False, cache=False))


# ---- ops.EventMix and ops.events_bin on the host ----------------------------------------------------

def test_event_mix_validates_on_the_host():
  from snnquantprune_amd import ops
  lo, hi = -2 ** 31, 2 ** 31 - 1
  box = [[lo, lo, hi, hi, 0, 3], [5, 5, 2, 2, 2, 2]]
  m = ops.EventMix(2, partner=[1, -1], start=torch.tensor([7, -9]), box=box, augment=ops.EventAugment(2, dx=[1, 2]))
  partner, b, rec = m.records(3)
  assert partner.dtype == np.int32 and partner.tolist() == [1, -1] and b.dtype == np.int32 and b.tolist() == box
  np.testing.assert_array_equal(rec, ea.records([ea.params(dx=1), ea.params(dx=2)]))
  assert m.start.tolist() == [7, -9] and ops.EventMix(2, partner=[0, 0], box=box).records(3)[2] is None
  assert ops.EventMix(0, partner=[], box=np.zeros((0, 6))).records(0)[1].shape == (0, 6)
  with pytest.raises(ValueError, match="box"):
    m.records(2)                                      # g1 = 3 > T
  with pytest.raises(ValueError, match="frames"):
    ops.EventMix(2, partner=[0, 0], box=box, augment=ops.EventAugment(2, frames=[[0, 3], [0, 0]])).records(2)
  ok = dict(partner=[0, 1], box=box)
  for key, bad in (("partner", [0]), ("partner", [0, -2]), ("partner", [0, 2 ** 31]), ("partner", [0.5, 1.0]),
                   ("start", [0]), ("start", [0, 2 ** 31]), ("box", [[0, 0, 1, 1, 0, 1]]), ("box", [[0, 0, 1, 1]] * 2),
                   ("box", [[0, 0, 1, hi + 1, 0, 1]] * 2), ("box", [[0, lo - 1, 1, 1, 0, 1]] * 2),
                   ("box", [[0, 0, 1, 1, 2, 1]] * 2), ("box", [[0, 0, 1, 1, -1, 1]] * 2), ("box", [[0.5, 0, 1, 1, 0, 1]] * 2),
                   ("augment", ops.EventAugment(3)), ("augment", {"dx": [0, 0]})):
    with pytest.raises(ValueError, match="mix" if key in ("start", "augment") else key):
      ops.EventMix(2, **dict(ok, **{key: bad}))
  with pytest.raises(ValueError, match="rows"):
    ops.EventMix(-1, partner=[], box=[])


def test_events_bin_validates_the_mix_before_any_upload():
  from snnquantprune_amd import ops
  rng = RNG(7)
  ev = ec.make_set([ec.make_sample(rng, n, 20, 30, t_lo=10, t_hi=500) for n in (50, 0, 7)])
  es = ops.EventSet(ev["addrs"], ev["times"], ev["offsets"], (20, 30))
  box = [[0, 0, 5, 5, 0, 3]] * 2
  with pytest.raises(ValueError, match="mix"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="number", mix=ops.EventMix(3, partner=[0] * 3, box=box[:1] * 3))
  with pytest.raises(ValueError, match="mix"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="number", mix={"partner": [0, 0]})
  with pytest.raises(ValueError, match="partner"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="number", mix=ops.EventMix(2, partner=[0, 3], box=box))
  with pytest.raises(ValueError, match="box"):
    ops.events_bin(es, [0, 1], 2, 20, 30, mode="number", mix=ops.EventMix(2, partner=[0, 2], box=box))
  with pytest.raises(ValueError, match="start"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="time", start=[0, 0], step_us=10, mix=ops.EventMix(2, partner=[0, 2], box=box))
  # a valid one reaches the same refusal as the plain call: CPU tensors
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="time", start=[0, 0], step_us=10,
                   mix=ops.EventMix(2, partner=[2, -1], start=[5, 5], box=box), augment=ops.EventAugment(2))


# ---- the C entry point's argument checks ----------------------------------------------------------

def test_events_bin_mix_argument_errors_without_a_gpu():
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  p = ctypes.c_void_p(64)                                  # never dereferenced: the checks come first

  for aug in (p, None):
    def call(S=1, B=1, mode=1, T=1, step=10, H=4, W=4, scale=1.0, out_type=L.U8, times=p, start=p, sample2=p, start2=p,
             aug2=aug, box=p, counts=p):
      return lib.snnqp_events_bin_mix(None, times, None, S, None, start, aug, sample2, start2, aug2, box, counts, B, mode,
                                      T, step, H, W, scale, None, out_type, None, None)

    # snnqp_events_bin's refusals
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
    assert call() == L.EINVAL and b"null" in lib.snnqp_last_error()
    # its own: a partner array without boxes, and without origins in time mode -- before B == 0 returns
    for B in (0, 1):
      assert call(B=B, box=None) == L.EINVAL and b"box" in lib.snnqp_last_error()
      assert call(B=B, start2=None) == L.EINVAL and b"start2" in lib.snnqp_last_error()
      assert call(B=B, mode=0, box=None, times=None, start=None, step=0) == L.EINVAL and b"box" in lib.snnqp_last_error()
    assert call(mode=0, start2=None, times=None, start=None, step=0) == L.EINVAL and b"null" in lib.snnqp_last_error()
    assert call(sample2=None, start2=None, box=None, counts=None) == L.EINVAL and b"null" in lib.snnqp_last_error()
    assert call(B=0) == L.OK and call(T=0) == L.OK and call(mode=0, B=0, times=None, start=None, start2=None) == L.OK
    assert call(B=0, sample2=None, start2=None, box=None, counts=None, aug2=None) == L.OK
    assert call(B=0, out_type=9) == L.EINVAL


# ---- soft targets -----------------------------------------------------------------------------------

def test_mixed_targets():
  from snnquantprune_amd import train_utils as tu
  y, y2 = torch.tensor([0, 2, 1, 1], dtype=torch.int8), torch.tensor([1, 2, 0, 1])
  w = torch.tensor([0.25, 0.5, 1.0, 0.0])
  t = tu.mixed_targets(y, y2, w, 3)
  assert t.dtype == torch.float32 and tuple(t.shape) == (4, 3)
  assert t.tolist() == [[0.25, 0.75, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]
  assert torch.equal(t.sum(1), torch.ones(4))
  assert torch.equal(tu.mixed_targets(y, y2, torch.ones(4), 3), tu.onehot(y, 3))


@pytest.mark.parametrize("smoothing", [0, 0.1])
def test_losses_on_soft_targets(smoothing):
  from snnquantprune_amd import train_utils as tu
  g = torch.Generator()
  g.manual_seed(3)
  B, C = 6, 5
  logits = torch.randn(B, C, generator=g, dtype=torch.float64) * 3
  y, y2 = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
  w = torch.rand(B, generator=g, dtype=torch.float64)
  soft = w[:, None] * tu.onehot(y, C).double() + (1 - w[:, None]) * tu.onehot(y2, C).double()
  # cross entropy is linear in the target: the weighted sum of the two rows' losses, row by row.
  # Without smoothing the two are the integer-label calls.  With it those smooth their one-hot in
  # float32, as they always have (an error of 1e-7 that is theirs), so the float64 one-hot stands in.
  hard = (lambda lab: lab) if smoothing == 0 else (lambda lab: tu.onehot(lab, C).double())   # noqa: E731
  rows = lambda lab: torch.stack([tu.cross_entropy_loss(logits[b:b + 1], hard(lab[b:b + 1]), smoothing)   # noqa: E731
                                  for b in range(B)])
  want = (w * rows(y) + (1 - w) * rows(y2)).mean()
  got = tu.cross_entropy_loss(logits, soft, smoothing)
  assert got.dtype == torch.float64 and abs(float(got - want)) <= 1e-12
  sm = soft * (1 - smoothing) + smoothing / C
  assert abs(float(tu.mse_loss(logits, soft, smoothing) - torch.mean((logits - sm) ** 2))) <= 1e-12
  # w = 1: the integer-label call, exactly -- in float64 and in float32
  for lg in (logits, logits.float()):
    one = tu.mixed_targets(y, y2, torch.ones(B), C)
    assert torch.equal(tu.cross_entropy_loss(lg, one, smoothing), tu.cross_entropy_loss(lg, y, smoothing))
    assert torch.equal(tu.mse_loss(lg, one, smoothing), tu.mse_loss(lg, y, smoothing))
    assert torch.equal(tu.mse_loss(lg, one, smoothing, T=2), tu.mse_loss(lg, y, smoothing, T=2))
  with pytest.raises(ValueError, match="soft target"):
    tu.cross_entropy_loss(logits, soft[:, :4])
