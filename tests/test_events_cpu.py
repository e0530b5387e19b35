"""The batched event front end without a GPU: the numpy restatement of tests/event_cases.py against
the oracle and a per-event loop, that its cases cover what they claim, ops.EventSet on CPU
tensors, snnqp_events_bin's argument checks, and the pipeline's planning (input_pipeline.EventPlan)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import event_cases as ec

RNG = lambda seed: np.random.Generator(np.random.PCG64(seed))


# ---- the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_number_mode_equals_the_oracle(oracle, scale):
  rng = RNG(3)
  H, W = 9, 13
  for n, T in ((0, 3), (2, 3), (3, 3), (500, 7), (1000, 20)):
    addrs, _ = ec.make_sample(rng, n, H, W, scale, outside=False)     # (the oracle wraps what falls outside)
    want = oracle.events_to_frames(addrs[:, 0], addrs[:, 1], addrs[:, 2], T, H, W, scale)
    np.testing.assert_array_equal(ec.decode_number(addrs, T, H, W, scale), want)
    np.testing.assert_array_equal(ec.decode_number(addrs, T, H, W, scale, frame=ec.frame_of), want)
  assert ec.decode_number(addrs, 20, H, W, scale).sum() == 1000


def test_time_mode_equals_a_per_event_loop():
  rng = RNG(4)
  H, W, T, start, step, scale = 6, 5, 4, 700, 90, 2.0
  addrs, times = ec.edge_sample(rng, 400, H, W, T, start, step, scale)
  want = np.zeros((T, H, W, 2), np.int64)
  on_edge = dropped = odd_polarity = 0
  for (x, y, p), t in zip(addrs, times):
    xs, ys = int(np.floor(np.float32(x) / np.float32(scale))), int(np.floor(np.float32(y) / np.float32(scale)))
    for f in range(T):
      if start + f * step < t < start + (f + 1) * step:
        if 0 <= xs < W and 0 <= ys < H:
          want[f, ys, xs, 0 if p == 0 else 1] += 1
          odd_polarity += p not in (0, 1)
        else:
          dropped += 1
    on_edge += (t - start) % step == 0 and 0 < (t - start) // step < T
  for frame in (ec.frame_of, ec.frame_of_fast):
    np.testing.assert_array_equal(ec.decode_time(addrs, times, start, step, T, H, W, scale, frame=frame), want)
  # the case is what it claims: events on a lower and on an upper edge, in no frame; events out of
  # range, dropped; polarities that are neither 0 nor 1, counted in channel 1
  assert np.any(times == start) and np.any(times == start + T * step) and np.any(times == start + step)
  inside = (times > start) & (times < start + T * step)
  assert on_edge >= T - 1 and want.sum() + dropped == inside.sum() - on_edge      # (on_edge: the inner edges)
  assert dropped > 0 and odd_polarity > 0
  assert np.any(times < start) and np.any(times > start + T * step)


def test_batch_rows_and_starts():
  rng = RNG(5)
  H, W, T, step = 4, 6, 3, 50
  ev = ec.make_set([ec.edge_sample(rng, n, H, W, T, 100 * (i + 1), step) for i, n in enumerate((40, 0, 90))])
  sample, start = [2, 0, 2, 1, 0], [300, 100, 330, 0, 10 ** 6]
  got = ec.decode_batch(ev, sample, T, H, W, "time", start, step)
  off = ev["offsets"]
  for b, s in enumerate(sample):
    np.testing.assert_array_equal(got[b], ec.decode_time(ev["addrs"][off[s]:off[s + 1]], ev["times"][off[s]:off[s + 1]],
                                                         start[b], step, T, H, W))
  assert got[0].sum() > 0 and got[1].sum() > 0 and not np.array_equal(got[0], got[2])
  assert got[3].sum() == 0 and got[4].sum() == 0          # the empty sample; windows beyond the recording
  num = ec.decode_batch(ev, sample, T, H, W, "number")
  np.testing.assert_array_equal(num[0], num[2])
  assert num[0].sum() <= 90 and num[3].sum() == 0


@pytest.mark.parametrize("count,pol", ec.HOT_CASES)
def test_hot_pixel_cases_expose_a_16_bit_counter(count, pol):
  rng = RNG(6)
  H = W = 34
  step = 5000
  addrs, times, (hx, hy) = ec.hot_sample(rng, H, W, step, count=count, polarity=pol)
  assert addrs.shape[0] == ec.HOT_N
  exposed = []
  for counts in (ec.decode_time(addrs, times, 0, step, 3, H, W), ec.decode_number(addrs, 1, H, W)):
    assert counts[0, hy, hx, pol] == count >= 65536 and counts[0, hy, hx, 1 - pol] == 0
    u8, f = ec.wire(counts, None)
    assert u8[0, hy, hx, pol] == 255 and u8[0, hy, hx, 1 - pol] == 0 and f == 0
    e4, f4 = ec.wire(counts, ec.EV4)
    assert e4[0, hy * W + hx] == (0xF0 if pol else 0x0F) and f4 == ec.FLAG_GT_15
    e1, f1 = ec.wire(counts, ec.EV1)
    i = (hy * W + hx) * 2
    assert (e1[0, i >> 5] >> (i & 31)) & 3 == (2 if pol else 1) and f1 == ec.FLAG_GT_ONE
    # packed 16-bit halves with nothing done about overflow would give other frames: in which formats?
    bad = ec.wrapped_halves(counts)
    exposed.append([not np.array_equal(ec.wire(bad, fmt)[0], ec.wire(counts, fmt)[0]) for fmt in (None, ec.EV4, ec.EV1)])
  # a lost carry of the low half shows in every format (the silent polarity 1 reads 1); of the high half
  # only through the residue: 66 000 leaves 464, which saturates all the same, 65 539 leaves 3
  want = [True, True, True] if pol == 0 else [count == 65539, count == 65539, False]
  assert exposed == [want, want], exposed
  assert ec.decode_time(addrs, times, 0, step, 3, H, W)[1:].sum() > 0


def test_clean_streams_set_no_flag():
  rng = RNG(6)
  # clean twins: a stream of distinct (pixel, polarity) events sets no flag, and its frames are the counts
  a, _ = ec.make_sample(rng, 60, 5, 7, unique=True)
  c = ec.decode_number(a, 3, 5, 7)
  assert c.max() == 1 and c.sum() == 60
  e1, f1 = ec.wire(c, ec.EV1)
  e4, f4 = ec.wire(c, ec.EV4)
  assert f1 == 0 and f4 == 0 and e1.shape == (3, 3) and e4.shape == (3, 35)
  bits = np.unpackbits(e1.view(np.uint8), axis=-1, bitorder="little")[:, :70]
  np.testing.assert_array_equal(bits.reshape(3, 5, 7, 2), c)
  np.testing.assert_array_equal(np.stack([e4 & 15, e4 >> 4], -1).reshape(3, 5, 7, 2), c)


# ---- EventSet on CPU tensors --------------------------------------------------------------------

def test_event_set_packs_validates_and_sorts():
  from snnquantprune_amd import ops
  rng = RNG(7)
  ev = ec.make_set([ec.make_sample(rng, n, 20, 30, t_lo=10, t_hi=500) for n in (50, 0, 7)])
  ev["addrs"][3] = (16383, 16383, 255)
  es = ops.EventSet(torch.from_numpy(ev["addrs"]), torch.from_numpy(ev["times"]), torch.from_numpy(ev["offsets"]), (20, 30))
  assert es.num_samples == 3 and es.num_events == 57 and not es.sorted_by_time and es.sensor_size == (20, 30)
  assert es.addr.dtype == torch.int32 and es.times.dtype == torch.int32 and es.offsets.dtype == torch.int64
  want = ev["addrs"].copy()
  want[:, 2] = want[:, 2] != 0
  np.testing.assert_array_equal(es.unpack().numpy(), want)
  np.testing.assert_array_equal(es.times.numpy(), ev["times"])
  np.testing.assert_array_equal(es.t_min, [ev["times"][0], 0, ev["times"][50]])
  np.testing.assert_array_equal(es.t_max, [ev["times"][49], 0, ev["times"][56]])
  assert ops.EventSet(ev["addrs"], ev["times"], ev["offsets"], 128).sensor_size == (128, 128)
  for bad in ([1, 50, 57], [0, 50, 50, 56], [0, 51, 50, 57], []):
    with pytest.raises(ValueError, match="offsets"):
      ops.EventSet(ev["addrs"], ev["times"], np.asarray(bad, np.int64), (20, 30))
  for col, v in ((0, 16384), (1, 16384), (0, -1)):
    a = ev["addrs"].copy()
    a[5, col] = v
    with pytest.raises(ValueError, match="coordinates"):
      ops.EventSet(a, ev["times"], ev["offsets"], (20, 30))
  for v in (2 ** 31, -2 ** 31 - 1):
    t = ev["times"].copy()
    t[56] = v
    with pytest.raises(ValueError, match="int32"):
      ops.EventSet(ev["addrs"], t, ev["offsets"], (20, 30))
  # a sample's first event may be earlier than the previous sample's last: nothing to sort
  assert ev["times"][50] < ev["times"][49]
  # an unsorted sample is sorted stably, once, and the set then refuses number mode (on the host,
  # before any device is asked for)
  t = ev["times"].copy()
  t[52], t[55] = t[55] + 5, t[52]
  t[53] = t[54]
  es2 = ops.EventSet(ev["addrs"], t, ev["offsets"], (20, 30))
  assert es2.sorted_by_time
  order = 50 + np.argsort(t[50:], kind="stable")
  np.testing.assert_array_equal(es2.times.numpy()[50:], t[order])
  np.testing.assert_array_equal(es2.unpack().numpy()[50:], want[order])
  np.testing.assert_array_equal(es2.unpack().numpy()[:50], want[:50])
  with pytest.raises(ValueError, match="number mode"):
    ops.events_bin(es2, [0], 3, 20, 30, mode="number")
  # rows and starts are validated on the host as well
  with pytest.raises(ValueError, match="sample"):
    ops.events_bin(es, [0, 3], 3, 20, 30, mode="number")
  with pytest.raises(ValueError, match="sample"):
    ops.events_bin(es, [-1], 3, 20, 30, mode="number")
  with pytest.raises(ValueError, match="start"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="time", start=[0, 2 ** 31], step_us=10)
  with pytest.raises(ValueError, match="start"):
    ops.events_bin(es, [0, 1], 3, 20, 30, mode="time", start=[0], step_us=10)
  with pytest.raises(ValueError, match="step_us"):
    ops.events_bin(es, [0], 3, 20, 30, mode="time", start=[0], step_us=0)
  with pytest.raises(ValueError, match="time mode needs"):
    ops.events_bin(es, [0], 3, 20, 30, mode="time")
  with pytest.raises(RuntimeError, match="GPU only"):
    ops.events_bin(es, [0], 3, 20, 30, mode="number")


# ---- the C entry point's argument checks --------------------------------------------------------

def test_events_bin_argument_errors_without_a_gpu():
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  p = ctypes.c_void_p(64)                                  # never dereferenced: the checks come first

  def call(S=1, B=1, mode=1, T=1, step=10, H=4, W=4, scale=1.0, out_type=L.U8, times=p, start=p):
    return lib.snnqp_events_bin(None, times, None, S, None, start, B, mode, T, step, H, W, scale, None,
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
  # number mode needs neither; with valid arguments the null tensors are what is refused
  assert call(mode=0, times=None, start=None, step=0) == L.EINVAL and b"null" in lib.snnqp_last_error()
  assert call() == L.EINVAL and b"null" in lib.snnqp_last_error()
  # nothing to do: no launch, no pointer looked at
  assert call(B=0) == L.OK and call(T=0) == L.OK and call(mode=0, B=0, times=None, start=None) == L.OK
  assert call(B=0, out_type=9) == L.EINVAL


# ---- planning: shuffle and window origins -------------------------------------------------------

def _config(**kw):
  from snnquantprune_amd import synthetic as syn
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  cfg.split_by, cfg.num_frames, cfg.resolution_scale = "time", 3, 2
  cfg.time_step, cfg.input_scale, cfg.train_chunk_size, cfg.test_chunk_size = 1, 1, 4, 7
  cfg.batch_size, cfg.eval_batch_size, cfg.seed, cfg.feed_format = 4, 2, 11, "u8"
  for k, v in kw.items():
    setattr(cfg, k, v)
  return cfg


def test_plan_is_reproducible_and_follows_the_formula():
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import input_pipeline as ip
  n = 10
  # recordings of 30 ms, one shorter than two chunks (tend == tbegin) and an empty one
  t_min = np.array([1000 + 10 * i for i in range(n)], np.int64)
  t_max = t_min + 30000
  t_max[3] = t_min[3] + 7999
  t_min[6] = t_max[6] = 0

  def take(plan, k):
    it = plan.batches(t_min, t_max)
    return [next(it) for _ in range(k)]

  train = ip.EventPlan(_config(), (16, 16), n, train=True)
  assert (train.H, train.W, train.T, train.step_us, train.chunk_ms, train.per, train.nb) == (8, 8, 3, 1000, 4, 4, 2)
  assert train.divisor is None and train.fmt is None
  lo, hi = train.start_range(t_min, t_max)
  np.testing.assert_array_equal(lo, t_min)
  np.testing.assert_array_equal(hi, np.maximum(t_min, t_max - 2 * 4 * 1000))
  assert hi[3] == lo[3] and hi[6] == lo[6] == 0 and hi[0] == lo[0] + 22000
  a, b = take(train, 6), take(ip.EventPlan(_config(), (16, 16), n, train=True), 6)
  for (ia, sa), (ib, sb) in zip(a, b):
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(sa, sb)
    assert ia.shape == (4,) and np.all(lo[ia] <= sa) and np.all(sa <= hi[ia])
  # an epoch is a permutation of the slice with the remainder dropped; epochs differ
  e0, e1, e2 = (np.concatenate([a[2 * e][0], a[2 * e + 1][0]]) for e in range(3))
  assert len(set(e0)) == 8 and set(e0) <= set(range(n)) and not np.array_equal(e0, e1) and not np.array_equal(e1, e2)
  other = take(ip.EventPlan(_config(seed=12), (16, 16), n, train=True), 2)
  assert not all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, other))
  # the origins use the range: many draws of one recording reach both halves of it, never leave it
  draws = np.concatenate([train.draw_starts(t_min[:1].repeat(64), t_max[:1].repeat(64)) for _ in range(8)])
  assert draws.min() >= lo[0] and draws.max() <= hi[0] and draws.min() < lo[0] + 2000 and draws.max() > hi[0] - 2000
  np.testing.assert_array_equal(train.draw_starts(t_min[[3, 6]], t_max[[3, 6]]), [lo[3], 0])

  # eval: in order, test_chunk_size, the same origins every pass
  ev = ip.EventPlan(_config(), (16, 16), n, train=False)
  assert (ev.chunk_ms, ev.per, ev.nb) == (7, 2, 5)
  passes = take(ev, 10)
  for i in range(5):
    np.testing.assert_array_equal(passes[i][0], [2 * i, 2 * i + 1])
    np.testing.assert_array_equal(passes[i][1], passes[5 + i][1])
  lo7, hi7 = ev.start_range(t_min, t_max)
  assert hi7[0] == lo7[0] + 16000 and all(np.all((lo7[i] <= s) & (s <= hi7[i])) for i, s in passes)

  # number mode: no origins, frames in feed_format
  num = ip.EventPlan(_config(split_by="number", feed_format="ev4"), (16, 16), n, train=False)
  assert num.fmt == L.EV4 and num.step_us is None and take(num, 1)[0][1] is None
  # time_step * input_scale: 1 keeps the counts in feed_format, anything else makes float32 batches
  assert ip.EventPlan(_config(time_step=2, input_scale=0.5, feed_format="ev1"), (16, 16), n, train=False).fmt == L.EV1
  p = ip.EventPlan(_config(time_step=5, input_scale=2), (16, 16), n, train=False)
  assert p.divisor == np.float32(10) and p.step_us == 5000
  with pytest.raises(ValueError, match="feed_format"):
    ip.EventPlan(_config(time_step=5, feed_format="ev4"), (16, 16), n, train=False)
  with pytest.raises(ValueError, match="feed_format"):
    ip.EventPlan(_config(split_by="number", feed_format="ev1"), (16, 16), n, train=True)
  with pytest.raises(ValueError, match="batch_size"):
    ip.EventPlan(_config(batch_size=16), (16, 16), n, train=True)
  # two ranks: half the batch each, different draws
  r1 = ip.EventPlan(_config(), (16, 16), n // 2, train=True, rank=1, world=2)
  assert r1.per == 2 and r1.nb == 2 and r1.seed == 12


def test_load_source_tells_event_sources_from_frame_sources(tmp_path):
  from snnquantprune_amd import input_pipeline as ip
  rng = RNG(8)
  ev = ec.make_set([ec.make_sample(rng, n, 8, 8) for n in (5, 0, 9)])
  src = dict(ev, label=np.array([1, 2, 3]), sensor_size=np.array(8))
  path = str(tmp_path / "events.npz")
  np.savez(path, **src)
  for s in (src, path):
    d = ip.load_source(s)
    assert ip.is_event_source(d) and d["label"].dtype == np.int8 and list(d["sensor_size"]) == [8, 8]
    np.testing.assert_array_equal(d["offsets"], ev["offsets"])
  with pytest.raises(ValueError, match="offsets"):
    ip.load_source(dict(src, label=np.array([1, 2])))
  frames = {"dvs_matrix": np.zeros((4, 3, 8, 8, 2), np.uint8), "label": np.arange(4)}
  d = ip.load_source(frames)
  assert not ip.is_event_source(d) and set(d) == {"dvs_matrix", "label"}
  with pytest.raises(NotImplementedError):
    ip.create_split(frames, _config(), train=True, cache=False)
