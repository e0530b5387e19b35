"""ops.events_bin (snnqp_events_bin, csrc/events.hip) on the GPU, bit for bit against the numpy
restatement of tests/event_cases.py: every output format with its flag word, both modes, frames
from one pixel to the banded 240 x 240, ragged and empty samples, events on window edges, a pixel
hotter than a 16-bit counter, guarded output buffers; number mode against the per-sample
ops.events_to_frames (+ ops.pack_frames) it replaces; and the pipeline on an event source -- an
eval against the same frames fed as a frame source, two train steps from the train split."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import conv_train_reference as cr
from tests import event_cases as ec

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 7), (34, 34), (128, 128), (240, 240)]
SCALES = {(5, 7): 3.0, (34, 34): 2.0}          # the others decode at scale 1
FRAMES = [1, 3, 20]
START, STEP = 5000, 300
SENTINEL = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A}


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _np(t):
  return t.detach().cpu().numpy()


def _event_set(ev, hw, dev):
  from snnquantprune_amd import ops
  return ops.EventSet(ev["addrs"], ev["times"], ev["offsets"], hw, device=dev)


def _bin_guarded(es, sample, T, H, W, fmt, dev, guard=64, **kw):
  """events_bin into the middle of a sentinel-filled buffer -> (result array, flag word); asserts
  that nothing outside the result was written."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  packed = fmt in (L.EV1, L.EV4)
  shape = (len(sample), T, ops.frame_units(H, W, fmt)) if packed else (len(sample), T, H, W, 2)
  dtype = torch.int32 if fmt == L.EV1 else torch.uint8
  n = int(np.prod(shape))
  buf = torch.full((guard + n + guard,), SENTINEL[dtype], dtype=dtype, device=dev)
  flags = torch.zeros(1, dtype=torch.int32, device=dev)
  got = ops.events_bin(es, sample, T, H, W, fmt=fmt, flags=flags, out=buf[guard:guard + n].view(shape), **kw)
  data = got.data if packed else got
  assert data.data_ptr() == buf.data_ptr() + guard * buf.element_size()
  torch.cuda.synchronize()
  assert bool((buf[:guard] == SENTINEL[dtype]).all()) and bool((buf[guard + n:] == SENTINEL[dtype]).all())
  return _np(data), int(flags.item())


def _check_all_formats(es, ev, sample, T, H, W, mode, dev, scale=1.0, start=None, guard=64):
  """Every format against the restatement (the flag word included); returns the counts."""
  from snnquantprune_amd import _lib as L
  kw = dict(mode=mode, scale=scale)
  if mode == "time":
    kw.update(start=start, step_us=STEP)
  want = ec.decode_batch(ev, sample, T, H, W, mode, start, STEP, scale)
  for fmt in (None, L.EV4, L.EV1):
    exp, exp_flag = ec.wire(want, fmt)
    got, flag = _bin_guarded(es, sample, T, H, W, fmt, dev, guard=guard, **kw)
    assert got.shape == exp.shape and got.dtype == exp.dtype
    np.testing.assert_array_equal(got, exp, err_msg="format %r" % (fmt,))
    assert flag == exp_flag, (fmt, flag, exp_flag)
  return want


_sets = {}


def _ragged(dev, hw, T):
  """The ragged set of a (size, T): samples of 0, 1, T - 1, T and 1000 events (shared, never modified)."""
  if (hw, T) not in _sets:
    H, W = hw
    scale = SCALES.get(hw, 1.0)
    ev = ec.ragged_set(100 * H + T, H, W, T, START, STEP, scale)
    _sets[(hw, T)] = (ev, _event_set(ev, (int(H * scale), int(W * scale)), dev), scale)
  return _sets[(hw, T)]


@pytest.mark.parametrize("mode", ["number", "time"])
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("hw", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_ragged_samples_every_format(dev, hw, T, mode):
  H, W = hw
  ev, es, scale = _ragged(dev, hw, T)
  sample = [3, 0, 4, 1, 2]
  want = _check_all_formats(es, ev, sample, T, H, W, mode, dev, scale, start=[START] * 5)
  # the cases are not vacuous: the long sample fills frames, the empty one yields zero frames, and
  # in time mode the events on the window edges are in no frame
  assert want[1].sum() == 0 and want[2].sum() > 0
  if mode == "number" and hw != (1, 1):
    assert want[2, -1].sum() > 0 and want[3].sum() <= 1 and want[3, :-1].sum() == 0
  if mode == "time":
    off, t = ev["offsets"], ev["times"]
    long = t[off[4]:off[5]]
    inner = sum(int(np.sum(long == START + f * STEP)) for f in range(1, T))
    assert np.any(long == START) and np.any(long == START + T * STEP)
    assert want[2].sum() <= int(np.sum((long > START) & (long < START + T * STEP))) - inner


@pytest.mark.parametrize("mode", ["number", "time"])
def test_batch_rows_pick_permute_and_repeat_samples(dev, mode):
  """B = 5 rows over S = 3 ragged samples: permuted, one repeated, one empty; in time mode one row's
  origin leaves part of its windows beyond the recording and another's all of them."""
  H, W, T = 34, 34, 3
  rng = np.random.Generator(np.random.PCG64(41))
  ev = ec.make_set([ec.edge_sample(rng, 900, H, W, T, START, STEP), ec.edge_sample(rng, 0, H, W, T, START, STEP),
                    ec.edge_sample(rng, 350, H, W, T, START + 40, STEP)])
  es = _event_set(ev, (H, W), dev)
  sample = [2, 0, 2, 1, 0]
  t_max = int(ev["times"][:900].max())
  start = [START + 40, START, START + 2 * STEP, START, t_max + 1]
  want = _check_all_formats(es, ev, sample, T, H, W, mode, dev, start=start)
  assert want[0].sum() > 0 and want[1].sum() > 0 and want[3].sum() == 0
  if mode == "time":
    assert want[2, 0].sum() > 0 and want[2, 2].sum() == 0 and want[4].sum() == 0
    assert not np.array_equal(want[0], want[2])
  else:
    np.testing.assert_array_equal(want[0], want[2])


@pytest.mark.parametrize("count,pol", ec.HOT_CASES)
@pytest.mark.parametrize("mode,T", [("time", 3), ("number", 1)])
def test_hot_pixel_beyond_a_16_bit_counter(dev, mode, T, count, pol):
  """One frame of a 70 000-event sample puts 66 000 (65 539) events on one pixel and polarity: exact
  until it saturates, the other polarity of the pixel and its neighbours untouched, flags set.  On
  polarity 0 a lost carry would show in the pixel's polarity 1; on polarity 1 a wrapped count of
  65 539 would read 3 (tests/test_events_cpu.py models both)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  H = W = 34
  rng = np.random.Generator(np.random.PCG64(43))
  addrs, times, (hx, hy) = ec.hot_sample(rng, H, W, STEP, count=count, polarity=pol)
  quiet = ec.make_sample(rng, 40, H, W, unique=True, t_lo=1, t_hi=3 * STEP)
  ev = ec.make_set([(addrs, times), quiet])
  es = _event_set(ev, (H, W), dev)
  want = _check_all_formats(es, ev, [1, 0], T, H, W, mode, dev, start=[0, 0])
  assert want[1, 0, hy, hx, pol] == count >= 65536 and want[1, 0, hy, hx, 1 - pol] == 0 and want[0].max() <= 1
  kw = dict(start=[0, 0], step_us=STEP) if mode == "time" else {}
  u8 = _np(ops.events_bin(es, [1, 0], T, H, W, mode=mode, **kw))
  assert u8[1, 0, hy, hx, pol] == 255 and u8[1, 0, hy, hx, 1 - pol] == 0
  # without the hot sample in the batch the flags stay clear
  for fmt in (L.EV4, L.EV1):
    _, flag = _bin_guarded(es, [1, 1], T, H, W, fmt, dev, mode=mode, **kw)
    assert flag == 0


@pytest.mark.parametrize("hw", [(5, 7), (34, 34)], ids=["5x7", "34x34"])
def test_output_at_an_odd_address(dev, hw):
  """Frames that begin on no 8- or 4-byte boundary (the byte path of the uint8 / EV4 epilogues)."""
  H, W = hw
  ev, es, scale = _ragged(dev, hw, 3)
  for mode in ("number", "time"):
    _check_all_formats(es, ev, [4, 3, 4], 3, H, W, mode, dev, scale, start=[START] * 3, guard=3)


def test_two_calls_give_identical_bytes(dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  ev, es, scale = _ragged(dev, (128, 128), 20)
  for fmt in (None, L.EV4, L.EV1):
    a = ops.events_bin(es, [4, 4, 3], 20, 128, 128, mode="time", start=[START, START + 7, START], step_us=STEP, fmt=fmt)
    b = ops.events_bin(es, [4, 4, 3], 20, 128, 128, mode="time", start=[START, START + 7, START], step_us=STEP, fmt=fmt)
    assert torch.equal(a.data if fmt else a, b.data if fmt else b)
  empty = ops.events_bin(es, [], 20, 128, 128, mode="number")
  assert tuple(empty.shape) == (0, 20, 128, 128, 2)
  # a set of samples without a single event: zero frames
  none = _event_set(ec.make_set([ec.make_sample(np.random.default_rng(0), 0, 5, 7)] * 2), (5, 7), dev)
  for mode in ("number", "time"):
    z = ops.events_bin(none, [1, 0, 1], 3, 5, 7, mode=mode, start=[0, 0, 0], step_us=10, fmt=L.EV1)
    assert tuple(z.shape) == (3, 3, 5, 7, 2) and not bool(z.data.any())


@pytest.mark.parametrize("mode", [0, 1], ids=["number", "time"])
def test_rows_outside_the_set_yield_zero_frames(dev, mode):
  """The C entry point alone (ops.events_bin refuses such rows on the host): sample[b] outside
  [0, S) gives zero frames for that row, in every format."""
  import ctypes
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  H, W, T = 34, 34, 3
  ev, es, scale = _ragged(dev, (H, W), T)
  rows = torch.tensor([-1, 4, es.num_samples, 2 ** 31 - 1], dtype=torch.int32, device=dev)
  start = torch.full((4,), START, dtype=torch.int32, device=dev)
  want = ec.decode_batch(ev, [4], T, H, W, "number" if mode == 0 else "time", [START], STEP, scale)[0]
  for fmt in (L.U8, L.EV4, L.EV1):
    units = ops.frame_units(H, W, fmt) if fmt != L.U8 else H * W * 2
    out = torch.full((4, T, units), SENTINEL[torch.int32 if fmt == L.EV1 else torch.uint8],
                     dtype=torch.int32 if fmt == L.EV1 else torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L.check(L.lib().snnqp_events_bin(p(es.addr), p(es.times), p(es.offsets), es.num_samples, p(rows), p(start), 4,
                                     mode, T, STEP, H, W, scale, p(out), fmt, None,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = _np(out)
    assert not got[0].any() and not got[2].any() and not got[3].any()
    np.testing.assert_array_equal(got[1], ec.wire(want, fmt)[0].reshape(T, units))


def test_a_set_of_empty_samples_needs_no_event_array(dev):
  """The C entry point with a null addr and S = 2 samples without an event (number mode reads no
  times either): the launch itself writes the zero frames."""
  import ctypes
  from snnquantprune_amd import _lib as L
  off = torch.zeros(3, dtype=torch.int64, device=dev)
  rows = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
  out = torch.full((3, 2, 5 * 7 * 2), 0xA5, dtype=torch.uint8, device=dev)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  L.check(L.lib().snnqp_events_bin(None, None, p(off), 2, p(rows), None, 3, 0, 2, 0, 5, 7, 1.0, p(out), L.U8, None,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
  torch.cuda.synchronize()
  assert not bool(out.any())


def test_number_mode_equals_events_to_frames_and_feeds_the_model(dev):
  """Number mode against the path it replaces -- one ops.events_to_frames per sample, then
  ops.pack_frames -- on the same streams: the same bytes in every format, and a small ConvDenseSNN
  gives identical logits from either."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, ops, synthetic as syn
  c = cases.conv_net_case()                    # 16 x 16 input, T = 4, B = 2
  H = W = 16
  T = 4
  model = models.ConvDenseSNN(num_classes=11, config=syn.make_config(bits=c["bits"], prune_percentage=0.9))
  variables = nn.tree_from_numpy(c["vars"], dev)
  rng = np.random.Generator(np.random.PCG64(47))
  streams = {None: [ec.make_sample(rng, n, H, W) for n in (900, 1400)],
             L.EV4: [ec.make_sample(rng, n, H, W) for n in (900, 1400)],
             L.EV1: [ec.make_sample(rng, n, H, W, unique=True) for n in (300, 420)]}
  for fmt, samples in streams.items():
    ev = ec.make_set(samples)
    es = _event_set(ev, (H, W), dev)
    frames = []
    for a, _ in samples:
      x, y, p = (torch.from_numpy(a[:, k].astype(np.int32)).to(dev) for k in range(3))
      frames.append(ops.events_to_frames(x, y, p, T, H, W))
    old = torch.stack(frames, 0)
    limit = {None: 255, L.EV4: 15, L.EV1: 1}[fmt]
    assert 0 < int(old.max()) <= limit
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    new = ops.events_bin(es, [0, 1], T, H, W, mode="number", fmt=fmt, flags=flags[:1])
    if fmt is None:
      assert torch.equal(new, old)
    else:
      packed = ops.pack_frames(old, fmt, flags[1:])
      assert torch.equal(new.data, packed.data) and _np(flags).tolist() == [0, 0]
      old = packed
    logits = []
    for x in (new, old):
      (l, _), _ = model.apply(variables, x, trgt=None, train=False, rng=None, mutable=["intermediates"])
      logits.append(l)
    torch.cuda.synchronize()
    assert torch.equal(logits[0], logits[1]) and bool(torch.isfinite(logits[0]).all())


# ---- the pipeline on an event source ---------------------------------------------------------------

def _source(rng, n, hw, T, labels, start=START, events=260):
  samples = [ec.edge_sample(rng, events + 17 * i, hw, hw, T, start, STEP) for i in range(n)]
  return dict(ec.make_set(samples), label=np.asarray(labels), sensor_size=np.array([hw, hw]))


def test_eval_on_an_event_source_equals_the_frame_source(dev, tmp_path):
  """An event source through create_input_iter(train=False) and evaluate_metrics gives the loss and
  accuracy of the same frames fed as a frame source, in both modes."""
  from snnquantprune_amd import checkpoint, eval as ev_mod
  from snnquantprune_amd import synthetic as syn
  from snnquantprune_amd.train_utils import mse_loss
  c = cases.conv_net_case(B=8)
  rng = np.random.Generator(np.random.PCG64(53))
  labels = rng.integers(0, 11, 8).astype(np.int8)
  state = {"step": np.int32(3), "params": {"params": c["vars"]["params"]}, "batch_stats": c["vars"]["batch_stats"]}
  (tmp_path / "checkpoint_3").write_bytes(checkpoint.msgpack_serialize(state))
  T = 4
  src = _source(rng, 8, 32, T, labels, start=0, events=700)        # 32 x 32 sensor at resolution_scale 2
  src["times"] = src["times"] - src["times"].min()
  off = src["offsets"]

  def config(split_by, fmt):
    cfg = syn.make_config(bits=4, prune_percentage=0.9)
    cfg.model, cfg.feed_format, cfg.split_by = "ConvDenseSNN", fmt, split_by
    cfg.num_frames, cfg.resolution_scale, cfg.time_step, cfg.input_scale = T, 2, 1, 1
    cfg.train_chunk_size = cfg.test_chunk_size = 1000              # longer than the recordings: origin = t_min
    cfg.eval_batch_size, cfg.batch_size, cfg.steps_per_eval = 4, 4, -1
    cfg.loss_fn, cfg.smoothing = mse_loss, 0.0
    return cfg

  for split_by, fmt in (("number", "u8"), ("number", "ev4"), ("time", "u8")):
    frames = np.zeros((8, T, 16, 16, 2), np.int64)
    for i in range(8):
      a, t = src["addrs"][off[i]:off[i + 1]], src["times"][off[i]:off[i + 1]]
      frames[i] = ec.decode_number(a, T, 16, 16, 2.0) if split_by == "number" else \
          ec.decode_time(a, t, int(t.min()), 1000, T, 16, 16, 2.0)
    assert 0 < frames.max() <= 15 and frames.sum() > 0
    cfg = config(split_by, fmt)
    _, got, per_step = ev_mod.evaluate_metrics(cfg, str(tmp_path), source=src, device=dev)
    _, want, per_want = ev_mod.evaluate_metrics(config("number", "u8"), str(tmp_path), device=dev,
                                                source={"dvs_matrix": frames.astype(np.uint8), "label": labels})
    assert got["steps"] == 2 and got["samples"] == 8
    assert got["loss"] == want["loss"] and got["accuracy"] == want["accuracy"]
    assert torch.equal(per_step["loss"], per_want["loss"]) and torch.equal(per_step["accuracy"], per_want["accuracy"])


def test_time_step_times_input_scale_divides_the_counts(dev):
  """time_step * input_scale != 1 (input_pipeline.py:137): float32 batches, counts / float32(product),
  from windows of time_step ms; the eval split draws the same origins every pass."""
  from snnquantprune_amd import input_pipeline as ip
  from snnquantprune_amd import synthetic as syn
  rng = np.random.Generator(np.random.PCG64(61))
  T, hw, n = 3, 8, 4
  samples = [ec.make_sample(rng, 600, hw, hw, t_lo=50 * i, t_hi=50 * i + 9000) for i in range(n)]
  src = dict(ec.make_set(samples), label=np.arange(n), sensor_size=np.array(hw))
  cfg = syn.make_config(bits=4, prune_percentage=0.9)
  cfg.split_by, cfg.num_frames, cfg.resolution_scale, cfg.time_step, cfg.input_scale = "time", T, 1, 2, 1.5
  cfg.train_chunk_size, cfg.test_chunk_size, cfg.batch_size, cfg.eval_batch_size = 1, 1, 2, 2
  cfg.seed, cfg.feed_format = 9, "u8"
  it = ip.create_input_iter(src, cfg, train=False, cache=False, device=dev)
  plan = ip.EventPlan(cfg, src["sensor_size"], n, train=False)
  drawn = plan.batches(np.array([t.min() for _, t in samples]), np.array([t.max() for _, t in samples]))
  first = []
  for i in range(4):                                               # two passes of two batches
    batch = next(it)
    idx, starts = next(drawn)
    want = ec.decode_batch(src, idx, T, hw, hw, "time", starts, 2000)
    assert batch["dvs_matrix"].dtype == torch.float32 and want.sum() > 0 and len(set(starts.tolist())) > 1
    np.testing.assert_array_equal(_np(batch["dvs_matrix"]), want.astype(np.float32) / np.float32(3.0))
    np.testing.assert_array_equal(_np(batch["label"]), idx)
    first.append(batch["dvs_matrix"])
  assert torch.equal(first[0], first[2]) and torch.equal(first[1], first[3])


def test_two_train_steps_from_an_event_source(dev):
  """create_input_iter(train=True) on an 8 x 8 sensor, T = 3: the batches are the restatement's for
  the permutation and the origins the plan draws; two train_steps of the tiny ConvDenseSNN give a
  finite loss and move the parameters."""
  from snnquantprune_amd import input_pipeline as ip
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  from snnquantprune_amd import train_utils as tu
  v, _ = cr.fixture(True)
  cfg = syn.make_config(bits=cr.BITS, prune_percentage=0.9, channels=cr.CHANNELS, tau=cr.TAU, quantized=True,
                        num_conv_blocks=cr.NBLOCKS, dropout=cr.KEEP)
  cfg.optimizer = "adam"
  cfg.split_by, cfg.num_frames, cfg.resolution_scale, cfg.time_step, cfg.input_scale = "time", cr.T_STEPS, 1, 1, 1
  cfg.train_chunk_size, cfg.test_chunk_size, cfg.batch_size, cfg.eval_batch_size = 1, 1, 4, 4
  cfg.seed, cfg.feed_format = 5, "u8"
  model = models.ConvDenseSNN(num_classes=cr.CLASSES, config=cfg)
  variables = nn.tree_from_numpy(v, dev)
  rng = np.random.Generator(np.random.PCG64(59))
  n = 6
  labels = (np.arange(n) % cr.CLASSES).astype(np.int8)
  samples = []
  for i in range(n):                                               # 6 ms recordings: origins have 4 ms to move in
    a, t = ec.make_sample(rng, 500 + 30 * i, cr.HW, cr.HW, t_lo=100 * i, t_hi=100 * i + 6000)
    samples.append((a, t))
  src = dict(ec.make_set(samples), label=labels, sensor_size=np.array(cr.HW))
  it = ip.create_input_iter(src, cfg, train=True, cache=False, device=dev)
  plan = ip.EventPlan(cfg, src["sensor_size"], n, train=True)      # the same seed: the same draws
  t_min = np.array([t.min() for _, t in samples])
  t_max = np.array([t.max() for _, t in samples])
  drawn = plan.batches(t_min, t_max)
  state = tu.create_train_state(variables, cfg, model)
  before = [p.clone() for _, p in tu._flatten(state.params["params"])]
  seen = []
  for step in range(2):
    batch = next(it)
    idx, starts = next(drawn)
    seen.append(starts)
    assert np.all(starts >= t_min[idx]) and np.all(starts <= t_max[idx] - 2000)
    want = ec.decode_batch(src, idx, cr.T_STEPS, cr.HW, cr.HW, "time", starts, 1000)
    assert batch["dvs_matrix"].dtype == torch.uint8 and want.sum() > 0
    np.testing.assert_array_equal(_np(batch["dvs_matrix"]), np.minimum(want, 255).astype(np.uint8))
    np.testing.assert_array_equal(_np(batch["label"]), labels[idx])
    state, m = tu.train_step(state, batch, step, lambda s: 1e-2, 0.0, 0.0, tu.mse_loss)
    assert bool(torch.isfinite(m["loss"]))
  assert len(set(np.concatenate(seen).tolist())) > 1 and state.step == 2
  after = [p for _, p in tu._flatten(state.params["params"])]
  assert any(not torch.equal(a, b) for a, b in zip(after, before))
