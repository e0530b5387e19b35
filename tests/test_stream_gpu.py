"""Streaming inference on the GPU, everything bit for bit: for any split of T into
windows the concatenated rasters, the final membranes and the vote over all steps equal the single
whole-run call -- the oracle's, and the `u_state=None` call of the fused / compacted paths."""
import ctypes

import numpy as np
import pytest
import torch

from tests import stream_cases as sc
from tests.helpers import pack_ev1, pack_ev4, packbits_lastaxis

pytestmark = pytest.mark.gpu
F32 = np.float32
eq = np.testing.assert_array_equal


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()                      # fails loudly if the HIP extension is missing
  return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def clean_device_status():
  yield
  from snnquantprune_amd import ops
  assert ops.device_status() == 0


def _t(a, dev):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(x):
  from snnquantprune_amd import ops
  if isinstance(x, ops.PackedSpikes):
    return x.bits.cpu().numpy().view(np.uint32)
  return x.cpu().numpy()


def _raster(x):
  """A sown raster as uint8 0 / 1, whatever format the block wrote it in."""
  from snnquantprune_amd import ops
  d = x.to_dense() if isinstance(x, ops.PackedSpikes) else x
  return d.cpu().numpy().astype(np.uint8)


def _packed_kernel(leaf, bits, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import packing
  from snnquantprune_amd.quant import QuantDesc
  a, c = float(leaf["DuQ_0"]["a"][0]), float(leaf["DuQ_0"]["c"][0])
  desc = QuantDesc(L.Q_DUQ, bits, a, c, float(2 ** (bits - 1) - 1), c)
  mask = leaf.get("prune_0", {}).get("mask")
  return packing.PackedKernel(_t(leaf["kernel"], dev), desc, None if mask is None else _t(mask, dev))


def _neuron(oracle, cfg, dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  vth, vr = cfg["v_threshold"], cfg["v_reset"]
  if cfg["kind"] == "multi_step_LIF":
    return ops.Neuron(L.NEURON_MULTI_STEP_LIF, cfg["tau"], vth, vr)
  if cfg["kind"] == "parametric_leaky_IF":
    return ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, float(oracle.sigmoid_f32(cfg["tau_param"])), vth, vr)
  return ops.Neuron(L.NEURON_LIF, 1.0, vth, vr, decay=_t(oracle.sigmoid_f32(cfg["tau_vec"]), dev))


class _Head:
  """The device side of a head case: weights, neurons, the windows of x in the case's row format."""

  def __init__(self, oracle, dev, leaf1, bits1, leaf2, bits2, cfg1, cfg2, x, rows):
    from snnquantprune_amd import ops
    self.dev, self.rows = dev, rows
    self.K, self.N1, self.N2 = leaf1["kernel"].shape[0], leaf1["kernel"].shape[1], leaf2["kernel"].shape[1]
    pk1, pk2 = _packed_kernel(leaf1, bits1, dev), _packed_kernel(leaf2, bits2, dev)
    self.w1 = pk1.int_weight_mfma((self.N1 + 31) // 32 * 32)
    self.w2 = pk2.int_weight_mfma((self.N2 + 31) // 32 * 32)
    self.n1, self.n2 = _neuron(oracle, cfg1, dev), _neuron(oracle, cfg2, dev)
    self.fb = (lambda: ops.FloatFallback(pk1.float_weight())) if rows in ("f32", "f32frac") else (lambda: None)
    self.x = x
    self.B = x.shape[1]

  def window(self, t0, tw):
    from snnquantprune_amd import ops
    xw = _t(self.x[t0:t0 + tw], self.dev)
    return ops.pack_bits(xw) if self.rows == "bits" else xw

  def state(self):
    from snnquantprune_amd import models
    return models.StreamState.zeros([(self.B, self.N1), (self.B, self.N2)], self.N2, self.dev)

  def stream(self, split, workspace=True):
    """The one-launch head window by window -> (state, hidden words, output words, window logits)."""
    from snnquantprune_amd import ops
    st = self.state()
    s1s, s2s, wl, t0 = [], [], [], 0
    for tw in split:
      lg, s1, s2, u1, u2 = ops.dense_head_forward_state(
          self.window(t0, tw), self.w1, self.K, self.N1, self.n1, self.w2, self.N2, self.n2,
          st.membranes[0], st.membranes[1], st.counts, group=10, want_s1=True, want_s2=True,
          fallback=self.fb(), workspace=workspace)
      st.membranes[0], st.membranes[1] = u1, u2
      st.advance(tw)
      s1s.append(_np(s1)); s2s.append(_np(s2)); wl.append(_np(lg))
      t0 += tw
    return st, np.concatenate(s1s), np.concatenate(s2s), wl

  def per_block(self, split):
    """What a streaming caller had before: two dense_lif_forward calls with their carries, a vote."""
    from snnquantprune_amd import ops
    st = self.state()
    s1s, s2s, wl, t0 = [], [], [], 0
    for tw in split:
      u1, s1 = ops.dense_lif_forward(self.window(t0, tw), self.w1, self.K, self.N1, self.n1, u0=st.membranes[0],
                                     want_u=True, packed_out=True, fallback=self.fb())
      u2, s2 = ops.dense_lif_forward(s1, self.w2, self.N1, self.N2, self.n2, u0=st.membranes[1], want_u=True,
                                     packed_out=True)
      st.membranes[0], st.membranes[1] = u1, u2
      ops.vote_accumulate(s2, st.counts)
      st.advance(tw)
      s1s.append(_np(s1)); s2s.append(_np(s2)); wl.append(_np(ops.vote(s2, 10)))
      t0 += tw
    return st, np.concatenate(s1s), np.concatenate(s2s), wl


def _check_stream(got, want, what):
  """got: (state, s1 words, s2 words, window logits); want: a dict of stream_cases.head_run."""
  st, s1, s2, wl = got
  eq(s1, packbits_lastaxis(want["s1"]), err_msg=what + " hidden raster")
  eq(s2, packbits_lastaxis(want["s2"]), err_msg=what + " output raster")
  eq(_np(st.membranes[0]), want["u1"], err_msg=what + " u1")
  eq(_np(st.membranes[1]), want["u2"], err_msg=what + " u2")
  eq(_np(st.counts), want["counts"], err_msg=what + " counts")
  assert len(wl) == len(want["window_logits"])
  for i, (a, b) in enumerate(zip(wl, want["window_logits"])):
    eq(a, b, err_msg="%s logits of window %d" % (what, i))
  eq(_np(st.logits(10)), want["logits"], err_msg=what + " state.logits()")
  assert st.steps == want["s2"].shape[0]


# ---------------------------------------------------------------------------
# the head kernel alone
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("workspace", [True, False], ids=["ws", "no_ws"])
@pytest.mark.parametrize("id", sc.HEAD_IDS)
def test_head_state_kernel_streams(dev, oracle, id, workspace):
  """snnqp_dense_head_forward_state over every split: rasters, u1, u2, counts, every window's logits
  and state.logits() equal the oracle's whole run, with the hand-over workspace (N1 = 512: the
  column split) and without it."""
  b = sc.head(id)
  c = b["case"]
  h = _Head(oracle, dev, b["leaf1"], 8, b["leaf2"], 8, b["cfg1"], b["cfg2"], b["x"], c["rows"])
  whole = sc.head_whole(oracle, id)
  if workspace and c["N1"] > 256:
    from snnquantprune_amd import ops
    assert ops.dense_wide_plan(sc.HEAD_T, c["B"], c["N1"], fused=True, may_split=True)[3] == 1   # csplit is served
  for split in sc.HEAD_SPLITS:
    want = dict(whole, window_logits=sc.head_run(oracle, b, split)["window_logits"])
    _check_stream(h.stream(split, workspace), want, "%s %s" % (id, split))


@pytest.mark.parametrize("id", sc.HEAD_IDS)
def test_head_state_kernel_equals_per_block_path(dev, oracle, id):
  """... and the two-launch-plus-vote path a streaming caller had before (snnqp_dense_lif_forward with
  u0 / u_out per block, the counting vote), which in turn equals the oracle."""
  b = sc.head(id)
  h = _Head(oracle, dev, b["leaf1"], 8, b["leaf2"], 8, b["cfg1"], b["cfg2"], b["x"], b["case"]["rows"])
  whole = sc.head_whole(oracle, id)
  for split in ([sc.HEAD_T], [7, 13], [3, 1, 16]):
    pb = h.per_block(split)
    _check_stream(pb, dict(whole, window_logits=sc.head_run(oracle, b, split)["window_logits"]),
                  "%s %s per block" % (id, split))
    got = h.stream(split)
    eq(got[1], pb[1]); eq(got[2], pb[2])
    for a, bb in zip(got[0]._tensors(), pb[0]._tensors()):
      eq(_np(a), _np(bb))


def test_head_state_kernel_at_ties(dev, oracle):
  """Potentials exactly on v_threshold, with a window boundary directly before the tie step and
  directly after it: the carried potential, not a recomputed one, decides the spike."""
  b, c, r, t = sc.tie_head(oracle)
  h = _Head(oracle, dev, b["leaf"], c["bits"], b["leaf2"], c["bits2"], b["cfg"], b["cfg2"], b["x"], c["rows"])
  for split in ([t, c["T"] - t], [t + 1, c["T"] - t - 1], [c["T"]]):
    st, s1, s2, _ = h.stream(split)
    eq(s1, packbits_lastaxis(r["s"]), err_msg=str(split))
    eq(s2, packbits_lastaxis(r["second"]["s"]), err_msg=str(split))
    eq(_np(st.membranes[0]), r["u"])
    eq(_np(st.membranes[1]), r["second"]["u"])
    eq(_np(st.logits(10)), r["logits"])


# ---------------------------------------------------------------------------
# the counting vote
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("packed", [True, False], ids=["bits", "f32"])
@pytest.mark.parametrize("N,group", [(110, 10), (33, 11)])
def test_vote_accumulate_and_counts(dev, oracle, N, group, packed):
  from snnquantprune_amd import ops
  B = 5
  raster = (np.random.Generator(np.random.PCG64(N)).random((7, B, N)) < 0.3).astype(np.uint8)
  counts = torch.full((B, N), 2, dtype=torch.int32, device=dev)       # counts are ADDED to what is there
  t0 = 0
  for tw in (1, 2, 4):
    w = _t(raster[t0:t0 + tw], dev)
    assert ops.vote_accumulate(ops.pack_bits(w) if packed else w.to(torch.float32), counts) is counts
    t0 += tw
    eq(_np(counts), 2 + raster[:t0].astype(np.int32).sum(0))
  counts -= 2
  whole = _t(raster, dev)
  want = _np(ops.vote(ops.pack_bits(whole) if packed else whole.to(torch.float32), group))
  eq(want, oracle.vote(raster, group))
  eq(_np(ops.vote_counts(counts, 7, group)), want)
  # every row its own number of steps: row 1 has seen the last four steps only, row 2 none
  steps = torch.tensor([7, 4, 0, 7, 7], dtype=torch.int32, device=dev)
  counts[1] = _t(raster[3:, 1].astype(np.int32).sum(0).astype(np.int32), dev)
  counts[2] = 0
  got = _np(ops.vote_counts(counts, steps, group))
  eq(got[[0, 3, 4]], want[[0, 3, 4]])
  eq(got[1], oracle.vote(raster[3:, 1:2], group)[0])
  eq(got[2], np.zeros(N // group, F32))
  with pytest.raises(ValueError):
    ops.vote_counts(counts, 7, 7)
  with pytest.raises(ValueError):
    ops.vote_accumulate(whole.to(torch.float32), counts[:, :N - 1].contiguous())


# ---------------------------------------------------------------------------
# the models through apply
# ---------------------------------------------------------------------------


def _dense_snn(hidden, dev, c):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  model = models.DenseSNN(num_classes=11, config=syn.make_config(bits=8, prune_percentage=0.5, hidden=hidden))
  return model, nn.tree_from_numpy(c["vars"], dev)


def _conv_snn(dev, c):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  model = models.ConvDenseSNN(num_classes=11, config=syn.make_config(bits=c["bits"], prune_percentage=0.9))
  return model, nn.tree_from_numpy(c["vars"], dev)


def _model_input(x, fmt, dev):
  """x uint8 [B, Tw, ...] in one of the formats the eval path takes."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  if fmt == "u8":
    return _t(x, dev)
  if fmt == "f32":
    return _t(x.astype(F32), dev)
  if fmt == "bits":
    return ops.pack_bits(_t(x, dev))
  H, W = x.shape[2], x.shape[3]
  if fmt == "ev1":
    return ops.PackedFrames(_t(pack_ev1(x).view(np.int32), dev), H, W, L.EV1)
  return ops.PackedFrames(_t(pack_ev4(x), dev), H, W, L.EV4)


def _apply(model, variables, x, state=None, sown=False):
  kw = dict(trgt=None, train=False, rng=None, u_state=state)
  if sown:
    (lg, st), mut = model.apply(variables, x, mutable=["intermediates"], **kw)
    return lg, st, {k: v[0] for k, v in mut["intermediates"].items()}
  lg, st = model.apply(variables, x, **kw)
  return lg, st, {}


def _stream_model(model, variables, x, fmt, split, dev, names, sown=True):
  """-> (state, {name: concatenated sown raster, dense}, window logits)."""
  from snnquantprune_amd import models
  state = models.StreamState()
  rasters = {n: [] for n in names}
  wl = []
  for xw in sc.windows(x, split, 1):
    lg, st, got = _apply(model, variables, _model_input(xw, fmt, dev), state, sown)
    assert st is state
    wl.append(_np(lg))
    for n in names if sown else ():
      rasters[n].append(_raster(got[n]))
  return state, {n: np.concatenate(v) for n, v in rasters.items() if v}, wl


@pytest.mark.parametrize("fmt", ["u8", "f32"])
@pytest.mark.parametrize("hidden", [160, 96], ids=["one_launch", "block_by_block"])
def test_dense_snn_streams(dev, oracle, hidden, fmt):
  """DenseSNN with u_state over [6], [1, 2, 3], [2, 2, 2]: sown rasters, membranes, counts, every
  window's logits and state.logits() equal the oracle and the u_state=None whole-run call, which
  gives the same bits before and after the streaming sessions."""
  from tests import cases
  c = sc.dense_model(hidden)
  e = cases.dense_net_expected(oracle, c)
  model, variables = _dense_snn(hidden, dev, c)
  whole_x = _model_input(c["x"], fmt, dev)
  lg0, none, _ = _apply(model, variables, whole_x)
  assert none is None
  eq(_np(lg0), e["logits"])
  want = sc.dense_model_run(oracle, c, [sc.MODEL_T])
  for split in sc.MODEL_SPLITS:
    wl_want = sc.dense_model_run(oracle, c, split)["window_logits"]
    for sown in (True, False, False):          # (unsown twice: the prepared head plan, then its cache)
      st, r, wl = _stream_model(model, variables, c["x"], fmt, split, dev, ("dense1_out", "dense2_out"), sown)
      if sown:
        eq(r["dense1_out"], want["s1"]); eq(r["dense2_out"], want["s2"])
      for a, b in zip(wl, wl_want):
        eq(a, b)
      eq(_np(st.membranes[0]), want["u1"]); eq(_np(st.membranes[1]), want["u2"])
      eq(_np(st.counts), want["counts"])
      eq(_np(st.logits(10)), e["logits"])
      assert st.steps == sc.MODEL_T and st.row_steps.tolist() == [sc.MODEL_T] * sc.MODEL_B
  lg1, none, _ = _apply(model, variables, whole_x)
  assert none is None
  eq(_np(lg1), e["logits"])


def test_dense_snn_state_keeps_its_tensors(dev):
  """Integer-typed windows update the state's tensors in place: their addresses are what a captured
  window was recorded with."""
  for hidden in (160, 96):
    c = sc.dense_model(hidden)
    model, variables = _dense_snn(hidden, dev, c)
    from snnquantprune_amd import models
    state = models.StreamState()
    ptrs = None
    for xw in sc.windows(c["x"], [2, 2, 2], 1):
      _apply(model, variables, _t(xw, dev), state)
      now = [t.data_ptr() for t in state._tensors()]
      assert ptrs is None or now == ptrs
      ptrs = now
    before = state.clone()
    lg, st, _ = _apply(model, variables, _t(c["x"][:, :0], dev), state)      # Tw == 0: untouched
    assert st is state and tuple(lg.shape) == (sc.MODEL_B, 11) and state.steps == sc.MODEL_T
    for a, b in zip(state._tensors(), before._tensors()):
      eq(_np(a), _np(b))


@pytest.mark.parametrize("fmt", ["u8", "ev1", "ev4", "f32"])
def test_conv_dense_snn_streams(dev, oracle, fmt):
  """ConvDenseSNN with u_state (uncompacted, every block carrying its membranes) against the oracle
  and the compacted u_state=None whole-run call."""
  from tests import cases
  counts = fmt == "ev4"
  c = sc.conv_model(counts)
  e = cases.conv_net_expected(oracle, c)
  want = sc.conv_model_whole(oracle, counts)
  model, variables = _conv_snn(dev, c)
  whole_x = _model_input(c["x"], fmt, dev)
  lg0, none, sown0 = _apply(model, variables, whole_x, sown=True)
  assert none is None
  eq(_np(lg0), e["logits"])
  eq(_raster(sown0["dense_out"]), e["dense_s"])
  names = ("pool0", "pool1", "pool2", "dense_out")
  for split in sc.MODEL_SPLITS:
    st, r, wl = _stream_model(model, variables, c["x"], fmt, split, dev, names)
    for i in range(3):
      eq(r["pool%d" % i], want["pool%d" % i], err_msg="%s pool%d" % (split, i))
    eq(r["dense_out"], want["dense_s"])
    for a, b in zip(wl, sc.conv_model_run(oracle, c, split)["window_logits"]):
      eq(a, b)
    assert len(st.membranes) == 4
    for a, b in zip(st.membranes, want["u"]):
      eq(_np(a), b)
    eq(_np(st.counts), want["counts"])
    eq(_np(st.logits(10)), e["logits"])
  lg1, none, _ = _apply(model, variables, whole_x)
  assert none is None
  eq(_np(lg1), e["logits"])


@pytest.mark.parametrize("hidden", [160, 96], ids=["one_launch", "block_by_block"])
def test_reset_rows_mid_stream(dev, oracle, hidden):
  """reset(rows=[1]) after the first window: row 1 goes on as a fresh stream of the remaining steps
  would, rows 0 and 2 as if nothing had happened."""
  from snnquantprune_amd import models
  c = sc.dense_model(hidden)
  model, variables = _dense_snn(hidden, dev, c)
  want = sc.dense_model_run(oracle, c, [sc.MODEL_T])
  fresh = sc.dense_model_run(oracle, dict(c, x=c["x"][1:2, 2:]), [sc.MODEL_T - 2])
  state = models.StreamState()
  for i, xw in enumerate(sc.windows(c["x"], [2, 1, 3], 1)):
    _apply(model, variables, _t(xw, dev), state)
    if i == 0:
      state.reset(rows=[1])
  assert state.row_steps.tolist() == [6, 4, 6]
  lg = _np(state.logits(10))
  eq(lg[[0, 2]], want["logits"][[0, 2]])
  eq(lg[1], fresh["logits"][0])
  for u, w, f in zip(state.membranes, (want["u1"], want["u2"]), (fresh["u1"], fresh["u2"])):
    eq(_np(u)[[0, 2]], w[[0, 2]])
    eq(_np(u)[1], f[0])
  eq(_np(state.counts)[1], fresh["counts"][0])
  eq(_np(state.counts)[[0, 2]], want["counts"][[0, 2]])


# ---------------------------------------------------------------------------
# replay
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("which", ["dense_one_launch", "dense_block_by_block", "conv_ev1"])
def test_captured_window_replays(dev, oracle, which):
  """nn.capture(..., u_state=state) records one window; three replays equal three eager windows, and
  recording leaves the state as it was."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models
  if which == "conv_ev1":
    c = sc.conv_model(False)
    model, variables = _conv_snn(dev, c)
    fmt = "ev1"
  else:
    hidden = 160 if which == "dense_one_launch" else 96
    c = sc.dense_model(hidden)
    model, variables = _dense_snn(hidden, dev, c)
    fmt = "u8"
  wins = [_model_input(xw, fmt, dev) for xw in sc.windows(c["x"], [2, 2, 2], 1)]
  eager = models.StreamState()
  eager_logits = [_np(_apply(model, variables, w, eager)[0]) for w in wins]
  state = models.StreamState()
  step = nn.capture(model, variables, wins[0], trgt=None, train=False, rng=None, u_state=state)
  assert state.steps == 0 and not any(bool(t.any()) for t in state._tensors())
  for w, want in zip(wins, eager_logits):
    lg, st = step(w)
    assert st is state
    eq(_np(lg), want)
  torch.cuda.synchronize()
  assert state.steps == sc.MODEL_T
  for a, b in zip(state._tensors(), eager._tensors()):
    eq(_np(a), _np(b))
  eq(_np(state.logits(10)), _np(eager.logits(10)))
  step.close()


def test_capture_refuses_float32_windows(dev):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models
  c = sc.dense_model(160)
  model, variables = _dense_snn(160, dev, c)
  with pytest.raises(NotImplementedError, match="integer-typed"):
    nn.capture(model, variables, _t(c["x"][:, :2].astype(F32), dev), trgt=None, train=False, rng=None,
               u_state=models.StreamState())


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------


def test_model_refusals(dev):
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  c = sc.dense_model(160)
  model, variables = _dense_snn(160, dev, c)
  x = _t(c["x"], dev)
  state = models.StreamState()
  _apply(model, variables, x[:, :2].contiguous(), state)
  with pytest.raises(ValueError, match="batch rows"):           # a state of another batch size
    _apply(model, variables, x[:2, :2].contiguous(), state)
  other, other_vars = _dense_snn(96, dev, sc.dense_model(96))   # ... of another model
  with pytest.raises(ValueError, match="sized for"):
    _apply(other, other_vars, x[:, :2].contiguous(), state)
  assert state.steps == 2
  probing = models.DenseSNN(num_classes=11, config=syn.make_config(bits=8, prune_percentage=0.5, hidden=160,
                                                                   density_probes=True))
  with pytest.raises(NotImplementedError, match="probes"):
    probing.apply(variables, x, trgt=None, train=False, rng=None, u_state=models.StreamState(),
                  mutable=["intermediates"])
  cc = sc.conv_model(False)
  cext = models.CextNet(num_classes=11, config=syn.make_config(bits=4, prune_percentage=0.9))
  with pytest.raises(NotImplementedError, match="TCJA"):
    cext.apply(nn.tree_from_numpy(cc["vars"], dev), _t(cc["x"], dev), trgt=None, train=False, rng=None,
               u_state=models.StreamState())


def test_head_state_entry_refusals(dev, oracle):
  """snnqp_dense_head_forward_state with a null u1 / u2 / counts (EINVAL), and with the shapes the
  stateless entry refuses (EUNSUPPORTED, nothing enqueued: the state stays as it was)."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  b = sc.head("n160_o20_b3_u8_tau2")
  h = _Head(oracle, dev, b["leaf1"], 8, b["leaf2"], 8, b["cfg1"], b["cfg2"], b["x"], "u8")
  st = h.state()
  for u in st.membranes:
    u.fill_(0.25)
  T, B = 4, h.B
  x = h.window(0, T)
  logits = torch.empty((B, h.N2 // 10), dtype=torch.float32, device=dev)

  def call(u1, u2, counts, T=T, N1=h.N1, N2=h.N2, group=10):
    a, bb, n1, n2 = h.w1.struct(), h.w2.struct(), h.n1.struct(), h.n2.struct()
    return L.lib().snnqp_dense_head_forward_state(
        ops._ptr(x), L.U8, B * h.K, h.K, T, B, h.K, N1, ctypes.byref(a), ops._ptr(h.w1.wt), ctypes.byref(n1),
        N2, ctypes.byref(bb), ops._ptr(h.w2.wt), ctypes.byref(n2), group, ops._ptr(u1), ops._ptr(u2),
        ops._ptr(counts), None, None, ops._ptr(logits), None, None, 0, ops._stream())

  u1, u2, counts = st.membranes[0], st.membranes[1], st.counts
  assert call(None, u2, counts) == L.EINVAL
  assert call(u1, None, counts) == L.EINVAL
  assert call(u1, u2, None) == L.EINVAL
  assert call(u1, u2, counts, N2=200) == L.EUNSUPPORTED          # more than 128 output features
  assert call(u1, u2, counts, N1=600) == L.EUNSUPPORTED          # more than 512 hidden features
  assert call(u1, u2, counts, T=65) == L.EUNSUPPORTED            # more than 64 time steps
  assert call(u1, u2, counts, T=0) == L.EUNSUPPORTED             # no time step
  assert call(u1, u2, counts, group=3) == L.EINVAL               # N2 not divisible by the group
  torch.cuda.synchronize()
  assert bool((u1 == 0.25).all()) and bool((u2 == 0.25).all()) and not bool(counts.any())
  assert call(u1, u2, counts) == L.OK
  torch.cuda.synchronize()
  assert bool(counts.any()) and not bool((u1 == 0.25).all())
  with pytest.raises(ValueError):                                 # the Python surface checks the state's shapes
    ops.dense_head_forward_state(x, h.w1, h.K, h.N1, h.n1, h.w2, h.N2, h.n2, u1, u2[:, :10].contiguous(), counts)
  with pytest.raises(ValueError, match="rows"):
    ops.dense_head_forward_state(x, h.w1, h.K, h.N1, h.n1, h.w2, h.N2, h.n2, u1[:2].contiguous(),
                                 u2[:2].contiguous(), counts[:2].contiguous())
