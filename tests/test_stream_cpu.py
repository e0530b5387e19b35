"""Streaming inference on the host: that the split property holds in the oracle itself,
that no case of tests/stream_cases.py is vacuous, and models.StreamState on CPU tensors."""
import numpy as np
import pytest
import torch

from tests import stream_cases as sc

F32 = np.float32
RATE_BAND = (0.005, 0.7)        # the band the model and kernel suites hold their rasters to


def _in_band(s):
  return RATE_BAND[0] < float(np.mean(s)) < RATE_BAND[1]


def _vacuity(whole, run, fresh, raster_keys, boundary_of, resets):
  """run: the carried stream, fresh: every window restarted from zero, over one split."""
  for k in raster_keys:
    assert _in_band(whole[k]), (k, float(np.mean(whole[k])))
  for w in range(1, len(run["boundaries"])):
    for k, (a, b) in raster_keys_windows(run, fresh, w).items():
      assert (a != b).any(), "window %d of %s: a restart from zero gives the same spikes" % (w, k)
  for bound in run["boundaries"][:-1]:
    for u, vr in zip(boundary_of(bound), resets):
      assert ((u != 0) & (u != F32(vr))).any()


def raster_keys_windows(run, fresh, w):
  if "windows1" in run:
    return {"s1": (run["windows1"][w], fresh["windows1"][w]), "s2": (run["windows2"][w], fresh["windows2"][w])}
  return {"block%d" % i: (run["windows"][i][w], fresh["windows"][i][w]) for i in range(4)}


# ---------------------------------------------------------------------------
# the split property in the authority, and no vacuous case
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("id", sc.HEAD_IDS)
def test_oracle_head_splits_equal_whole_run(oracle, id):
  """oracle.dense_block window by window with u0 == the whole run: rasters, final membranes, counts,
  vote -- for every split the GPU tests stream."""
  b, whole = sc.head(id), sc.head_whole(oracle, id)
  for split in sc.HEAD_SPLITS:
    run = sc.head_run(oracle, b, split)
    for k in ("s1", "s2", "u1", "u2", "counts", "logits"):
      np.testing.assert_array_equal(run[k], whole[k], err_msg="%s %s %s" % (id, split, k))
  r2 = oracle.dense2_forward(b["x"], sc.qweight_of(oracle, b["leaf1"], 8), sc.qweight_of(oracle, b["leaf2"], 8),
                             b["cfg1"], "int") if (b["case"]["neuron"] != "lif" and b["mode1"] == "int") else None
  if r2 is not None:      # (dense2_forward takes ONE neuron config and ONE mode for both blocks)
    np.testing.assert_array_equal(r2["s2"].astype(np.uint8), whole["s2"])
    np.testing.assert_array_equal(r2["logits"], whole["logits"])


@pytest.mark.parametrize("id", sc.HEAD_IDS)
def test_head_cases_are_not_vacuous(oracle, id):
  b, whole = sc.head(id), sc.head_whole(oracle, id)
  for split in sc.HEAD_SPLITS[1:]:
    _vacuity(whole, sc.head_run(oracle, b, split), sc.head_run(oracle, b, split, carry=False), ("s1", "s2"),
             lambda bound: bound, (b["cfg1"]["v_reset"], b["cfg2"]["v_reset"]))


def test_tie_case_ties_at_an_inner_step(oracle):
  """The streamed tie case has potentials exactly on v_threshold at a step with a window boundary
  directly before it and directly after it, and the oracle's splits there equal its whole run."""
  b, c, r, t = sc.tie_head(oracle)
  assert 1 <= t <= c["T"] - 2
  hb = {"leaf1": b["leaf"], "leaf2": b["leaf2"], "bits": None, "cfg1": b["cfg"], "cfg2": b["cfg2"], "mode1": "int",
        "x": b["x"]}
  from tests import tie_cases as tc
  q1, q2 = tc.qweight(oracle, b["leaf"], c["bits"]), tc.qweight(oracle, b["leaf2"], c["bits2"])
  for split in ([t, c["T"] - t], [t + 1, c["T"] - t - 1]):
    u1 = u2 = None
    s1s, s2s, t0 = [], [], 0
    for tw in split:
      u1, s1 = oracle.dense_block(hb["x"][t0:t0 + tw], q1, b["cfg"], "int", u0=u1)
      u2, s2 = oracle.dense_block(s1, q2, b["cfg2"], "int", u0=u2)
      s1s.append(s1); s2s.append(s2); t0 += tw
    np.testing.assert_array_equal(np.concatenate(s1s).astype(np.uint8), r["s"])
    np.testing.assert_array_equal(np.concatenate(s2s).astype(np.uint8), r["second"]["s"])
    np.testing.assert_array_equal(u1, r["u"])


@pytest.mark.parametrize("hidden", [160, 96])
def test_oracle_dense_model_splits(oracle, hidden):
  from tests import cases
  c = sc.dense_model(hidden)
  whole = sc.dense_model_run(oracle, c, [sc.MODEL_T])
  e = cases.dense_net_expected(oracle, c)                 # oracle.dense2_forward
  np.testing.assert_array_equal(whole["s2"], e["s2"])
  np.testing.assert_array_equal(whole["logits"], e["logits"])
  for split in sc.MODEL_SPLITS:
    run = sc.dense_model_run(oracle, c, split)
    for k in ("s1", "s2", "u1", "u2", "counts", "logits"):
      np.testing.assert_array_equal(run[k], whole[k], err_msg="%s %s" % (split, k))
  for split in sc.MODEL_SPLITS[1:]:
    _vacuity(whole, sc.dense_model_run(oracle, c, split), sc.dense_model_run(oracle, c, split, carry=False),
             ("s1", "s2"), lambda bound: bound, (0.0, 0.0))


@pytest.mark.parametrize("counts", [False, True])
def test_oracle_conv_model_splits(oracle, counts):
  from tests import cases
  c = sc.conv_model(counts)
  whole = sc.conv_model_whole(oracle, counts)
  e = cases.conv_net_expected(oracle, c)                  # oracle.conv3_dense_forward
  np.testing.assert_array_equal(whole["dense_s"], e["dense_s"])
  np.testing.assert_array_equal(whole["logits"], e["logits"])
  for split in sc.MODEL_SPLITS:
    run = sc.conv_model_run(oracle, c, split)
    for k in ("pool0", "pool1", "pool2", "dense_s", "counts", "logits"):
      np.testing.assert_array_equal(run[k], whole[k], err_msg="%s %s" % (split, k))
    for a, b in zip(run["u"], whole["u"]):
      np.testing.assert_array_equal(a, b)
  for split in sc.MODEL_SPLITS[1:]:
    _vacuity(whole, sc.conv_model_run(oracle, c, split), sc.conv_model_run(oracle, c, split, carry=False),
             ("pool0", "pool1", "pool2", "dense_s"), lambda bound: bound, (0.0,) * 4)


# ---------------------------------------------------------------------------
# models.StreamState on CPU tensors
# ---------------------------------------------------------------------------


def _state(B=3, N1=12, N2=20):
  from snnquantprune_amd import models
  return models.StreamState.zeros([(B, N1), (B, N2)], N2, "cpu")


@pytest.mark.parametrize("steps", [3, 7, 20])
def test_state_logits_equal_the_oracle_vote(oracle, steps):
  """counts / steps with an inexact 1 / steps, then the in-order group mean: the bits of oracle.vote
  of the concatenated raster, whatever windows the counts arrived in."""
  B, N = 5, 110
  raster = (np.random.Generator(np.random.PCG64(steps)).random((steps, B, N)) < 0.3).astype(np.uint8)
  from snnquantprune_amd import models
  st = models.StreamState.zeros([(B, 4), (B, N)], N, "cpu")
  t0 = 0
  for tw in [1, steps - 2, 1]:
    st.counts += torch.from_numpy(raster[t0:t0 + tw].astype(np.int32).sum(0).astype(np.int32))
    st.advance(tw)
    t0 += tw
  assert st.steps == steps and st.row_steps.tolist() == [steps] * B
  np.testing.assert_array_equal(st.logits(10).numpy(), oracle.vote(raster, 10))
  np.testing.assert_array_equal(st.logits(5).numpy(), oracle.vote(raster, 5))
  with pytest.raises(ValueError):
    st.logits(7)


def test_state_is_sized_once_and_typed():
  st = _state()
  assert [tuple(u.shape) for u in st.membranes] == [(3, 12), (3, 20)]
  assert all(u.dtype == torch.float32 and not u.any() for u in st.membranes)
  assert st.counts.dtype == torch.int32 and tuple(st.counts.shape) == (3, 20) and not st.counts.any()
  assert st.row_steps.dtype == torch.int32 and tuple(st.row_steps.shape) == (3,) and st.steps == 0
  ptrs = [t.data_ptr() for t in st._tensors()]
  st._fit([(3, 12), (3, 20)], 20, "cpu")                   # the same blocks again: nothing moves
  assert [t.data_ptr() for t in st._tensors()] == ptrs
  from snnquantprune_amd import models
  empty = models.StreamState()
  assert empty.membranes == [] and empty.counts is None and empty.steps == 0
  with pytest.raises(ValueError):
    empty.logits()


def test_state_refuses_what_does_not_fit():
  st = _state()
  with pytest.raises(ValueError, match="batch rows"):
    st._fit([(4, 12), (4, 20)], 20, "cpu")
  with pytest.raises(ValueError, match="sized for"):
    st._fit([(3, 16), (3, 20)], 20, "cpu")
  with pytest.raises(ValueError, match="sized for"):
    st._fit([(3, 12), (3, 20), (3, 20)], 20, "cpu")


def test_state_reset_rows_and_clone():
  st = _state()
  for u in st.membranes:
    u += 0.25
  st.counts += 3
  st.advance(4)
  snap = st.clone()
  st.reset(rows=[1])
  for u, v in zip(st.membranes, snap.membranes):
    assert not u[1].any() and torch.equal(u[0], v[0]) and torch.equal(u[2], v[2])
  assert st.counts[1].tolist() == [0] * 20 and st.counts[0].tolist() == [3] * 20
  assert st.row_steps.tolist() == [4, 0, 4] and st.steps == 4
  # the snapshot holds tensors of its own
  assert snap.row_steps.tolist() == [4, 4, 4] and snap.counts[1].tolist() == [3] * 20 and snap.steps == 4
  assert all(a.data_ptr() != b.data_ptr() for a, b in zip(st._tensors(), snap._tensors()))
  # a row that has seen no step votes 0; the others vote counts / steps
  lg = st.logits(10)
  assert lg[1].tolist() == [0.0, 0.0] and lg[0].tolist() == [0.75, 0.75]
  with pytest.raises(ValueError):
    st.reset(rows=[3])
  st.reset()
  assert st.steps == 0 and not any(t.any() for t in st._tensors())


def test_model_refusals_that_need_no_gpu():
  """CextNet with a state, probes with a state, something that is no StreamState; train=True with
  a carried state stays refused as before."""
  from snnquantprune_amd import linen as nn
  from snnquantprune_amd import models, synthetic as syn
  st = models.StreamState()
  x = torch.zeros((2, 3, 32), dtype=torch.uint8)
  cfg = syn.make_config(bits=8, prune_percentage=0.5, hidden=160)
  with pytest.raises(NotImplementedError, match="TCJA"):
    models.CextNet(num_classes=11, config=syn.make_config()).apply({"params": {}}, x, u_state=st)
  with pytest.raises(TypeError):
    models.DenseSNN(num_classes=11, config=cfg).apply({"params": {}}, x, u_state=object())
  probing = syn.make_config(bits=8, prune_percentage=0.5, hidden=160, density_probes=True)
  for model in (models.DenseSNN(num_classes=11, config=probing), models.ConvDenseSNN(num_classes=11, config=probing)):
    with pytest.raises(NotImplementedError, match="probes"):
      model.apply({"params": {}}, x, u_state=st, mutable=["intermediates"])
  assert st.counts is None                                # no refusal touched the state
