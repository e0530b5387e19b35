"""Gradual magnitude pruning, host side: the properties of the selection rule's NumPy
reference, its agreement with the one-shot host functions where those are defined (no ties), the
CPU path of ops.magnitude_prune on every case, the cubic schedule, prune_event on CPU tensors, and
what is refused before any launch (the config's refusals and the C ABI's)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import prune_select_cases as pc

CASES = pc.cases()


def test_case_table_covers_what_it_says():
  names = {c[0].split("-n")[0] for c in CASES}
  assert {"normal", "normal-some", "normal-all", "equal", "equal-some", "low10", "top11", "mid11", "zeros-denormals",
          "straddle", "straddle-some", "nonfinite", "drift", "layers"} <= names
  assert {c[1].size for c in CASES} >= set(pc.SIZES) | {sum(pc.LAYERS)}
  for n in pc.SIZES:
    ks = {c[3] for c in CASES if c[1].size == n and c[0].startswith("normal-some")}
    m = next(int((~pc.unpruned(c[2])).sum()) for c in CASES if c[1].size == n and c[0].startswith("normal-some"))
    assert ks >= {k for k in (0, 1, m, m + 1, n - 1, n) if 0 <= k <= n}, (n, ks)


def test_reference_properties():
  for name, w, mask, k in CASES:
    got = pc.reference_prune(w, mask, k)
    live0, live1 = pc.unpruned(mask), pc.unpruned(got)
    m = int((~live0).sum())
    assert int((~live1).sum()) == max(k, m), name                   # exactly max(k, m) zeros
    assert not (live1 & ~live0).any(), name                         # old zeros kept
    np.testing.assert_array_equal(pc.as_i32(got)[live1], pc.as_i32(mask)[live1], err_msg=name)   # the rest bitwise
    np.testing.assert_array_equal(pc.as_i32(got)[~live0], pc.as_i32(mask)[~live0], err_msg=name)   # (a -0.0 stays -0.0)
    new = live0 & ~live1
    assert (pc.as_i32(got)[new] == 0).all(), name                   # +0.0 is what is written
    key = pc.keys(w)
    if new.any() and live1.any():
      assert key[new].max() <= key[live1].min(), name               # every pruned key <= every kept key
      # ties at the cut: the lower indices go
      cut = key[new].max()
      tie_new, tie_kept = np.flatnonzero(new & (key == cut)), np.flatnonzero(live1 & (key == cut))
      if tie_kept.size:
        assert tie_new.max() < tie_kept.min(), name
    if k <= m:
      np.testing.assert_array_equal(pc.as_i32(got), pc.as_i32(mask), err_msg=name)


def test_key_order():
  f = lambda *v: pc.keys(np.array(v, np.float32))                   # noqa: E731
  z, d, one, inf, nan = f(-0.0, 0.0), f(1e-45, -3e-45), f(1.0, -1.0), f(np.inf, -np.inf), f(np.nan, -np.nan)
  assert z[0] == z[1] == 0 and one[0] == one[1] and inf[0] == inf[1]
  assert z[0] < d[0] < d[1] < f(1.1754944e-38)[0] < one[0] < f(3.4e38)[0] < inf[0] < nan.min()


def _distinct_tree(seed):
  """Three layers whose magnitudes are all distinct, asserted."""
  rng = np.random.Generator(np.random.PCG64(seed))
  shapes = ((3, 3, 2, 4), (7,), (20, 11))
  total = sum(int(np.prod(s)) for s in shapes)
  mags = (rng.permutation(total) + 1).astype(np.float32) / np.float32(64)
  mags *= np.where(rng.random(total) < 0.5, -1, 1).astype(np.float32)
  assert np.unique(np.abs(mags)).size == total                      # no ties: argpartition's choice is the rule's
  tree, off = {}, 0
  for i, s in enumerate(shapes):
    n = int(np.prod(s))
    tree["QuantConv_%d" % i] = {"kernel": torch.from_numpy(mags[off:off + n].reshape(s).copy())}
    off += n
  return {"block": tree, "BatchNorm_0": {"scale": torch.ones(3)}}


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9, 0.975, 1.0])
def test_reference_agrees_with_the_host_functions_without_ties(p):
  from snnquantprune_amd import prune_utils as pu
  tree = _distinct_tree(11)
  layers = pu._layers(tree)
  ws = [l["kernel"].numpy() for l in layers]
  if p < 1.0:                                                       # (argpartition takes no kth == n)
    glob = pu._layers(pu.update_global_prune_mask(tree, p))
    flat = np.concatenate([w.reshape(-1) for w in ws])
    want = pc.reference_prune(flat, np.ones(flat.size, np.float32), int(flat.size * p))
    np.testing.assert_array_equal(np.concatenate([l["prune_0"]["mask"].numpy().reshape(-1) for l in glob]), want)
    local = pu._layers(pu.update_prune_mask(tree, p))
    for l, w in zip(local, ws):
      np.testing.assert_array_equal(l["prune_0"]["mask"].numpy(),
                                    pc.reference_prune(w, np.ones(w.shape, np.float32), int(w.size * p)))
  # prune_event from masks of ones is the same selection
  for global_ in (True, False):
    t = pu.ones_masks(tree)
    pu.prune_event(t, p, global_)
    got = [l["prune_0"]["mask"].numpy() for l in pu._layers(t)]
    if global_:
      flat = np.concatenate([w.reshape(-1) for w in ws])
      want = pc.reference_prune(flat, np.ones(flat.size, np.float32), int(flat.size * p))
      np.testing.assert_array_equal(np.concatenate([g.reshape(-1) for g in got]), want)
    else:
      for g, w in zip(got, ws):
        np.testing.assert_array_equal(g, pc.reference_prune(w, np.ones(w.shape, np.float32), int(w.size * p)))


def test_cpu_path_equals_the_reference_on_every_case():
  from snnquantprune_amd import ops
  for name, w, mask, k in CASES:
    t = torch.from_numpy(mask.copy())
    version = t._version
    out = ops.magnitude_prune(torch.from_numpy(w.copy()), t, k)
    assert out is t, name
    np.testing.assert_array_equal(pc.as_i32(t.numpy()), pc.as_i32(pc.reference_prune(w, mask, k)), err_msg=name)
    if k > int((~pc.unpruned(mask)).sum()):
      assert t._version > version, name                             # what caches by version sees the write
  # shaped tensors, in place
  w, mask = torch.randn(5, 7, 3), torch.ones(5, 7, 3)
  ops.magnitude_prune(w, mask, 50)
  np.testing.assert_array_equal(mask.numpy(), pc.reference_prune(w.numpy(), np.ones((5, 7, 3), np.float32), 50))
  for bad in (lambda: ops.magnitude_prune(w, mask, -1), lambda: ops.magnitude_prune(w, mask, 106),
              lambda: ops.magnitude_prune(w, torch.ones(5, 7, 4), 1),
              lambda: ops.magnitude_prune(w, torch.ones(3, 7, 5).permute(2, 1, 0), 1)):
    with pytest.raises(ValueError):
      bad()
  with pytest.raises(TypeError):
    ops.magnitude_prune(w.double(), mask, 1)


def test_prune_event_on_the_three_layers_cpu():
  """Global and per layer, from masks that already hold zeros, written into the same leaves."""
  from snnquantprune_amd import prune_utils as pu
  ws, masks = pc.layer_tensors()
  for global_ in (True, False):
    tree = {"QuantConv_%d" % i: {"kernel": torch.from_numpy(w.copy()), "prune_0": {"mask": torch.from_numpy(m.copy())}}
            for i, (w, m) in enumerate(zip(ws, masks))}
    leaves = [l["prune_0"]["mask"] for l in pu._layers(tree)]
    assert pu.prune_event(tree, 0.5, global_) is None
    assert all(a is l["prune_0"]["mask"] for a, l in zip(leaves, pu._layers(tree)))
    got = [t.numpy() for t in leaves]
    if global_:
      fw, fm = np.concatenate([w.reshape(-1) for w in ws]), np.concatenate([m.reshape(-1) for m in masks])
      want = pc.reference_prune(fw, fm, int(fm.size * 0.5))
      np.testing.assert_array_equal(pc.as_i32(np.concatenate([g.reshape(-1) for g in got])), pc.as_i32(want))
      zeros, weights = pu.mask_zeros(tree)
      assert (int(zeros), weights) == (int(fm.size * 0.5), fm.size)
    else:
      for g, w, m in zip(got, ws, masks):
        np.testing.assert_array_equal(pc.as_i32(g), pc.as_i32(pc.reference_prune(w, m, int(m.size * 0.5))))
  with pytest.raises(ValueError, match="prune_0"):
    pu.prune_event({"QuantDense_0": {"kernel": torch.ones(3)}}, 0.5)


# ---- the schedule -----------------------------------------------------------------------------------

def _quant(**kw):
  from snnquantprune_amd import linen as nn
  return nn.ConfigDict(dict(dict(prune_percentage=0.9), **kw))


def test_sparsity_at():
  from snnquantprune_amd import prune_utils as pu
  q = _quant(prune_schedule=dict(start_epoch=2, end_epoch=9, every_steps=3, initial=0.25))
  s = pu.resolve_prune_schedule(q, 4)
  # end = 36; the last t0 + 3 j no later: 8 + 27 = 35
  assert s == pu.PruneSchedule(8, 35, 3, 0.25)
  events = [t for t in range(60) if s.is_event(t)]
  assert events == list(range(8, 36, 3)) and events[-1] == s.t1
  assert pu.sparsity_at(s.t0, s, 0.9) == 0.25 and pu.sparsity_at(s.t1, s, 0.9) == 0.9
  assert [pu.sparsity_at(t, s, 0.9) for t in (0, 7, 8)] == [0.25] * 3              # the clamps
  assert [pu.sparsity_at(t, s, 0.9) for t in (35, 36, 1000)] == [0.9] * 3
  vals = [pu.sparsity_at(t, s, 0.9) for t in range(60)]
  assert all(a <= b for a, b in zip(vals, vals[1:])) and all(0.25 <= v <= 0.9 for v in vals)
  ks = [int(9973 * v) for v in vals]
  assert all(a <= b for a, b in zip(ks, ks[1:]))
  for t in (11, 20, 34):                                            # the cubic, in Python floats
    assert pu.sparsity_at(t, s, 0.9) == 0.9 + (0.25 - 0.9) * (1.0 - (t - 8) / 27) ** 3
  # a schedule of one event prunes to the final sparsity at once; `initial` defaults to 0
  one = pu.resolve_prune_schedule(_quant(prune_schedule=dict(start_epoch=1, end_epoch=1, every_steps=5)), 4)
  assert one == pu.PruneSchedule(4, 4, 5, 0.0) and pu.sparsity_at(4, one, 0.9) == 0.9 and pu.sparsity_at(3, one, 0.9) == 0.0
  # an end that is no event step: t1 is the last one before it
  s = pu.resolve_prune_schedule(_quant(prune_schedule=dict(start_epoch=0, end_epoch=2, every_steps=3)), 4)
  assert (s.t0, s.t1) == (0, 6) and pu.sparsity_at(6, s, 0.9) == 0.9 and pu.sparsity_at(3, s, 0.9) == 0.9 + (0.0 - 0.9) * 0.5 ** 3


BAD_SCHEDULES = [
    (dict(start_epoch=0, end_epoch=1, every_steps=1, until=3), {}, "unknown keys"),
    (dict(start_epoch=0, end_epoch=1, every_steps=0), {}, "every_steps"),
    (dict(start_epoch=0, end_epoch=1, every_steps=1, initial=-0.1), {}, "initial"),
    (dict(start_epoch=0, end_epoch=1, every_steps=1, initial=0.95), {}, "initial"),
    (dict(start_epoch=2, end_epoch=1, every_steps=1), {}, "end_epoch"),
    (dict(start_epoch=0, end_epoch=1, every_steps=1), dict(prune_percentage=0.0), "prune_percentage"),
    (dict(start_epoch=0, end_epoch=1, every_steps=1), dict(prune_percentage=-0.5), "prune_percentage"),
]


@pytest.mark.parametrize("sched,kw,match", BAD_SCHEDULES, ids=[b[2] + str(i) for i, b in enumerate(BAD_SCHEDULES)])
def test_schedule_refusals(sched, kw, match):
  from snnquantprune_amd import prune_utils as pu
  with pytest.raises(ValueError, match=match):
    pu.check_prune_schedule(_quant(prune_schedule=sched, **kw))


# ---- the C ABI's refusals need no device -------------------------------------------------------------

def test_abi_refusals_without_a_gpu():
  from snnquantprune_amd import _lib as L
  lib = L.lib()
  p = ctypes.c_void_p(256)                                          # never dereferenced: every call is refused
  nbytes = lib.snnqp_magnitude_prune_workspace_bytes(1000)
  assert nbytes > 0 and nbytes % 4 == 0
  assert lib.snnqp_magnitude_prune_workspace_bytes(-1) == L.EINVAL
  assert lib.snnqp_magnitude_prune_workspace_bytes(2 ** 32) == L.EINVAL
  assert lib.snnqp_magnitude_prune_workspace_bytes(2 ** 32 - 1) > 0
  calls = {
      "k > n": (p, p, 10, 11, p, nbytes), "k < 0": (p, p, 10, -1, p, nbytes), "n < 0": (p, p, -1, 0, p, nbytes),
      "n >= 2^32": (p, p, 2 ** 32, 5, p, nbytes), "short workspace": (p, p, 10, 5, p, nbytes - 4),
      "null w": (None, p, 10, 5, p, nbytes), "null mask": (p, None, 10, 5, p, nbytes),
      "null workspace": (p, p, 10, 5, None, nbytes), "misaligned": (p, ctypes.c_void_p(258), 10, 5, p, nbytes),
      "k > n = 0": (None, None, 0, 1, None, 0)}
  for name, args in calls.items():
    assert lib.snnqp_magnitude_prune(*args, None) == L.EINVAL, name
    assert b"magnitude_prune" in lib.snnqp_last_error(), name
  assert lib.snnqp_magnitude_prune(None, None, 0, 0, None, 0, None) == L.OK      # n == 0: nothing looked at
