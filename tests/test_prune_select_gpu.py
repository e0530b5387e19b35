"""The device path of a prune event (csrc/prune.hip) against the NumPy reference of
tests/prune_select_cases.py, bit for bit on every case; that k <= m writes nothing, that two
launches agree, the C ABI's refusals, and prune_event on the three-layer tree."""
import ctypes

import numpy as np
import pytest
import torch

from tests import prune_select_cases as pc

pytestmark = pytest.mark.gpu

CASES = pc.cases()


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


@pytest.fixture(scope="module")
def expected():
  """The reference's masks, computed once and never written."""
  out = [pc.reference_prune(w, mask, k) for _, w, mask, k in CASES]
  for a in out:
    a.setflags(write=False)
  return out


def test_every_case_bit_for_bit(dev, expected):
  from snnquantprune_amd import ops
  # all launches first, one read at the end
  got = []
  for _, w, mask, k in CASES:
    t = torch.from_numpy(mask.copy()).to(dev)
    assert ops.magnitude_prune(torch.from_numpy(w).to(dev), t, k) is t
    got.append(t)
  torch.cuda.synchronize()
  bad = []
  for (name, _, mask, k), t, want in zip(CASES, got, expected):
    g = pc.as_i32(t.cpu().numpy())
    if not np.array_equal(g, pc.as_i32(want)):
      bad.append((name, int((g != pc.as_i32(want)).sum())))
    if k <= int((~pc.unpruned(mask)).sum()) and not np.array_equal(g, pc.as_i32(mask)):
      bad.append((name, "k <= m wrote"))
  assert not bad, bad
  assert ops.device_status() == 0


def test_k_not_above_m_leaves_the_buffer_unchanged(dev):
  """Also what lies around the n entries: the launch is handed the middle of a larger buffer."""
  from snnquantprune_amd import ops
  rng = np.random.Generator(np.random.PCG64(9))
  n, pad = 4099, 64
  w = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
  host = rng.standard_normal(n + 2 * pad).astype(np.float32)
  host[pad:pad + n][rng.random(n) < 0.4] = 0.0
  host[pad + 5] = -0.0
  m = int((host[pad:pad + n] == 0).sum())
  for k in (0, 1, m - 1, m):
    buf = torch.from_numpy(host.copy()).to(dev)
    ops.magnitude_prune(w, buf[pad:pad + n], k)
    np.testing.assert_array_equal(pc.as_i32(buf.cpu().numpy()), pc.as_i32(host), err_msg="k = %d" % k)
  buf = torch.from_numpy(host.copy()).to(dev)
  ops.magnitude_prune(w, buf[pad:pad + n], m + 7)
  got = buf.cpu().numpy()
  np.testing.assert_array_equal(pc.as_i32(got[:pad]), pc.as_i32(host[:pad]))
  np.testing.assert_array_equal(pc.as_i32(got[pad + n:]), pc.as_i32(host[pad + n:]))
  np.testing.assert_array_equal(pc.as_i32(got[pad:pad + n]),
                                pc.as_i32(pc.reference_prune(w.cpu().numpy(), host[pad:pad + n], m + 7)))


def test_two_launches_give_identical_bytes_and_more_than_one_range_per_workgroup(dev):
  """n past 1024 ranges of 4096: the workgroups' ranges grow, every kernel walks several chunks."""
  from snnquantprune_amd import ops
  rng = np.random.Generator(np.random.PCG64(10))
  n = 1024 * 4096 + 4099
  w = (rng.integers(1, 4000, n).astype(np.float32) / np.float32(4096)) * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32)
  mask = (rng.random(n) < 0.9).astype(np.float32)                   # heavy ties: 4000 magnitudes on 4 M entries
  k = int(n * 0.7)
  wd = torch.from_numpy(w).to(dev)
  a, b = torch.from_numpy(mask).to(dev), torch.from_numpy(mask).to(dev)
  ops.magnitude_prune(wd, a, k)
  ops.magnitude_prune(wd, b, k)
  ga, gb = a.cpu().numpy(), b.cpu().numpy()
  assert ga.tobytes() == gb.tobytes()
  np.testing.assert_array_equal(pc.as_i32(ga), pc.as_i32(pc.reference_prune(w, mask, k)))


def test_abi_refusals_launch_nothing(dev):
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  lib = L.lib()
  n = 300
  w = torch.randn(n, device=dev)
  mask = torch.ones(n, device=dev)
  nbytes = lib.snnqp_magnitude_prune_workspace_bytes(n)
  ws = torch.full((nbytes // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  p = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
  for name, args in {"k > n": (p(w), p(mask), n, n + 1, p(ws), nbytes), "k < 0": (p(w), p(mask), n, -1, p(ws), nbytes),
                     "short workspace": (p(w), p(mask), n, 5, p(ws), nbytes - 1),
                     "null w": (None, p(mask), n, 5, p(ws), nbytes), "null mask": (p(w), None, n, 5, p(ws), nbytes),
                     "null workspace": (p(w), p(mask), n, 5, None, nbytes)}.items():
    assert lib.snnqp_magnitude_prune(*args, st) == L.EINVAL, name
  assert lib.snnqp_magnitude_prune(p(w), p(mask), 0, 0, p(ws), nbytes, st) == L.OK       # n == 0
  assert lib.snnqp_magnitude_prune(None, None, 0, 0, None, 0, st) == L.OK
  torch.cuda.synchronize()
  assert bool((mask == 1).all()) and bool((ws == 0x5A5A5A5A).all())   # not even the workspace was zeroed
  assert ops.device_status() == 0


@pytest.mark.parametrize("global_", [True, False], ids=["global", "per-layer"])
def test_prune_event_on_the_three_layers(dev, global_):
  from snnquantprune_amd import prune_utils as pu
  ws, masks = pc.layer_tensors()
  tree = {"QuantConv_%d" % i: {"kernel": torch.from_numpy(w.copy()).to(dev), "prune_0": {"mask": torch.from_numpy(m.copy()).to(dev)}}
          for i, (w, m) in enumerate(zip(ws, masks))}
  leaves = [l["prune_0"]["mask"] for l in pu._layers(tree)]
  ptrs, versions = [t.data_ptr() for t in leaves], [t._version for t in leaves]
  assert pu.prune_event(tree, 0.6, global_) is None
  now = [l["prune_0"]["mask"] for l in pu._layers(tree)]
  assert all(a is b for a, b in zip(leaves, now)) and [t.data_ptr() for t in now] == ptrs
  assert all(t._version > v for t, v in zip(now, versions))         # the packs cached by version are stale now
  got = [t.cpu().numpy() for t in now]
  if global_:
    fw, fm = np.concatenate([w.reshape(-1) for w in ws]), np.concatenate([m.reshape(-1) for m in masks])
    want = pc.reference_prune(fw, fm, int(fm.size * 0.6))
    np.testing.assert_array_equal(pc.as_i32(np.concatenate([g.reshape(-1) for g in got])), pc.as_i32(want))
    zeros, weights = pu.mask_zeros(tree)
    assert (int(zeros), weights) == (int(fm.size * 0.6), fm.size)
  else:
    for g, w, m in zip(got, ws, masks):
      assert g.shape == m.shape
      np.testing.assert_array_equal(pc.as_i32(g), pc.as_i32(pc.reference_prune(w, m, int(m.size * 0.6))))
