"""The work-queue pool of the fused conv kernels (csrc/workqueue.hip): 512 eager slots
per device, sized by the launches a caller may have outstanding.

A step whose first two conv blocks run as 8 batch chunks each has 8 + 8 + 1 conv launches, and a
caller may enqueue 20 such steps without a fence (tools/corun_ab.py): 340 launches outstanding,
on two streams.  None of them may find its slot busy (the static walk is correct, only slower), and
every one computes the oracle's raster.  More than 512 launches in a row come back to slots that
were used before: the zeroing in front of each launch and the busy event behind it are what that
checks, on three streams at once."""
import numpy as np
import pytest
import torch

from tests import cases
from tests.test_parity_gpu import _bn, _mslif, _np, _t, _weight

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available(), "GPU tests need a GPU"
  from snnquantprune_amd import _lib
  _lib.lib()                      # fails loudly if the HIP extension is missing
  return torch.device("cuda:0")


@pytest.fixture(scope="module")
def blocks(dev, oracle):
  """(launch(name) -> PackedSpikes, expected bits by name) of one small launch per conv kernel."""
  from snnquantprune_amd import _lib as L
  from snnquantprune_amd import ops
  jobs, expected = {}, {}
  for name, c in (("bits", cases.conv_block_case(T=3, B=5, hw=16)),
                  ("u8c2", cases.conv_block_case(T=3, B=5, hw=16, cin=2, seed=961, gain=4.0))):
    expected[name] = cases.conv_block_expected(oracle, c)["pooled_bits"]
    w = _weight(c["leaf"], c["bits"], dev, transposed=True)
    g = ops.ConvGeom(16, 16, c["x"].shape[-1], 128, 3, 3, (1, 1), ((1, 1), (1, 1)))
    x = _t(c["x"], dev)
    xin = ops.pack_bits(x) if name == "bits" else x           # (the event layer on uint8 count frames)
    jobs[name] = (xin, g, w, _mslif(), _bn(c["bn"], dev), int(c["x"].max()))

  def launch(name):
    xin, g, w, nrn, bn, x_max = jobs[name]
    return ops.conv_lif_forward(xin, g, w, nrn, bn=bn, want_u=False, packed_out=True, pool=2,
                                impl=L.IMPL_MFMA, x_max=x_max)[1]

  for name in jobs:                  # the pool, the occupancy cache and the allocator's blocks
    np.testing.assert_array_equal(_np(launch(name)), expected[name], err_msg=name)
  torch.cuda.synchronize()
  return launch, expected


def test_twenty_chunked_steps_outstanding_find_every_slot_free(dev, blocks):
  from snnquantprune_amd import ops
  launch, expected = blocks
  side = torch.cuda.Stream(device=dev, priority=-1)
  torch.cuda.synchronize()
  before = ops.workqueue_stats()["busy_static_walks"]
  outs = []
  for step in range(20):
    for chunk in range(8):           # the event layer on the caller's stream, its consumer beside it
      outs.append(("u8c2", launch("u8c2")))
      with torch.cuda.stream(side):
        outs.append(("bits", launch("bits")))
    outs.append(("bits", launch("bits")))
  assert len(outs) == 340
  assert ops.workqueue_stats()["busy_static_walks"] == before      # (counted at the launch, not after it)
  torch.cuda.synchronize()
  want = {name: _t(e.view(np.int32), dev) for name, e in expected.items()}
  for name, s in outs:
    assert torch.equal(s.bits, want[name]), name
  assert ops.device_status() == 0


def test_a_busy_slot_means_the_static_walk(dev, blocks):
  """More launches outstanding than the pool has slots: the stream is held up by a few hundred
  milliseconds of matrix products (the host enqueues 600 small launches in a fraction of that), so
  the launches past the 512th find their slot's event incomplete, are counted and walk their
  patches statically -- the same rasters."""
  from snnquantprune_amd import ops
  launch, expected = blocks
  a = torch.ones((8192, 8192), dtype=torch.float32, device=dev)
  b = torch.empty_like(a)
  torch.mm(a, a, out=b)
  torch.cuda.synchronize()
  before = ops.workqueue_stats()["busy_static_walks"]
  for _ in range(40):
    torch.mm(a, a, out=b)
  outs = []
  for i in range(600):
    name = "bits" if i % 2 else "u8c2"
    outs.append((name, launch(name)))
  busy = ops.workqueue_stats()["busy_static_walks"] - before
  torch.cuda.synchronize()
  want = {name: _t(e.view(np.int32), dev) for name, e in expected.items()}
  for name, s in outs:
    assert torch.equal(s.bits, want[name]), name
  assert 1 <= busy <= 600 - 512, busy
  assert ops.device_status() == 0


def test_slots_reused_after_the_pool_wraps(dev, blocks):
  from snnquantprune_amd import ops
  launch, expected = blocks
  streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
  torch.cuda.synchronize()
  outs = []
  for rep in range(100):             # 600 launches: 88 slots a second time, whatever the pointer was
    for st in streams:
      with torch.cuda.stream(st):
        name = "bits" if (rep + len(outs)) % 2 else "u8c2"
        outs.append((name, launch(name)))
  torch.cuda.synchronize()
  want = {name: _t(e.view(np.int32), dev) for name, e in expected.items()}
  for name, s in outs:
    assert torch.equal(s.bits, want[name]), name
  assert ops.device_status() == 0
