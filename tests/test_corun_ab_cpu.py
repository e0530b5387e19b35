"""The host-side pieces of tools/corun_ab.py that need no GPU: the batch chunks
the schedules launch, and the reading of a rocprofv3 kernel trace (which launches of the event layer
and of the bit-input conv were on the device together, and for how long)."""
import importlib.util
import os

import pytest


@pytest.fixture(scope="module")
def tool():
  path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "corun_ab.py")
  spec = importlib.util.spec_from_file_location("corun_ab", path)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.mark.parametrize("B,K", [(1024, 2), (1024, 4), (1024, 8), (5, 2), (4, 4), (7, 3), (9, 1)])
def test_chunks_tile_the_batch_once_in_order(tool, B, K):
  ch = tool.batch_chunks(B, K)
  assert len(ch) == K
  covered = [b for b0, bc in ch for b in range(b0, b0 + bc)]
  assert covered == list(range(B))                       # every sample once, ascending: no gap, no overlap
  sizes = [bc for _, bc in ch]
  assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def test_uneven_batch(tool):
  assert tool.batch_chunks(5, 2) == [(0, 3), (3, 2)]
  assert tool.batch_chunks(4, 4) == [(0, 1), (1, 1), (2, 1), (3, 1)]
  with pytest.raises(AssertionError):
    tool.batch_chunks(3, 4)                              # a chunk would be empty


def test_trace_overlap(tool, tmp_path):
  rows = ["Kernel_Name,Start_Timestamp,End_Timestamp,Grid_Size_X",
          # an earlier schedule of the same process: left out by `last`
          '"void snnqp::conv3x3_u8c2_kernel<1, true>(snnqp::ConvMfmaArgs)",10,20,1536',
          '"void snnqp::conv3x3_bits_kernel<0, 80>(snnqp::ConvMfmaArgs)",20,30,512',
          # conv0(0) alone; conv1(0) beside conv0(1) for 1.5 ms; conv1(1) alone; another kernel ignored
          '"void snnqp::conv3x3_u8c2_kernel<1, true>(snnqp::ConvMfmaArgs)",1000000,2000000,1536',
          '"void snnqp::conv3x3_bits_kernel<0, 80>(snnqp::ConvMfmaArgs)",2000000,4000000,512',
          '"void snnqp::conv3x3_u8c2_kernel<1, true>(snnqp::ConvMfmaArgs)",2000000,3500000,256',
          '"void snnqp::dense_fp6_kernel<3>(snnqp::DenseFp6Args)",2000000,9000000,64',
          '"void snnqp::conv3x3_bits_kernel<0, 80>(snnqp::ConvMfmaArgs)",4000000,5000000,512']
  p = tmp_path / "trace.csv"
  p.write_text("\n".join(rows) + "\n")
  got = tool.trace_overlap(str(p), 2)
  assert got["intervals_ms"] == {"conv0": [[0.0, 1.0], [1.0, 2.5]], "conv1": [[1.0, 3.0], [3.0, 4.0]]}
  assert got["grid_x"] == {"conv0": [1536, 256], "conv1": [512, 512]}
  assert got["side_by_side_ms"] == 1.5 and got["span_ms"] == 4.0
