"""The oracle's convolution off the 3x3 / stride 1 / pad 1 path, pinned by something independent.

tests/test_generic_block_gpu.py calls the direct-form kernel right when it equals the oracle at the
geometries of tests/generic_cases.py; this file is what makes the oracle worth equalling there:
its integer accumulators against torch's convolution (dilations and groups as torch's own
arguments), a census showing each case spikes enough to tell a kernel apart, and the order of the
`fseq` chain under groups.
"""
import numpy as np
import pytest
import torch

from tests import generic_cases as gc

F32 = np.float32
BITS = [b for b, _ in gc.CODES]


def _torch_conv(o, x, q, g):
  """float64 torch convolution of channels-last x [NB, *spatial, Cin] with HWIO / DHWIO codes q:
  zeros inserted for the input dilation, padded by oracle.resolve_padding, the kernel dilation
  and the groups handed to torch.  A 1-D case runs as H = 1."""
  nsp = len(g.spatial)
  in_dil = g.in_dil or (1,) * nsp
  k_dil = g.k_dil or (1,) * nsp
  pads = o.resolve_padding(g.spatial, g.kernel, g.strides, g.padding)
  sp = tuple((g.spatial[i] - 1) * in_dil[i] + 1 for i in range(nsp))
  xd = np.zeros((x.shape[0],) + sp + (g.cin,), np.float64)
  xd[(slice(None),) + tuple(slice(None, None, d) for d in in_dil)] = x
  xd = np.pad(xd, ((0, 0),) + tuple(pads) + ((0, 0),))
  xt = torch.from_numpy(np.ascontiguousarray(np.moveaxis(xd, -1, 1)))                  # [NB, Cin, *spatial]
  wt = torch.from_numpy(np.ascontiguousarray(
      np.transpose(q.astype(np.float64), (nsp + 1, nsp) + tuple(range(nsp)))))        # [Cout, CinG, *k]
  strides, dil = tuple(g.strides), tuple(k_dil)
  if nsp == 1:
    xt, wt, strides, dil = xt.unsqueeze(2), wt.unsqueeze(2), (1,) + strides, (1,) + dil
  fn = torch.nn.functional.conv3d if nsp == 3 else torch.nn.functional.conv2d
  y = fn(xt, wt, stride=strides, dilation=dil, groups=g.groups)
  if nsp == 1:
    y = y.squeeze(2)
  return np.moveaxis(y.numpy(), 1, -1)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", gc.NAMES)
def test_oracle_accumulators_equal_torch(oracle, name, bits):
  """oracle.quant_conv(mode="int", return_acc=True) == torch conv2d / conv3d in float64 (integers:
  the float64 sum is exact, no tolerance), at the output shape written in the table."""
  c = gc.build(oracle, name, bits)
  g = c["g"]
  x = c["x"].reshape((-1,) + c["x"].shape[2:])
  acc = oracle.quant_conv(x, c["qw"], mode="int", return_acc=True, **gc.oracle_kwargs(g))
  assert acc.shape == (x.shape[0],) + tuple(g.out) + (g.cout,)
  assert c["u0"].shape == (g.B,) + tuple(g.out) + (g.cout,)
  e = _torch_conv(oracle, x, c["qw"].q, g)
  assert e.shape == acc.shape
  np.testing.assert_array_equal(acc.astype(np.float64), e)
  assert np.any(acc != 0)


def test_expected_output_shapes_are_the_written_ones():
  """The table's last column, literally."""
  assert {g.name: g.out for g in gc.TABLE} == {
      "dilated_grouped": (4, 21), "group_straddles_word": (6, 7), "depthwise": (8, 6),
      "k5_stride2_valid": (5, 7), "same_kernel_dilation": (8, 8), "input_dilation": (11, 13),
      "kernel_larger_than_image": (2, 3), "1d_dilated_stride": (12,), "1d_same_k4": (10,),
      "explicit_dilated_grouped": (3, 5, 5)}


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", gc.NAMES)
def test_census(oracle, name, bits):
  """Every case, as a block: a spike rate between 0.03 and 0.5, and both a spike and a non-spike in
  the last time step (a kernel that drops the carry is then visible).  A case that leaves the band
  after a change of seeds gets another seed, not another band."""
  c = gc.build(oracle, name, bits)
  u, s = oracle.conv_block(c["x"], c["qw"], c["bn"], None, "int", u0=c["u0"], **gc.oracle_kwargs(c["g"]))
  assert s.shape == (gc.T, c["g"].B) + tuple(c["g"].out) + (c["g"].cout,)
  rate = float(s.mean())
  print("census %s %d-bit: rate %.4f, last step %.4f" % (name, bits, rate, float(s[-1].mean())))
  assert 0.03 <= rate <= 0.5, rate
  assert s[-1].max() == 1 and s[-1].min() == 0
  # the carry matters: the same block from a zero carry ends elsewhere
  u_z, s_z = oracle.conv_block(c["x"], c["qw"], c["bn"], None, "int", **gc.oracle_kwargs(c["g"]))
  assert np.any(u_z != u)


def test_fseq_chain_order_under_groups(oracle):
  """The `fseq` chain of quant_conv with groups runs over (k..., cin) WITHIN the group.  On
  mixed-magnitude real inputs a chain in another order -- (cin, k...) within the group -- gives
  the same sums to rounding but other bits, so the GPU comparison can tell the orders apart."""
  c = gc.build(oracle, "dilated_grouped", 4)
  g = c["g"]
  x = c["xr"][0]
  qw = c["qw"]
  y = oracle.quant_conv(x, qw, mode="fseq", **gc.oracle_kwargs(g))
  pads = oracle.resolve_padding(g.spatial, g.kernel, g.strides, g.padding)
  cg, og, kk = g.cin // g.groups, g.cout // g.groups, int(np.prod(g.kernel))
  w = qw.w_fq.reshape(kk, cg, g.cout)
  straight, permuted = [], []
  for grp in range(g.groups):
    cols = oracle.im2col(x[..., grp * cg:(grp + 1) * cg], g.kernel, g.strides, pads, g.in_dil, g.k_dil)
    lead = cols.shape[:-1]
    c3 = cols.reshape(-1, kk, cg)
    wg = w[:, :, grp * og:(grp + 1) * og]
    straight.append(oracle.fseq_matmul(c3.reshape(-1, kk * cg), wg.reshape(kk * cg, og)).reshape(lead + (og,)))
    permuted.append(oracle.fseq_matmul(np.ascontiguousarray(c3.transpose(0, 2, 1)).reshape(-1, kk * cg),
                                       np.ascontiguousarray(wg.transpose(1, 0, 2)).reshape(kk * cg, og)
                                       ).reshape(lead + (og,)))
  straight, permuted = np.concatenate(straight, -1), np.concatenate(permuted, -1)
  np.testing.assert_array_equal(y, straight)
  assert np.mean(permuted.view(np.uint32) != y.view(np.uint32)) > 0.1
  # ... the same sums: float32 accumulation error of a chain of kk * cg terms
  scale = np.abs(x).max() * np.abs(qw.w_fq).max() * kk * cg
  assert np.max(np.abs(permuted.astype(np.float64) - y)) <= scale * kk * cg * 2.0 ** -24
