"""The tie cases of tests/tie_cases.py on the oracle alone: every case the GPU file
(tests/test_threshold_ties_gpu.py) compares bit for bit must actually HOLD what it is there for --
membrane potentials exactly on the threshold, rasters that a strict compare would change, pooled
windows whose only spike is a tie.  These are conditions on the cases, not measurements: a case
that misses them is re-tuned (k, input density, prune rate, seed), never exempted."""
import numpy as np
import pytest

from tests import tie_cases as tc

F32 = np.float32

MIN_TIES = 8            # neuron-steps with pre-reset u - v_th == 0
MIN_STRICT_FLIPS = 8    # raster bits a strict compare (u - v_th > 0) changes
MIN_TIE_WINDOWS = 2     # pooled cases: ties that fire alone in their 2x2 window
RATE_BAND = (0.005, 0.7)


def _check(r, what, pooled):
  assert r["ties"] >= MIN_TIES, "%s: %d exact ties in %d neuron-steps" % (what, r["ties"], r["steps"])
  assert r["strict_flips"] >= MIN_STRICT_FLIPS, "%s: a strict compare flips %d bits" % (what, r["strict_flips"])
  assert RATE_BAND[0] <= r["rate"] <= RATE_BAND[1], "%s: firing rate %.4f" % (what, r["rate"])
  if pooled:
    assert r["tie_only_windows"] >= MIN_TIE_WINDOWS, "%s: %d tie-only windows" % (what, r["tie_only_windows"])


@pytest.mark.parametrize("id", tc.CASE_IDS)
def test_case_holds_its_ties(oracle, id):
  r = tc.tie_census(oracle, id)
  c = tc.case(id)
  print("%s: ties %d, strict flips %d, tie-only windows %d, %d neuron-steps, rate %.3f"
        % (id, r["ties"], r["strict_flips"], r["tie_only_windows"], r["steps"], r["rate"]))
  _check(r, id, 2 in c.get("pools", ()))
  if "second" in r:                       # the head: both blocks tie
    _check(r["second"], id + " (second block)", False)
  # a tie fires and is reset: the raster holds the spike, u_T nothing above the threshold
  assert r["u"].dtype == F32 and r["s"].dtype == np.uint8
  assert np.all(r["u"] < F32(tc.build(id)["cfg"]["v_threshold"]))


def test_census_counts_a_known_sequence(oracle):
  """u = u / 2 + x / 2 from 0 with x = 2 every step: every step is a tie that fires and resets;
  a strict compare never fires (u climbs 1, 1.5, 1.75: above the threshold from step 2 on, so
  it fires there) -- counted by hand."""
  x = np.full((3, 1, 1), 2.0, F32)
  r = tc.census_of_currents(oracle, x, tc.neuron_cfg("mul0"))
  assert (r["ties"], r["s"].ravel().tolist(), float(r["u"][0, 0])) == (3, [1, 1, 1], 0.0)
  # strict: step 1 u = 1 (no spike), step 2 u = 1.5 (spike, reset), step 3 u = 1 (no spike)
  assert r["strict_flips"] == 2
  # a 2x2 window whose only spike is the tie, next to one where a neighbour fires as well
  x = np.zeros((1, 1, 2, 4, 1), F32)
  x[0, 0, 0, 0, 0] = 2.0
  x[0, 0, 0, 2, 0] = 2.0
  x[0, 0, 1, 3, 0] = 3.0
  r = tc.census_of_currents(oracle, x, tc.neuron_cfg("mul0"), pooled=True)
  assert (r["ties"], r["tie_only_windows"]) == (2, 1)
  np.testing.assert_array_equal(r["pooled"].ravel(), [1, 1])


BN_CASES = [c["id"] for c in tc.CASES if c.get("bn")]


@pytest.mark.parametrize("id", BN_CASES)
def test_batchnorm_fixtures_fold_to_dyadic_coefficients(oracle, id):
  """The BatchNorm each case actually builds, folded by the oracle's bn_coeffs."""
  c, bn = tc.case(id), tc.build(id)["bn"]
  n = c["cout"] if "cout" in c else c["N"]
  mean, mul, bias = oracle.bn_coeffs(bn["mean"], bn["var"], bn["scale"], bn["bias"], 1e-5)
  assert mean.shape == mul.shape == bias.shape == (n,)
  assert set(np.abs(mul).tolist()) <= {1.0, 0.5, 2.0}
  assert np.all(mean * 8 == np.rint(mean * 8)) and np.all(bias * 8 == np.rint(bias * 8))
  if c["bn"] == "uniform":
    assert set(mul.tolist()) == {{1.0: 1.0, 4.0: 0.5, 0.25: 2.0}[c.get("bn_t", 1.0)]}
    assert not mean.any() and not bias.any()
  else:
    assert len(set(mul.tolist())) > 1                      # the per-channel path, not the uniform fold
  assert ((mul < 0).any() and (mul > 0).any()) == (c["bn"] == "negative")


def test_batchnorm_kinds_are_all_used():
  assert {tc.case(i)["bn"] for i in BN_CASES} == {"uniform", "per_channel", "negative"}


def test_dyadic_constants(oracle):
  assert oracle.sigmoid_f32(F32(0)) == F32(0.5)                     # PLIF tau_param 0, LIF tau_vec 0
  assert oracle.sigmoid_f32(F32(20)) == F32(1.0)                    # LIF tau_vec >= 17
  for bits, k in ((2, 1), (4, 2), (6, 3), (8, 5)):
    leaf = tc.dyadic_leaf((8, 8), bits, k, 3)
    L = 2 ** (bits - 1) - 1
    assert float(leaf["DuQ_0"]["c"][0]) == L * 2.0 ** -k
    assert float(leaf["DuQ_0"]["a"][0]) > 0
  # the grid: fl(fl(n / L) * L * 2^-k) == n * 2^-k for the small accumulators
  qw = tc.qweight(oracle, tc.dyadic_leaf((8, 8), 4, 2, 3), 4)
  n = np.arange(-30, 31)
  np.testing.assert_array_equal(qw.dequant_acc(n), (n * 0.25).astype(F32))
  assert set(tc.gates((50,), 1).tolist()) <= {0.25, 0.5, 0.75, 1.0}


def test_case_list_covers_the_forms_on_both_sides():
  """NF_MUL0, NF_MUL, NF_DIV and NF_DECAY (conv_tile.h) each on a dense path and a conv path."""
  dense = {c["form"] for c in tc.CASES if "K" in c}
  conv = {c["form"] for c in tc.CASES if "cin" in c}
  for side in (dense, conv):
    assert {"mul0", "mul", "div"} <= side and side & {"decay", "decay1"}
