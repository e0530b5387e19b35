"""The four scans of training over windows (snnqp_lif_forward_save_state, snnqp_lif_backward_state,
snnqp_neuron_forward_save_state, snnqp_neuron_backward_state) one at a time on the
cases of tests/train_state_cases.py: bit for bit against the oracle-stepped references of
tests/train_state_reference.py and against the existing whole-run entries, the parameter sums
inside nr.param_sum_bound of their float64 reference with u_{-1} = u0."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from snnquantprune_amd import _lib as L
from snnquantprune_amd import ops
from tests import neuron_train_reference as nr
from tests import train_state_cases as sc
from tests import train_state_reference as sr
from tests.train_helpers import _frame_untouched, _framed as _framed_at, _np

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = -12345.5
SURR = L.SURR_ATAN                  # sc.SURROGATE
CASES = sc.kernel_cases()
_ids = [c[0] for c in CASES]
SUM_CASES = [c for c in sc.kernel_cases(sc.SHAPES_C) if c[1] in ("plif", "lif")]
_sum_ids = [c[0] for c in SUM_CASES]
_framed = partial(_framed_at, pad=37)
_frame_intact = partial(_frame_untouched, pad=37)


@pytest.fixture(scope="module")
def dev():
  assert torch.cuda.is_available()
  return torch.device("cuda:0")


def _t(a, dev):
  return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the cases are read-only)


def _ptr(t):
  return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _neuron(c, dev):
  if c["kind"] == sr.MSL:
    return ops.Neuron(L.NEURON_MULTI_STEP_LIF, float(c["par32"]), c["vth"], c["vr"])
  if c["kind"] == sr.PLIF:
    return ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, float(c["par32"]), c["vth"], c["vr"])
  return ops.Neuron(L.NEURON_LIF, 0.0, c["vth"], c["vr"], decay=_t(np.asarray(c["par32"], F32), dev))


def _forward(c):
  return ops.lif_forward_save if c["kind"] == sr.MSL else ops.neuron_forward_save


def _backward(c, h, x, nrn, **kw):
  """-> (gI, gparam or None, gu0 when asked) of either backward."""
  if c["kind"] == sr.MSL:
    out = ops.lif_backward(h, nrn, SURR, **kw)
    return (out[0], None, out[1]) if kw.get("return_gu0") else (out, None)
  return ops.neuron_backward(h, x, nrn, SURR, **kw)


# ---- forward ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_windowed_forward_is_the_whole_run(dev, case):
  """For every split: the windows' h and s, concatenated, are the oracle-stepped reference and the
  existing whole-run scan; every u_T is the reference's carried state; a window without a step
  hands its state on; u0=None is zeros."""
  c = sc.kernel_case(*case[1:])
  nrn, fwd = _neuron(c, dev), _forward(c)
  cur = _t(c["cur"], dev)
  whole_h, whole_s = fwd(cur, nrn)
  np.testing.assert_array_equal(_np(whole_h), c["h"])
  np.testing.assert_array_equal(_np(whole_s), c["s"])
  for split in sc.SPLITS:
    u, hs, ss = None, [], []
    states = sc.boundary_states(c, split) + [c["u_T"]]
    for k, (t0, t1) in enumerate(sr.windows(sc.T, split)):
      h, s, u_T = fwd(cur[t0:t1], nrn, u0=u, return_state=True)
      assert tuple(u_T.shape) == tuple(cur.shape[1:]) and tuple(h.shape) == (t1 - t0,) + tuple(cur.shape[1:])
      np.testing.assert_array_equal(_np(u_T), states[k + 1], err_msg="u_T %s window %d" % (split, k))
      if u is None:
        z = fwd(cur[t0:t1], nrn, u0=torch.zeros_like(cur[0]), return_state=True)
        assert all(torch.equal(a, b) for a, b in zip(z, (h, s, u_T)))
      else:
        assert torch.equal(u, _t(states[k], dev))                       # the input is an input
        h2, s2 = fwd(cur[t0:t1], nrn, u0=u)                             # no u_out asked
        assert torch.equal(h2, h) and torch.equal(s2, s)
      if t1 == t0:
        assert torch.equal(u_T, torch.zeros_like(u_T) if u is None else u)
      u = u_T
      hs.append(h)
      ss.append(s)
    assert torch.equal(torch.cat(hs), whole_h), split
    assert torch.equal(torch.cat(ss), whole_s), split


@pytest.mark.parametrize("case", [c for c in CASES if c[2:4] in ((17, 15), (1, 257))], ids=lambda c: c[0])
def test_forward_abi_in_place_state_frames_and_empties(dev, case):
  """The raw entries with u0 and u_out one buffer, the inputs framed by NaN and the outputs by a
  sentinel: the state walks the reference's boundary states in place, nothing outside is touched;
  T == 0 writes u_out = u0 and nothing else."""
  c = sc.kernel_case(*case[1:])
  nrn = _neuron(c, dev)
  lib = L.lib()
  entry = lib.snnqp_lif_forward_save_state if c["kind"] == sr.MSL else lib.snnqp_neuron_forward_save_state
  R, C = c["cur"].shape[1:]
  st = ctypes.byref(nrn.struct())
  bu, vu = _framed(dev, np.zeros((R, C), F32), SENTINEL)
  split = (2, 0, 3, 1)
  states = sc.boundary_states(c, split) + [c["u_T"]]
  for k, (t0, t1) in enumerate(sr.windows(sc.T, split)):
    bx, vx = _framed(dev, np.array(c["cur"][t0:t1]), float("nan"))        # (a copy: the cases are read-only)
    bh, vh = _framed(dev, np.zeros((t1 - t0, R, C), F32), SENTINEL)
    bs, vs = _framed(dev, np.zeros((t1 - t0, R, C), F32), SENTINEL)
    vh.fill_(SENTINEL)
    vs.fill_(SENTINEL)
    if t1 == t0:
      L.check(entry(None, 0, R, C, st, _ptr(vu), _ptr(vu), None, None, _stream()))
    else:
      L.check(entry(_ptr(vx), t1 - t0, R, C, st, _ptr(vu), _ptr(vu), _ptr(vh), _ptr(vs), _stream()))
      np.testing.assert_array_equal(_np(vh), c["h"][t0:t1])
      np.testing.assert_array_equal(_np(vs), c["s"][t0:t1])
    np.testing.assert_array_equal(_np(vu), states[k + 1])
    assert _frame_intact(bu, R * C, SENTINEL) and _frame_intact(bh, vh.numel(), SENTINEL)
    assert _frame_intact(bs, vs.numel(), SENTINEL) and _frame_intact(bx, vx.numel(), float("nan"))
  # u0 null is zeros; u_out null: h and s alone
  bh, vh = _framed(dev, np.zeros((2, R, C), F32), SENTINEL)
  vs = torch.empty((2, R, C), device=dev)
  L.check(entry(_ptr(_t(c["cur"][:2], dev)), 2, R, C, st, None, None, _ptr(vh), _ptr(vs), _stream()))
  np.testing.assert_array_equal(_np(vh), c["h"][:2])
  assert _frame_intact(bh, vh.numel(), SENTINEL)
  # T == 0 from a null u0 writes zeros; R == 0 launches nothing
  vu.fill_(7.0)
  L.check(entry(None, 0, R, C, st, None, _ptr(vu), None, None, _stream()))
  assert not _np(vu).any() and _frame_intact(bu, R * C, SENTINEL)
  assert entry(None, 3, 0, C, st, None, None, None, None, _stream()) == L.OK


def test_state_entries_refuse_what_the_whole_run_entries_refuse(dev):
  lib = L.lib()
  msl = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  plif = ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, 0.5, 1.0, 0.0)
  lif_no_decay = ops.Neuron(L.NEURON_LIF, 0.0, 1.0, 0.0)
  t = torch.zeros((3, 4, 30), device=dev)
  u = torch.zeros((4, 30), device=dev)
  p, pu, s = _ptr(t), _ptr(u), _stream()
  ws = torch.zeros(4096, dtype=torch.float64, device=dev)
  gp = torch.zeros(30, dtype=torch.float64, device=dev)
  # outputs of their own for the calls that run
  oh, os_, ou, og = (torch.zeros_like(t), torch.zeros_like(t), torch.zeros_like(u), torch.zeros_like(u))
  ph, ps, po, pg = _ptr(oh), _ptr(os_), _ptr(ou), _ptr(og)
  for nrn, lif_rc, neuron_rc in ((msl, L.OK, L.EUNSUPPORTED), (plif, L.EUNSUPPORTED, L.OK)):
    st = ctypes.byref(nrn.struct())
    assert lib.snnqp_lif_forward_save_state(p, 3, 4, 30, st, pu, po, ph, ps, s) == lif_rc
    assert lib.snnqp_lif_backward_state(p, p, None, 10, 3, 4, 30, st, SURR, pu, ph, pg, s) == lif_rc
    assert lib.snnqp_neuron_forward_save_state(p, 3, 4, 30, st, pu, po, ph, ps, s) == neuron_rc
    assert lib.snnqp_neuron_backward_state(p, p, pu, p, None, 10, 3, 4, 30, st, SURR, 1, pu, ph, pg, _ptr(gp),
                                           _ptr(ws), 4096 * 8, s) == neuron_rc
    if neuron_rc != L.OK:
      assert b"snnqp_lif_backward_state" in lib.snnqp_last_error()       # names the entry that serves it
  st = ctypes.byref(msl.struct())
  assert lib.snnqp_lif_forward_save_state(None, 3, 4, 30, st, pu, pu, p, p, s) == L.EINVAL
  assert lib.snnqp_lif_forward_save_state(p, 3, 4, 30, None, pu, pu, p, p, s) == L.EUNSUPPORTED
  assert lib.snnqp_lif_forward_save_state(p, -1, 4, 30, st, pu, pu, p, p, s) == L.EINVAL
  assert lib.snnqp_lif_backward_state(p, p, p, 10, 3, 4, 30, st, SURR, pu, p, pu, s) == L.EINVAL     # gs and glogits
  assert lib.snnqp_lif_backward_state(p, None, p, 7, 3, 4, 30, st, SURR, pu, p, pu, s) == L.EINVAL    # 30 % 7
  assert lib.snnqp_lif_backward_state(None, p, None, 10, 3, 4, 30, st, SURR, pu, p, pu, s) == L.EINVAL
  assert lib.snnqp_lif_backward_state(p, p, None, 10, 3, 4, 30, st, 99, pu, p, pu, s) == L.EINVAL
  st = ctypes.byref(plif.struct())
  assert lib.snnqp_neuron_backward_state(p, p, pu, p, None, 10, 3, 4, 30, st, SURR, 5, pu, p, pu, _ptr(ws), _ptr(ws),
                                         4096 * 8, s) == L.EINVAL                                     # splits > R
  assert lib.snnqp_neuron_backward_state(p, p, pu, p, None, 10, 3, 4, 30, st, SURR, 1, pu, p, pu, _ptr(ws), _ptr(ws),
                                         8, s) == L.EINVAL                                            # workspace
  assert lib.snnqp_neuron_backward_state(p, None, pu, p, None, 10, 3, 4, 30, st, SURR, 1, pu, p, pu, _ptr(ws),
                                         _ptr(ws), 4096 * 8, s) == L.EINVAL                           # PLIF reads x
  assert lib.snnqp_neuron_forward_save_state(p, 3, 4, 30, ctypes.byref(lif_no_decay.struct()), pu, pu, p, p,
                                             s) == L.EINVAL
  with pytest.raises(ValueError, match="u0"):
    ops.lif_forward_save(t, msl, u0=torch.zeros((4, 29), device=dev))
  with pytest.raises(ValueError, match="gu_T"):
    ops.lif_backward(t, msl, SURR, gs=t, gu_T=torch.zeros((5, 30), device=dev))
  torch.cuda.synchronize()


# ---- backward -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_chained_and_truncated_backward(dev, case):
  """Chained: gu0 of window k handed to window k-1 as gu_T -- the concatenated gI is the existing
  whole-run backward's and the float32 recurrence's, the last gu0 the recurrence's.  Truncated
  (gu_T=None): every window's gI is the existing entry run on that window's h.  A window without a
  step hands gu_T on as gu0."""
  c = sc.kernel_case(*case[1:])
  nrn = _neuron(c, dev)
  h, x, gs = _t(c["h"], dev), _t(c["cur"], dev), _t(c["gs"], dev)
  whole = _backward(c, h, x, nrn, gs=gs)[0]
  want_gI, _, want_gu0 = sr.backward_ref32(c["kind"], c["h"], c["gs"], c["par32"], c["vth"], sc.SURROGATE)
  np.testing.assert_array_equal(_np(whole), want_gI)
  g0 = _backward(c, h, x, nrn, gs=gs, return_gu0=True)
  assert torch.equal(g0[0], whole)
  np.testing.assert_array_equal(_np(g0[2]), want_gu0)
  for split in sc.SPLITS:
    wins = sr.windows(sc.T, split)
    u0s = [None if k == 0 else _t(u, dev) for k, u in enumerate(sc.boundary_states(c, split))]
    ref = sc.chained_reference(c, split)
    gu, parts = None, []
    for k in range(len(wins) - 1, -1, -1):
      t0, t1 = wins[k]
      gI, _, gu0 = _backward(c, h[t0:t1], x[t0:t1], nrn, gs=gs[t0:t1], u0=u0s[k], gu_T=gu, return_gu0=True)
      np.testing.assert_array_equal(_np(gu0), ref[k][6], err_msg="gu0 %s window %d" % (split, k))
      if t1 == t0:
        assert torch.equal(gu0, torch.zeros_like(gu0) if gu is None else gu)
      gu = gu0
      parts.append(gI)
      if t1 > t0:
        trunc = _backward(c, h[t0:t1], x[t0:t1], nrn, gs=gs[t0:t1], u0=u0s[k], gu_T=None, return_gu0=True)[0]
        assert torch.equal(trunc, _backward(c, h[t0:t1], x[t0:t1], nrn, gs=gs[t0:t1])[0]), (split, k)
    assert torch.equal(torch.cat(parts[::-1]), whole), split
    np.testing.assert_array_equal(_np(gu), want_gu0)


@pytest.mark.parametrize("case", [c for c in CASES if c[2:4] == (27, 19) or c[2:4] == (16, 16)], ids=lambda c: c[0])
def test_window_vote_is_over_the_windows_own_length(dev, case):
  """glogits: gs_t = glogits / (group T) with T the window's length -- the fused vote equals the
  expanded upstream, with gu_T and gu0 as well."""
  c = sc.kernel_case(*case[1:])
  nrn = _neuron(c, dev)
  R, C = c["h"].shape[1:]
  group = 1 if C % 4 else 4
  rng = np.random.default_rng(R + C)
  gl = (rng.standard_normal((R, C // group))).astype(F32)
  gu_T = rng.standard_normal((R, C)).astype(F32)
  for t0, t1 in ((0, 6), (1, 3), (5, 6)):
    T = t1 - t0
    h, x = _t(c["h"][t0:t1], dev), _t(c["cur"][t0:t1], dev)
    u0 = _t(sc.boundary_states(c, (t0, sc.T - t0))[1], dev) if t0 else None
    gs = _t(sr.vote_upstream(gl, group, T, (T, R, C)), dev)
    a = _backward(c, h, x, nrn, glogits=_t(gl, dev), group=group, u0=u0, gu_T=_t(gu_T, dev), return_gu0=True)
    b = _backward(c, h, x, nrn, gs=gs, u0=u0, gu_T=_t(gu_T, dev), return_gu0=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert a[1] is None or torch.equal(a[1], b[1])
    want = sr.backward_ref32(c["kind"], c["h"][t0:t1], _np(gs), c["par32"], c["vth"], sc.SURROGATE, gu_T)
    np.testing.assert_array_equal(_np(a[0]), want[0])
    np.testing.assert_array_equal(_np(a[2]), want[2])


@pytest.mark.parametrize("case", SUM_CASES, ids=_sum_ids)
def test_window_parameter_sums(dev, case):
  """PLIF and LIF, C at 1, 15, 16, 17 and 65, `splits` in {1, 2, 3, default}: every window's gparam
  lies within nr.param_sum_bound of the float64 sum of the same exact products with u_{-1} = u0
  (tests/test_train_state_cpu.py: with u0 ignored the reference is off by more than that bound);
  gI and gu0 are the recurrence's for every `splits`; two runs give equal bits."""
  c = sc.kernel_case(*case[1:])
  kind, per_feature = c["kind"], c["kind"] == sr.LIF
  nrn = _neuron(c, dev)
  R, C = c["h"].shape[1:]
  h, x, gs = _t(c["h"], dev), _t(c["cur"], dev), _t(c["gs"], dev)
  worst = 0.0
  for split in ((6,), (2, 2, 2), (1, 5), (5, 1)):
    wins = sr.windows(sc.T, split)
    for chained in (True, False):
      ref = sc.chained_reference(c, split, chained)
      for (t0, t1, u0, gu_T, want_gI, gh, want_gu0) in ref:
        n = (t1 - t0) * R * (1 if per_feature else C)
        f = sr.param_factor(kind, c["h"][t0:t1], c["cur"][t0:t1], c["vth"], c["vr"], u0)
        want, _ = nr.param_sum(gh, f, per_feature)
        bound = np.asarray(nr.param_sum_bound(gh, np.zeros(gh.shape), f, per_feature, n))
        for splits in (1, 2, 3, None):
          kw = dict(gs=gs[t0:t1], splits=splits, u0=_t(u0, dev), gu_T=None if gu_T is None else _t(gu_T, dev),
                    return_gu0=True)
          gI, gp, gu0 = ops.neuron_backward(h[t0:t1], x[t0:t1], nrn, SURR, **kw)
          gI2, gp2, gu02 = ops.neuron_backward(h[t0:t1], x[t0:t1], nrn, SURR, **kw)
          assert torch.equal(gI, gI2) and torch.equal(gp, gp2) and torch.equal(gu0, gu02)
          np.testing.assert_array_equal(_np(gI), want_gI)
          np.testing.assert_array_equal(_np(gu0), want_gu0)
          err = np.abs(_np(gp) - np.asarray(want).reshape(gp.shape))
          b = bound.reshape(gp.shape)
          print("%s %s window %d:%d splits %s: error %s of bound %s" % (case[0], split, t0, t1, splits,
                                                                        float(err.max()), float(b.max())))
          assert (err <= b).all(), (split, t0, splits, err, b)
          worst = max(worst, float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0)
  print("%s: largest error / bound %.4f" % (case[0], worst))


def test_backward_empties(dev):
  """R == 0 -- the one shape with fewer rows than `splits` (the interface takes splits in
  1..max(R, 1)), an empty range: zero sums, empty gI and gu0, nothing launched.  T == 0: zero
  sums, gu0 = gu_T."""
  plif = ops.Neuron(L.NEURON_PARAMETRIC_LEAKY_IF, 0.5, 1.0, 0.0)
  lif = ops.Neuron(L.NEURON_LIF, 0.0, 1.0, 0.0, decay=torch.full((30,), 0.5, device=dev))
  msl = ops.Neuron(L.NEURON_MULTI_STEP_LIF, 2.0, 1.0, 0.0)
  e = torch.empty((3, 0, 30), device=dev)
  eu = torch.empty((0, 30), device=dev)
  for nrn, n in ((plif, 1), (lif, 30)):
    gI, gp, gu0 = ops.neuron_backward(e, e, nrn, SURR, gs=e, splits=1, u0=eu, gu_T=eu, return_gu0=True)
    assert tuple(gI.shape) == (3, 0, 30) and tuple(gu0.shape) == (0, 30)
    assert tuple(gp.shape) == (n,) and not _np(gp).any()
  gI, gu0 = ops.lif_backward(e, msl, SURR, gs=e, gu_T=eu, return_gu0=True)
  assert tuple(gI.shape) == (3, 0, 30) and tuple(gu0.shape) == (0, 30)
  z = torch.empty((0, 4, 30), device=dev)
  g = torch.randn((4, 30), device=dev)
  for nrn in (plif, lif):
    gI, gp, gu0 = ops.neuron_backward(z, z, nrn, SURR, gs=z, u0=g, gu_T=g, return_gu0=True)
    assert torch.equal(gu0, g) and not _np(gp).any()
    assert not _np(ops.neuron_backward(z, z, nrn, SURR, gs=z, u0=g, return_gu0=True)[2]).any()
  assert torch.equal(ops.lif_backward(z, msl, SURR, gs=z, gu_T=g, return_gu0=True)[1], g)
  # the raw entries write gu0 = gu_T themselves
  lib = L.lib()
  gu0 = torch.full((4, 30), 7.0, device=dev)
  gp = torch.full((30,), 7.0, dtype=torch.float64, device=dev)
  assert lib.snnqp_neuron_backward_state(None, None, None, _ptr(g), None, 10, 0, 4, 30, ctypes.byref(lif.struct()),
                                         SURR, 1, _ptr(g), None, _ptr(gu0), _ptr(gp), None, 1 << 20, _stream()) == L.OK
  assert torch.equal(gu0, g) and not _np(gp).any()
  gu0.fill_(7.0)
  assert lib.snnqp_lif_backward_state(None, _ptr(g), None, 10, 0, 4, 30, ctypes.byref(msl.struct()), SURR, _ptr(g),
                                      None, _ptr(gu0), _stream()) == L.OK
  assert torch.equal(gu0, g)
