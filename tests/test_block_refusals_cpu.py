"""Every refusal of the fused blocks' host side, pinned: return code and the whole error text of each
row of tests/block_refusal_cases.py, through the C ABI with made-up pointers.  Nothing is launched --
every row is stopped by a host check (or is an empty batch) -- so no GPU is needed, and none is used
where there is one."""
import ctypes

import pytest

from snnquantprune_amd import _lib as L
from tests import block_refusal_cases as cases


def _fallback_reason(lib, reset):
  conv, dense = ctypes.c_int64(), ctypes.c_int64()
  buf = ctypes.create_string_buffer(256)
  assert lib.snnqp_fallback_counts(ctypes.byref(conv), ctypes.byref(dense), buf, 256, int(reset)) == L.OK
  return conv.value, dense.value, buf.value.decode()


def _run(lib, r):
  symbol, args, keep = cases.call_args(r)
  _fallback_reason(lib, True)
  rc = getattr(lib, symbol)(*args)
  del keep
  return rc, lib.snnqp_last_error().decode(), _fallback_reason(lib, False)


def test_every_row_is_refused_as_recorded():
  lib = L.lib()
  wrong = []
  for r in cases.ROWS:
    rc, text, (nconv, ndense, reason) = _run(lib, r)
    got = (rc, None if rc == L.OK else text)
    if got != (r.code, r.text):
      wrong.append("%s: %r, recorded %r" % (r.name, got, (r.code, r.text)))
    if r.fallback is not None:
      # a call that falls back is counted once, under its kind, with the reason; one that does not, not
      want = (int(r.fallback.startswith("conv: ")), int(r.fallback.startswith("dense: ")))
      if ((nconv, ndense), reason) != (want, r.fallback):
        wrong.append("%s: fallback %r %r, recorded %r" % (r.name, (nconv, ndense), reason, r.fallback))
  assert not wrong, "\n".join(wrong)


def test_no_row_reaches_a_launch():
  """A row that passed every host check would launch on invented pointers: without a device that
  shows as SNNQP_EHIP, with one it must not happen at all -- so every SNNQP_OK row is an empty batch
  (or an answer of the two query functions), by the table itself."""
  for r in cases.ROWS:
    assert r.code in (L.OK, L.EINVAL, L.EUNSUPPORTED), r.name
    if r.code == L.OK and r.entry not in ("half_group", "dequant_form"):
      c = dict(cases.BASE[r.entry][1], **r.change)
      sizes = [c.get(k) for k in ("T", "B", "NB")]
      g = dict(cases.GEOM, **(r.change.get("g") or {}))
      g3 = dict(cases.GEOM3, **(r.change.get("g3") or {}))
      assert 0 in sizes or g["H"] == 0 or g3["D"] == 0, r.name


@pytest.mark.parametrize("name,change,want", cases.WS_ROWS, ids=[w[0] for w in cases.WS_ROWS])
def test_dense_workspace_bytes(name, change, want):
  a = dict(cases.WS_BASE, **change)
  w = None if a["w"] is None else cases._struct("w", a["w"])
  got = L.lib().snnqp_dense_workspace_bytes(a["in_type"], a["T"], a["B"], a["K"], a["N"],
                                            None if w is None else ctypes.byref(w))
  assert got == want, (name, got)
