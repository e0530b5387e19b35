"""Plain numpy restatement of snnqp_events_bin_mix (include/snnqp.h) on top of event_aug_cases and
event_cases, and the fixtures the mixing tests share.  The box is stated in final frame pixels, so on
exact, unsaturated counts "drop the events inside it" is "zero the counts inside it": the expected
frame is the primary's exact counts under its record with the box emptied, plus the partner's exact
counts under its record with everything but the box emptied -- saturated per format afterwards
(event_cases.wire) --, and the two sums are the kept-event counts.  Nothing here imports the package
under test."""
import numpy as np

from tests import event_aug_cases as ea
from tests import event_cases as ec

# (H, W) -> scale: 13 x 17 ends in the byte loops; 32 x 32 decodes a 64 x 64 sensor; 130 x 128 is two
# bands whose boundary is the line between rows 127 and 128
SHAPES = {(13, 17): 1.0, (32, 32): 2.0, (130, 128): 1.0}
FRAMES = (1, 3)
START, STEP = 5000, 300
EMPTY, ONE, T_LESS_1, T_EVENTS, THOUSAND, DENSE_A, DENSE_B = range(7)     # the samples of fixture_set
NO_BOX = (0, 0, 0, 0, 0, 0)


def box_slices(box, T, H, W):
  """(frames, rows, columns) slices of a box (x0, y0, x1, y1, g0, g1), clipped to the volume; a box
  that is empty on any axis gives an empty slice there."""
  x0, y0, x1, y1, g0, g1 = (int(v) for v in box)
  cut = lambda lo, hi, n: slice(min(max(lo, 0), n), max(min(max(lo, 0), n), min(max(hi, 0), n)))  # noqa: E731
  return cut(g0, g1, T), cut(y0, y1, H), cut(x0, x1, W)


def mix_counts(own, other, box):
  """Exact counts [T, H, W, 2] of a mixed row from the exact counts of the primary (`own`) and of
  the partner (`other`), and the kept events (nA, nB)."""
  T, H, W = own.shape[:3]
  f, y, x = box_slices(box, T, H, W)
  a = own.copy()
  a[f, y, x] = 0
  b = np.zeros_like(other)
  b[f, y, x] = other[f, y, x]
  return a + b, (int(a.sum()), int(b.sum()))


def decode_batch_mix(ev, sample, plist, partner, plist2, box, T, H, W, mode, start=None, start2=None, step_us=None,
                     scale=1.0):
  """(counts int64 [B, T, H, W, 2], kept int64 [B, 2]): row b decodes sample[b] of `ev` under
  plist[b], mixed with partner[b] (outside [0, S): not mixed) under plist2[b] in box[b].  plist and
  plist2 may be None (identity records)."""
  B, S = len(sample), len(ev["offsets"]) - 1
  ident = [ea.params()] * B
  own = ea.decode_batch_aug(ev, sample, plist or ident, T, H, W, mode, start, step_us, scale)
  out, kept = own.copy(), np.zeros((B, 2), np.int64)
  for b in range(B):
    kept[b, 0] = own[b].sum()
    if not 0 <= int(partner[b]) < S:
      continue
    other = ea.decode_batch_aug(ev, [int(partner[b])], [(plist2 or ident)[b]], T, H, W, mode,
                                None if start2 is None else [start2[b]], step_us, scale)[0]
    out[b], kept[b] = mix_counts(own[b], other, box[b])
  return out, kept


# ---- fixtures --------------------------------------------------------------------------------------

_sets = {}


def fixture_set(hw, T):
  """The samples of a shape and frame count (shared, never modified): 0, 1, T - 1, T and 1000 events
  (event_cases.ragged_set) and two dense ones of 3000 and 2200, all with events on the window edges
  of (START, STEP) and a little outside the scaled frame.  -> (set, scale)"""
  if (hw, T) not in _sets:
    H, W = hw
    scale = SHAPES[hw]
    rng = np.random.Generator(np.random.PCG64(1000 * H + W + 7 * T))
    ragged = [ec.edge_sample(rng, n, H, W, T, START, STEP, scale) for n in ec.ragged_counts(T)]
    dense = [ec.edge_sample(rng, n, H, W, T, START, STEP, scale) for n in (3000, 2200)]
    _sets[(hw, T)] = (ec.make_set(ragged + dense), scale)
  return _sets[(hw, T)]


def all_rules(H, W, T, seed, sign=1):
  """Every rule of a record at once (frame 1 emptied where there is one)."""
  return ea.params(flip_x=1, flip_y=1, swap=1, dx=sign * 3, dy=-sign * 2, cut=(W // 3, H // 4, W // 3 + 5, H // 4 + 4),
                   frames=(1, 2) if T > 1 else (0, 0), drop_below=2 ** 30, seed=seed)


def row(sample, partner, box, p=None, p2=None, expect="both"):
  """One fixture row.  expect: which kept-event counts are positive -- "both", "A" (nB = 0), "B"
  (nA = 0), "none", or "any" for the ragged rows, whose one or two events fall where they fall."""
  return dict(sample=sample, partner=partner, box=tuple(box), p=p or ea.params(), p2=p2 or ea.params(), expect=expect)


def groups(H, W, T):
  """name -> rows.  The middle box covers the central half of each axis; the band box crosses the
  line between rows 127 and 128 of the 130 x 128 frame."""
  P = ea.params
  mid = (W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2, 0, T)
  band = (3, H - 10, W - 3, H - 1, 0, T)
  R = lambda seed, sign=1: all_rules(H, W, T, seed, sign)                          # noqa: E731
  sp = lambda g0, g1: mid[:4] + (g0, g1)                                           # noqa: E731
  return {
      # the box alone: identity records; an unmixed row and a box empty in x beside them
      "box": [row(DENSE_A, DENSE_B, mid), row(DENSE_B, DENSE_A, mid), row(THOUSAND, DENSE_A, mid),
              row(DENSE_A, THOUSAND, mid), row(DENSE_A, -1, mid, expect="A"),
              row(DENSE_B, DENSE_A, (5, 5, 5, 9, 0, T), expect="A")],
      # every rule of both records, two seeds; a row mixed with itself under two records; an unmixed
      # row under every rule; hashed drops alone on both sides
      "rules": [row(DENSE_A, DENSE_B, mid, R(1), R(2, -1)), row(DENSE_B, DENSE_A, mid, R(3, -1), R(4)),
                row(DENSE_A, DENSE_A, mid, R(5), R(6, -1)), row(THOUSAND, DENSE_B, mid, R(7), P(dx=2, dy=-1, swap=1)),
                row(DENSE_B, -1, mid, R(8), expect="A"),
                row(DENSE_A, DENSE_B, mid, P(drop_below=2 ** 31, seed=9), P(drop_below=2 ** 31, seed=10))],
      # the whole frame (the partner's frames), one line along each edge, the band boundary
      "edges": [row(DENSE_A, DENSE_B, (0, 0, W, H, 0, T), expect="B"), row(DENSE_A, DENSE_B, (0, 0, W, 1, 0, T)),
                row(DENSE_B, DENSE_A, (0, H - 1, W, H, 0, T)), row(DENSE_A, DENSE_B, (0, 0, 1, H, 0, T)),
                row(DENSE_B, DENSE_A, (W - 1, 0, W, H, 0, T)), row(DENSE_B, DENSE_A, band, R(11), R(12, -1)),
                row(DENSE_A, DENSE_A, band)],
      # g0 / g1 at 0, at T, and empty ranges
      "frames": [row(DENSE_A, DENSE_B, sp(0, 0), expect="A"), row(DENSE_A, DENSE_B, sp(0, T)),
                 row(DENSE_A, DENSE_B, sp(T, T), expect="A"), row(DENSE_B, DENSE_A, sp(0, 1)),
                 row(DENSE_B, DENSE_A, sp(T - 1, T)), row(DENSE_B, DENSE_A, sp(T // 2, T // 2), expect="A")],
      # an empty partner, an empty primary, both empty, and the samples of 1, T - 1 and T events
      "ragged": [row(DENSE_A, EMPTY, mid, expect="A"), row(EMPTY, DENSE_A, mid, expect="B"),
                 row(EMPTY, EMPTY, mid, expect="none"), row(ONE, DENSE_B, mid, expect="any"),
                 row(DENSE_B, ONE, mid, expect="any"), row(T_LESS_1, T_EVENTS, (0, 0, W // 2, H, 0, T), expect="any"),
                 row(T_EVENTS, T_LESS_1, (0, 0, W, H // 2, 0, T), expect="any"),
                 row(THOUSAND, T_EVENTS, mid, R(13), R(14), expect="any")],
  }


def columns_of(rows):
  """(sample, partner, box int64 [B, 6], plist, plist2, start, start2) of fixture rows; the origins
  differ from row to row and between a row and its partner."""
  B = len(rows)
  return ([r["sample"] for r in rows], [r["partner"] for r in rows],
          np.array([r["box"] for r in rows], np.int64).reshape(B, 6), [r["p"] for r in rows], [r["p2"] for r in rows],
          [START + 7 * (b % 3) - 7 for b in range(B)], [START + 5 - 9 * (b % 2) for b in range(B)])


_expected = {}


def expected(hw, T, group, mode):
  """(counts, kept) of a fixture group, computed once and shared (never modified)."""
  key = (hw, T, group, mode)
  if key not in _expected:
    H, W = hw
    ev, scale = fixture_set(hw, T)
    sample, partner, box, plist, plist2, start, start2 = columns_of(groups(H, W, T)[group])
    _expected[key] = decode_batch_mix(ev, sample, plist, partner, plist2, box, T, H, W, mode, start, start2, STEP, scale)
  return _expected[key]
