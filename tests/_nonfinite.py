"""Tableaux with NaN and infinite entries, and options that are not finite (TEST INFRASTRUCTURE, beside tests/_edges.py).

Same construction as tests/_edges.py: dense-LP(M, N, seed) with values planted by fixed formulas, some of them on the rows
and columns of `layout` (E.default_layout), where the kernels split their work.  What the reference (src/simplex.ts) does
with them, and so what every kernel has to do:

  every comparison with a NaN is false: a NaN reduced cost never enters (:75), a NaN right-hand side never leaves (:115), a
  NaN ratio is never taken (:90, :129); `value <= precision` (:87) does not skip a NaN entry, but its ratio is NaN;
  `Math.abs(v) > 1e-16` is false for NaN: a NaN in the pivot row becomes +0.0 (:22), a row whose entry in the pivot column
  is NaN is left alone (:31); a +inf pivot entry has the ratio rhs / inf = 0 <= precision: the early break (:93), the row is
  then divided by inf.

  N1  NaN on the lattice (5 r + 3 c) % 17 == 0, in every 9th reduced cost, in every 11th right-hand side, and where the
      layout's rows and columns cross
  N2  +inf and -inf in turn on the same lattice and crossings: infinite pivot elements, 0 * inf and inf - inf
  N3  infinities on the edges only: +inf right-hand sides, -inf reduced costs, one +inf reduced cost (it enters)
  N4  phase 1 on every third row (negated, as tests/test_resident2_slots.negative_rhs): one right-hand side -inf (it
      leaves), one NaN (it never does), -inf coefficients in the leaving row
  N5  overflow from finite input: column c enters, its only ratio <= precision is in row p (rhs 0) whose pivot entry is
      just above precision and whose other entries are 1e301-sized: p / q overflows to +inf, the updates to -inf and NaN
  N6  four NaN bit patterns -- the kernels' own FLUSHED marker (common.cuh), a negative quiet NaN, a quiet NaN with another
      payload, a signalling NaN -- in the first pivot's row, in its column and in a row that pivot updates; the first
      pivot is fixed as in E2: one reduced cost of 2.0, one smallest ratio 0.25 / 0.5
  N7  options: precision NaN, +inf, -1.0 and maxPivots NaN, -1.0, on dense-LP and on its negative-rhs form (seed - SEED
      counts the ten variants); NaN and +inf precision: "optimal" at once with the result NaN; maxPivots NaN or -1:
      "cycled" at once

All NaNs count as one value when results are compared (tests/_golden.sha256_canon): arithmetic NaNs get the sign and payload
of whichever unit made them."""
import math

import numpy as np

from tests import _edges as E

FAMILIES = ("N1", "N2", "N3", "N4", "N5", "N6", "N7")
PARTITION_FAMILIES = ("N1", "N2", "N6")  # above 8,000,000 cells: the families whose edges depend on the split
MIN_PIVOTS = {"N1": 3, "N2": 3, "N3": 1, "N4": 3, "N5": 1, "N6": 3, "N7": 0}

FLUSHED = 0x7FF8C0DEC0DE5EED  # yalps_amd/csrc/common.cuh
PATTERNS = (FLUSHED, 0xFFF8000000000000, 0x7FF8000000001234, 0x7FF0000000000001)
CANON = 0x7FF8000000000000

N7_PRECISION = (math.nan, math.inf, -1.0, 1e-8, 1e-8)
N7_MAX_PIVOTS = (None, None, None, math.nan, -1.0)  # (None: the budget of the size)
# N7 also runs at these two shapes of more than 8,000,000 cells: the paths `stream` and `stream3-j4` of
# tests/test_edge_paths.py split the pivot budget into launches, and have no smaller shape
N7_EXTRA_SHAPES = ((2800, 3300), (4300, 4096))

SEED = E.SEED
# (family, M, N) -> seed, where SEED does not do what the family is there for at that shape (tests/test_nonfinite_records.py
# asserts it from the reference's trace)
SEEDS = {("N4", 60, 64): 4, ("N4", 200, 150): 4}  # (seed 3: "unbounded" after 2 pivots)


def bits(pattern):
    return np.array([pattern], np.uint64).view(np.float64)[0]


def options(family, M, N, seed):
    o = E.options("E1", M, N, seed)
    if family == "N7":
        k = (seed - SEED) % 5
        o["precision"] = N7_PRECISION[k]
        if N7_MAX_PIVOTS[k] is not None:
            o["max_pivots"] = N7_MAX_PIVOTS[k]
    return o


def _negate_thirds(A):
    A[1::3, 0] *= -0.05
    A[1::3, 1:] *= -1.0


def _distinct(first, pool, count, skip):
    out = [x for x in first if x not in skip]
    for x in pool:
        if len(out) >= count:
            break
        if x not in out and x not in skip:
            out.append(x)
    return sorted(out[:count])


def n6_sites(M, N, layout=None):
    """(c, q, pattern columns of row q, pattern rows of column c, updated row u, its pattern columns)."""
    h, w = M + 1, N + 1
    if layout is None:
        layout = E.default_layout(M, N)
    c = E._cols(layout, w, 1)[0]
    q = E._rows(layout, h, 2)[-1]
    pc = _distinct(E._cols(layout, w, 4, skip=[c]), range(w - 1, 0, -3), 4, {0, c})
    pr = _distinct(E._rows(layout, h, 4), range(h - 1, 0, -5), 4, {0, q})
    u = next(r for r in list(range(q + 1, h)) + list(range(q - 1, 0, -1)) if r not in pr)
    uc = _distinct([], range(2, w, max(1, w // 7)), 4, {0, c} | set(pc))
    return c, q, pc, pr, u, uc


def make(family, M, N, seed, layout=None, dense_lp=None):
    """The (M+1) x (N+1) tableau of the family, flat, row-major, float64."""
    if dense_lp is None:
        from tests import _oracle
        dense_lp = _oracle.load().dense_lp
    if layout is None:
        layout = E.default_layout(M, N)
    h, w = M + 1, N + 1
    m = dense_lp(M, N, seed)
    A = m.reshape(h, w)
    prec = 1e-8
    R, C = E._rows(layout, h, 3), E._cols(layout, w, 3)
    if family in ("N1", "N2"):
        r, c = np.ogrid[:h, :w]
        lat = ((5 * r + 3 * c) % 17 == 0) & (r > 0) & (c > 0)
        lat[np.ix_(R, C)] = True
        if family == "N1":
            A[lat] = math.nan
            A[0, 4::9] = math.nan
            A[3::11, 0] = math.nan
        else:
            A[lat] = np.where((r + c) % 2 == 0, math.inf, -math.inf)[lat]
    elif family == "N3":
        A[2::7, 0] = math.inf
        A[R, 0] = math.inf
        A[0, 3::8] = -math.inf
        A[0, [x for x in C if x != 5]] = -math.inf
        A[0, 5] = math.inf
    elif family == "N4":
        _negate_thirds(A)
        thirds = list(range(1, h, 3))
        near = [t for t in thirds if any(abs(t - b) <= 1 for b in R)] or thirds
        p = near[len(near) // 2]
        n = next(t for t in thirds if t != p)
        A[p, 0] = -math.inf
        A[p, C] = -math.inf
        A[p, 2::13] = -math.inf
        A[n, 0] = math.nan
    elif family == "N5":
        c = E._cols(layout, w, 1)[0]
        p = E._rows(layout, h, 2)[-1]
        A[0, c] = 2.0
        A[p, 1:] *= 1e301
        A[p, 0] = 0.0
        A[p, c] = prec * (1.0 + 2.0 ** -20)
    elif family == "N6":
        c, q, pc, pr, u, uc = n6_sites(M, N, layout)
        pat = np.array(PATTERNS, np.uint64).view(np.float64)
        A[0, c] = 2.0
        A[q, 0], A[q, c] = 0.25, 0.5
        U = A.view(np.uint64)  # (by words: an assignment of doubles need not keep a signalling NaN)
        U[q, pc] = pat.view(np.uint64)[:len(pc)]  # (fewer than four only below the shapes of the records: w < 10, h < 6)
        U[pr, c] = pat.view(np.uint64)[:len(pr)]
        U[u, uc] = pat.view(np.uint64)[:len(uc)]
        U[u, pc[0]] = np.uint64(FLUSHED)
    elif family == "N7":
        if (seed - SEED) // 5 % 2 == 1:
            _negate_thirds(A)
    else:
        raise ValueError(family)
    return m


def shapes_for(family, M, N):
    if (M + 1) * (N + 1) <= 8_000_000:
        return True
    return family in PARTITION_FAMILIES or (family == "N7" and (M, N) in N7_EXTRA_SHAPES)


def specs():
    """(family, M, N, seed) of every record of tests/golden/simplex_nonfinite.json.gz."""
    return [(f, M, N, seed) for M, N in E.SHAPES for f in FAMILIES if shapes_for(f, M, N)
            for seed in (range(SEED, SEED + 10) if f == "N7" else (SEEDS.get((f, M, N), SEED),))]


def label(rec):
    return "%s-%dx%d-s%d" % (rec["family"], rec["M"], rec["N"], rec["seed"])


def initial(rec, dense_lp=None):
    """The initial tableau of a record, regenerated; its bytes (NaN payloads included) must be the ones the reference ran on."""
    m = make(rec["family"], rec["M"], rec["N"], rec["seed"], tuple(rec["layout"]), dense_lp)
    from tests import _golden as G
    assert G.sha256(m) == rec["init_sha256"], "initial tableau differs from the reference's"
    return m


def col0_matches(matrix, rec, exp):
    """Column 0 of a final tableau against the record, all NaNs one value: the doubles, or (large records) their SHA-256."""
    from tests import _golden as G
    col0 = G.canon(matrix.reshape(rec["height"], rec["width"])[:, 0])
    if exp["col0"] is None:
        return G.sha256(col0) == exp["col0_canon_sha256"]
    return np.array_equal(col0.view(np.int64), exp["col0"].view(np.int64))
