"""Helpers of tests/test_sensitivity_exact.py (TEST INFRASTRUCTURE): lp_sens_kernel's ranging epilogue on matrices the test
writes down entry by entry.

A tableau whose objective row has no entry above the precision in the columns >= 1 and whose column 0 has none below
-precision in the rows >= 1 ends "optimal" after 0 pivots: the final matrix IS the initial one, so the epilogue's input is what
the table says.  table(oracle) is a list of such LPs, one row per purpose, and asserts through the C oracle that each ends
optimal with 0 pivots and its matrix untouched.

  coverage   for the three kernel forms (256-lane LDS, 1024-lane LDS, 1024-lane HBM; checkCycles doubles them in the test), both
             passes and every group size G in 1 .. 64: line lengths on both sides of every power of two, and a number of
             lines that is a multiple of NG = T / G, a multiple plus one and fewer than NG, as far as the byte bounds of the
             form admit (reached(rows) says which)
  planted    LPs in which line j has its winner -- of all four arrays -- at lane position j % G
  IEEE       the threshold, NaN, infinity, signed-zero, subnormal, empty-set and tie rules: once small, once inside a
             1024-lane LDS shape and once inside an HBM shape
  shapes     the aux HBM form in both directions and w = 1, h = 1, w = 2, h = 2

loop_reference() is the reference: a plain double loop over Python floats with an explicit "ignore NaN" rule and strict
comparisons -- no numpy reduction, nothing shared with _np_sensitivity.restate or sensitivity.ranges_from_tableau.
lane_model() walks the matrix the way the kernel's lanes do and can be told to be wrong in four ways."""
import math

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB

INF, NAN = math.inf, math.nan
P = 1e-8  # the precision of every LP of the table
ABOVE_P, BELOW_MINUS_P = float(np.nextafter(P, INF)), float(np.nextafter(-P, -INF))
GROUPS = (1, 2, 4, 8, 16, 32, 64)
LENGTHS = {1: (1,), 2: (2,), 4: (3, 4), 8: (5, 7, 8), 16: (9, 15, 16), 32: (17, 31, 32), 64: (33, 63, 64, 65, 127, 128, 129)}
FORMS = ("256,lds", "1024,lds", "1024")  # lp_sens_kernel<...> without checkCycles
TAILS = ("multiple", "plus one", "fewer")


def group_lanes(count):
    """sens_group_lanes (lp_sens_kernel.cuh), restated: the power of two >= count, at most 64."""
    g = 1
    while g < count and g < 64:
        g *= 2
    return g


def form_of(w, h):
    cls = LB.size_class(w, h)
    assert cls >= 0, (w, h)
    return FORMS[0] if cls < 3 else FORMS[1] if cls == 3 else FORMS[2]


def lanes_of(form):
    return int(form.split(",")[0])


def tail_kind(lines, ng):
    if lines < ng:
        return "fewer"
    return "multiple" if lines % ng == 0 else "plus one" if lines % ng == 1 else "other"


def passes(w, h):
    """[(pass, G, line length, lines)] of a w x h tableau: pass 1 gives a column of h - 1 rows to a group, pass 2 a row of
    w - 1 columns.  A pass without lines is not in the list."""
    out = []
    if w > 1:
        out.append((1, group_lanes(h - 1), h - 1, w - 1))
    if h > 1:
        out.append((2, group_lanes(w - 1), w - 1, h - 1))
    return out


def reached(rows):
    """{(form, pass, G, tail kind)} over the table's rows, by the formulas of the kernel."""
    out = set()
    for _, lp in rows:
        form = form_of(lp[0], lp[1])
        for which, g, _, lines in passes(lp[0], lp[1]):
            out.add((form, which, g, tail_kind(lines, lanes_of(form) // g)))
    return out


# ---------------------------------------------------------------------------------------------- matrices

def random_matrix(rng, w, h):
    """h x w: entries of both signs in 0.25 .. 4, a tenth zeros, some within the precision and some exactly +-P; column 0 in
    0 .. 4 and the objective row in -4 .. 0, both with zeros."""
    M = rng.uniform(0.25, 4.0, (h, w)) * rng.choice([-1.0, 1.0], (h, w))
    kind = rng.random((h, w))
    M[kind < 0.10] = 0.0
    tiny = (kind >= 0.10) & (kind < 0.15)
    M[tiny] = np.sign(M[tiny]) * 1e-9
    edge = (kind >= 0.15) & (kind < 0.17)
    M[edge] = np.sign(M[edge]) * P
    M[:, 0] = np.where(rng.random(h) < 0.1, 0.0, rng.uniform(0.0, 4.0, h))
    M[0, :] = np.where(rng.random(w) < 0.1, 0.0, -rng.uniform(0.0, 4.0, w))
    M[0, 0] = rng.uniform(-5.0, 5.0)
    return M


def shape(which, length, lines):
    """(w, h) of the tableau whose pass `which` has `lines` lines of `length` entries."""
    return (lines + 1, length + 1) if which == 1 else (length + 1, lines + 1)


def coverage_shapes():
    """[(name, w, h)]: for every form, pass, G and tail kind a shape, where the form's byte bounds admit one.  The 256-lane
    form takes every line length of every G with every tail; the two 1024-lane forms, whose LPs are a hundred times larger,
    take every line length once and every tail they can have at least once."""
    out = []
    for form in FORMS:
        T = lanes_of(form)
        for which in (1, 2):
            for g in GROUPS:
                ng = T // g
                if form == FORMS[0]:
                    todo = [(length, tail) for length in LENGTHS[g] for tail in TAILS]
                else:
                    count = max(len(LENGTHS[g]), 2)
                    todo = [(LENGTHS[g][k % len(LENGTHS[g])], TAILS[k % 2]) for k in range(count)]
                    if g == 64:  # (fewer than NG lines of at most G < 64 entries are under 2048 entries: no 1024-lane form)
                        todo.append((LENGTHS[g][0], "fewer"))
                for length, tail in todo:
                    found = None
                    if tail == "fewer":
                        lines = max(1, ng // 2) if form == FORMS[0] else ng - 1
                        if lines >= ng:
                            continue  # (NG = 1 ... does not occur: G <= 64 < T)
                        # a longer line is still a line of G = 64 lanes: grow it until the form is reached
                        for longer in ([length] if g < 64 else [length + 64 * k for k in range(0, 64)]):
                            if form_of(*shape(which, longer, lines)) == form:
                                found = (longer, lines)
                                break
                    else:
                        for k in range(1, 4096):
                            lines = k * ng + (1 if tail == "plus one" else 0)
                            w, h = shape(which, length, lines)
                            if 8 * w * h > LB.MAX_BYTES:
                                break
                            if form_of(w, h) == form:
                                found = (length, lines)
                                break
                    if found:
                        w, h = shape(which, *found)
                        out.append(("%s pass %d G %d length %d lines %d (%s)" % (form, which, g, found[0], found[1], tail), w, h))
    return out


def planted(which, g):
    """An LP whose pass `which` has 2 * G lines of G entries, all beyond the precision; in line j the entry at lane position
    j % G is +64 and the one at (j + 1) % G is -64, so that they win all four arrays (every other |entry| is at most 4, the
    right-hand sides are in 1 .. 2, the objective row in -2 .. -1).  G = 1: the lines alternate in sign."""
    rng = np.random.default_rng(1000 * which + g)
    lines = 2 * g
    w, h = shape(which, g, lines)
    M = rng.uniform(0.5, 4.0, (h, w)) * rng.choice([-1.0, 1.0], (h, w))
    M[:, 0] = rng.uniform(1.0, 2.0, h)
    M[0, :] = -rng.uniform(1.0, 2.0, w)
    for j in range(lines):
        for at, value in (((j % g), 64.0), ((j + 1) % g, -64.0)) if g > 1 else ((0, 64.0 if j % 2 == 0 else -64.0),):
            if which == 1:
                M[1 + at, 1 + j] = value
            else:
                M[1 + j, 1 + at] = value
    return M


# The IEEE block: 20 rows x 20 columns of a tableau, zeros except where a rule is planted.  b[r] is column 0, k[c] the
# objective row; rows and columns are numbered from 1 as in the tableau.
IEEE_ROWS = IEEE_COLS = 20


def ieee_block():
    n = IEEE_ROWS
    A = np.zeros((n + 1, n + 1))
    A[1:, 0] = 1.0
    A[0, 1:] = -1.0
    A[0, 0] = 7.0
    b, k = A[:, 0], A[0, :]
    # entries exactly +P and -P are excluded, the next doubles beyond them are included: columns 1 and 2, rows 3 and 4
    b[1], b[2] = 2.0, 6.0
    A[1, 1], A[2, 1] = P, -P
    A[1, 2], A[2, 2] = ABOVE_P, BELOW_MINUS_P
    k[3], k[4] = -3.0, -5.0
    A[3, 3], A[3, 4] = P, -P
    A[4, 3], A[4, 4] = ABOVE_P, BELOW_MINUS_P
    # a NaN entry is in neither set: column 5 with two ordinary entries below it
    A[5, 5], A[6, 5], A[7, 5] = NAN, 0.5, -0.25
    # +-inf entries: a quotient of 0 that wins against an ordinary one (column 6)
    b[5], b[6], b[7] = 3.0, 4.0, 5.0
    A[5, 6], A[6, 6], A[7, 6] = INF, -INF, 1.0
    # +inf in column 0: against finite entries the quotient is inf, against infinite ones NaN, which is ignored (row 8);
    # row 9 gives the columns of row 8 an ordinary entry each
    b[8], b[9] = INF, 2.0
    A[8, 7], A[8, 8], A[8, 9] = 2.0, INF, -INF
    A[9, 7], A[9, 8], A[9, 9] = 4.0, 1.0, -1.0
    # -inf in the objective row: the same for pass two (column 10; row 10 has a NaN quotient and an ordinary one)
    k[10], k[11] = -INF, -1.0
    A[10, 10], A[10, 11] = INF, 2.0
    A[11, 10], A[11, 11] = 1.0, -0.5
    # 0 in column 0 against a negative and a positive entry: quotients -0.0 and 0.0 (row 12)
    b[12] = 0.0
    A[12, 12], A[12, 13] = -2.0, 2.0
    # a 0 objective entry against entries of both signs (column 14)
    k[14] = 0.0
    A[13, 14], A[14, 14] = 1.0, -1.0
    # subnormal quotients: 1e-300 / 1e10 in pass one (row 15), -1e-300 / -1e10 in pass two (column 16)
    b[15], k[16] = 1e-300, -1e-300
    A[15, 15], A[16, 16] = 1e10, -1e10
    A[16, 15], A[15, 16] = -1e10, 1e10
    # column 17 and row 17 have no entry beyond +-P: +inf, and -inf for row_lo
    A[17, 17], A[18, 17], A[17, 18] = 1e-9, -1e-9, -P
    # ties: equal quotients in neighbouring lanes (column 18 from row 18 on; row 20)
    b[18], b[19], k[19], k[20] = 2.0, 2.0, -1.5, -1.5
    A[18, 18], A[19, 18] = 0.5, 0.5
    A[20, 19], A[20, 20] = 0.5, 0.5
    A[19, 19], A[19, 20] = -0.5, -0.5
    return A


# what the rules above give, worked out by hand: {array: {index: value}} (every other entry of the block is checked against
# the loop reference alone)
IEEE_BY_HAND = {
    "col_up": {1: INF, 2: 2.0 / ABOVE_P, 3: 1.0 / ABOVE_P, 5: 8.0, 6: 0.0, 7: 0.5, 8: 2.0, 9: INF, 13: 0.0, 15: 1e-310, 17: INF, 18: 4.0},
    "col_dn": {1: INF, 2: 6.0 / ABOVE_P, 4: 1.0 / ABOVE_P, 5: 20.0, 6: 0.0, 8: INF, 9: 2.0, 12: 0.0, 17: INF, 18: INF},
    "row_lo": {1: -1.0 / ABOVE_P, 3: -INF, 4: -3.0 / ABOVE_P, 5: 0.0, 10: -0.5, 11: -INF, 13: 0.0, 17: -INF, 20: -3.0},
    "row_hi": {2: 1.0 / ABOVE_P, 3: INF, 4: 5.0 / ABOVE_P, 6: 0.0, 11: 2.0, 14: 0.0, 16: 1e-310, 17: INF, 19: 3.0},
}


def embedded(rng, w, h):
    """The IEEE block in the last rows and columns of an h x w tableau whose other entries are 0 or within the precision, so
    that every line of the block keeps its answer -- now in the last lanes of the last groups."""
    M = np.zeros((h, w))
    fill = rng.random((h, w))
    M[fill < 0.03] = 1e-9
    M[fill > 0.97] = -1e-9
    M[:, 0] = rng.uniform(0.0, 4.0, h)
    M[0, :] = -rng.uniform(0.0, 4.0, w)
    A = ieee_block()
    n = IEEE_ROWS
    M[h - n:, w - n:] = A[1:, 1:]
    M[h - n:, 0] = A[1:, 0]
    M[0, w - n:] = A[0, 1:]
    M[0, 0] = A[0, 0]
    return M


def table(oracle):
    """[(name, lp)], small LPs first.  Every LP is asserted to end optimal after 0 pivots with its matrix bit for bit the input."""
    rows = [("IEEE rules, small", ieee_block())]
    rows += [("planted winners pass %d G %d" % (which, g), planted(which, g)) for which in (1, 2) for g in GROUPS]
    rows += [
        ("w = 1", np.array([[3.0], [1.0], [0.0], [2.0], [5.0]])),
        ("h = 1", np.array([[1.5, -1.0, 0.0, -2.0, -0.0, -3.0]])),
        ("w = 1, h = 1", np.array([[7.0]])),
        ("w = 2", np.array([[0.0, -2.0], [4.0, 2.0], [3.0, -1.0], [0.0, 1e-9], [1.0, 0.5], [6.0, -3.0], [2.0, 0.0]])),
        ("h = 2", np.array([[0.0, -2.0, -1.0, 0.0, -4.0, -0.5, -3.0], [4.0, 2.0, -1.0, 5.0, 1e-9, 0.0, -8.0]])),
    ]
    rng = np.random.default_rng(20250)
    shapes = coverage_shapes()
    rows += [(name, random_matrix(rng, w, h)) for name, w, h in shapes if form_of(w, h) == FORMS[0]]
    rows += [("IEEE rules inside a 1024-lane LDS shape", embedded(rng, 150, 100)), ("IEEE rules inside an HBM shape", embedded(rng, 200, 160))]
    rows += [(name, random_matrix(rng, w, h)) for name, w, h in shapes if form_of(w, h) != FORMS[0]]
    rows += [("aux HBM 2 x 8200", random_matrix(rng, 8200, 2)), ("aux HBM 8200 x 2", random_matrix(rng, 2, 8200))]
    out = []
    for name, M in rows:
        h, w = M.shape
        lp = LB.from_dense(np.ascontiguousarray(M).ravel().copy(), w, h, precision=P)
        if name.startswith("aux HBM"):
            assert form_of(w, h) == FORMS[2] and BS.aux_hbm(w, h), name
        if "inside a 1024-lane LDS" in name or "inside an HBM" in name:
            assert form_of(w, h) == (FORMS[1] if "LDS" in name else FORMS[2]), name
        ref = LB.oracle_answer(oracle, lp)
        assert (ref["status"], ref["n_pivots"]) == ("optimal", 0), (name, ref["status"], ref["n_pivots"])
        assert LB.same_words(ref["matrix"], M.ravel()), name  # (-0.0 and NaN included: from_dense drops only +0.0)
        out.append((name, lp))
    return out


# ---------------------------------------------------------------------------------------------- the reference

def loop_reference(lp):
    """(row0, col_up, col_dn, row_lo, row_hi) of an LP's matrix as include/yalps_lpsens.h defines them, entry by entry: an
    entry v of the body counts for the "up" side where v > p and for the "down" side where v < -p (strictly); its quotient is
    one float64 division; a NaN quotient is ignored; a smaller (row_lo: larger) quotient replaces the running one.  Also
    returns the winners: {array: [index within the line of the entry that set the value, or None]}."""
    w, h, p = lp[0], lp[1], lp[5]
    m = LB.scatter(lp).tolist()
    row0 = m[:w]
    col_up, col_dn = [0.0] + [INF] * (w - 1), [0.0] + [INF] * (w - 1)
    row_lo, row_hi = [0.0] + [-INF] * (h - 1), [0.0] + [INF] * (h - 1)
    win = {"col_up": [None] * w, "col_dn": [None] * w, "row_lo": [None] * h, "row_hi": [None] * h}
    up_at, dn_at, lo_at, hi_at = win["col_up"], win["col_dn"], win["row_lo"], win["row_hi"]
    minus_p = -p
    for r in range(1, h):
        base = r * w
        b = m[base]
        lo, hi = -INF, INF
        for c in range(1, w):
            v = m[base + c]
            if v > p:
                q = b / v
                if q == q and q < col_up[c]:
                    col_up[c], up_at[c] = q, r - 1
                q = row0[c] / v
                if q == q and q > lo:
                    lo, lo_at[r] = q, c - 1
            elif v < minus_p:
                q = b / -v
                if q == q and q < col_dn[c]:
                    col_dn[c], dn_at[c] = q, r - 1
                q = row0[c] / v
                if q == q and q < hi:
                    hi, hi_at[r] = q, c - 1
        row_lo[r], row_hi[r] = lo, hi
    return tuple(np.array(a, np.float64) for a in (row0, col_up, col_dn, row_lo, row_hi)), win


NAMES = ("row0", "col_up", "col_dn", "row_lo", "row_hi")


def differences(got, want):
    """[(array, index)] where `got` is not `want`: row0 bit for bit; the four ratio arrays bit for bit wherever the reference
    is not a zero, and equal as numbers where it is (the minimum of a set is one of its elements: only +-0 depends on the order)."""
    out = []
    for name, g, e in zip(NAMES, got, want):
        g, e = np.ascontiguousarray(g, np.float64), np.ascontiguousarray(e, np.float64)
        if g.shape != e.shape:
            out.append((name, "shape"))
            continue
        same = g.view(np.int64) == e.view(np.int64)
        if name != "row0":
            same |= (e == 0) & (g == 0)
        out += [(name, int(i)) for i in np.flatnonzero(~same)]
    return out


# ---------------------------------------------------------------------------------------------- the kernel's walk, and four wrong ones

def _fmin(a, b):
    return b if a != a else a if b != b else (b if b < a else a)


def _fmax(a, b):
    return b if a != a else a if b != b else (b if b > a else a)


def _min_nan(a, b):
    return a if a != a else b if b != b else (b if b < a else a)  # np.minimum: a NaN operand is the result


def _max_nan(a, b):
    return a if a != a else b if b != b else (b if b > a else a)


FLAWS = ("skips the last lane", "inclusive thresholds", "NaN propagates", "tail left at zero")


def lane_model(lp, flaw=None):
    """The five arrays the way sens_epilogue's lanes compute them: groups of G lanes, lane l striding over the entries
    l, l + G, ... of its line, the butterfly fold, NG = T / G lines per step.  flaw: None, or one of FLAWS --
      "skips the last lane"   the fold loses lane position G - 1 of every group (G >= 2)
      "inclusive thresholds"  >= p and <= -p in place of the strict comparisons
      "NaN propagates"        np.minimum / np.maximum semantics in place of fmin / fmax
      "tail left at zero"     the lines of a last, partial step of NG lines keep 0.0"""
    assert flaw is None or flaw in FLAWS
    w, h, p = lp[0], lp[1], lp[5]
    T = lanes_of(form_of(w, h))
    M = LB.scatter(lp).reshape(h, w).tolist()
    lo_op, hi_op = (_max_nan, _min_nan) if flaw == "NaN propagates" else (_fmax, _fmin)
    inclusive = flaw == "inclusive thresholds"
    above = (lambda v: v >= p) if inclusive else (lambda v: v > p)
    below = (lambda v: v <= -p) if inclusive else (lambda v: v < -p)

    def fold(lanes, op):
        lanes = list(lanes)
        s = len(lanes) >> 1
        while s > 0:
            lanes = [op(lanes[l], lanes[l ^ s]) for l in range(len(lanes))]
            s >>= 1
        return lanes[0]

    def run(count, length, num, den, first_init, second_init, first_op, second_op, negate_second):
        """`count` lines of `length` entries: num(line, i) / den(line, i) folded into two arrays."""
        g = group_lanes(length)
        ng = T // g
        first, second = [0.0] * (count + 1), [0.0] * (count + 1)
        for line in range(1, count + 1):
            if flaw == "tail left at zero" and count % ng and line > count - count % ng:
                continue
            a, z = [first_init] * g, [second_init] * g
            for i in range(length):
                l = i % g
                if flaw == "skips the last lane" and g > 1 and l == g - 1:
                    continue
                v = den(line, i)
                if above(v):
                    a[l] = first_op(a[l], num(line, i) / v)
                elif below(v):
                    q = num(line, i) / v
                    z[l] = second_op(z[l], -q if negate_second else q)
            first[line], second[line] = fold(a, first_op), fold(z, second_op)
        return first, second

    col_up, col_dn = run(w - 1, h - 1, lambda c, i: M[i + 1][0], lambda c, i: M[i + 1][c], INF, INF, hi_op, hi_op, True)
    row_lo, row_hi = run(h - 1, w - 1, lambda r, i: M[0][i + 1], lambda r, i: M[r][i + 1], -INF, INF, lo_op, hi_op, False)
    return tuple(np.array(a, np.float64) for a in (M[0], col_up, col_dn, row_lo, row_hi))
