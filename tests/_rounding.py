"""The inputs of tests/golden/simplex_rounding.json.gz (TEST INFRASTRUCTURE): what the reference's roundToPrecision
(src/util.ts:1-4) and solution() (src/YALPS.ts:8-50) were called on by oracle/tools/gen_golden.py --only rounding.

Every float of that file is its 64-bit word in hex, so a record can tell -0 from +0 (a JSON number cannot: the older golden
files hold `result` as one).  All NaNs are one value (tests/_golden.NAN_WORD).

  kind "round"     one record per precision of PRECISIONS: nums(precision) and roundToPrecision of each
  kind "solution"  solution() on the hand-built final states of states(): the dense form n = 6, m_ub = 4, m_eq = 1
                   (a 7 x 7 tableau of which solution() reads column 0 and the permutations), both signs,
                   includeZeroVariables, as a dense x (tests/_np_dense.model_solution's convention) and a result

The rules the rows sit on: Math.round takes halves toward +infinity and keeps the sign of a zero, so everything in
[-0.5, -0] rounds to -0; `num + 2^-52` comes first; Math.round(1 / precision) is 0 for a precision above 2 (the result is
0 / 0), +-infinity for a precision of 0 or a subnormal one, negative for a negative precision (which also lets zeros past
solution()'s `value > precision`).

MUTANTS: deliberately wrong roundings; tests/test_rounding_records.py shows that the records reject each of them."""
import math

import numpy as np

from tests import _nonfinite as NF

EPS = 2.0 ** -52
NAN_WORD = 0x7FF8000000000000
PRECISIONS = (1e-8, 1e-17, 0.25, 0.75, 2.0, 2.5, 3.0, 0.0, -0.0, 5e-324, -1e-8, -1.0, math.inf, -math.inf, math.nan)

N, M_UB, M_EQ = 6, 4, 1
W, H = N + 1, 1 + M_UB + 2 * M_EQ


def word(x):
    """The 64-bit word of a double, all NaNs one value."""
    return NAN_WORD if x != x else int(np.array([x], np.float64).view(np.uint64)[0])


def hexd(x):
    return "%016x" % word(x)


def unhex(s):
    return float(np.array([int(s, 16)], np.uint64).view(np.float64)[0])


def same_bits(a, b):
    return word(a) == word(b)


def js_round(x):
    """ECMAScript's Math.round: floor(x + 0.5) computed exactly, and -0 for x in [-0.5, -0]."""
    if x != x or math.isinf(x):
        return x
    f = math.floor(x)
    r = f + 1.0 if x - f >= 0.5 else float(f)
    return math.copysign(0.0, x) if r == 0.0 else r


MUTANTS = {
    "old_js_round": "floor(x), + 1 when x - floor(x) >= 0.5: +0 on [-0.5, -0] (what every copy here did)",
    "c_round": "C round(): halves away from zero",
    "rint": "rint(): halves to even",
    "no_epsilon": "roundToPrecision without `+ 2^-52`",
}


def _old_js_round(x):
    if x != x or math.isinf(x):
        return x
    f = math.floor(x)
    return f + 1.0 if x - f >= 0.5 else float(f)


def _c_round(x):
    if x != x or math.isinf(x):
        return x
    r = math.floor(abs(x))
    r = r + 1.0 if abs(x) - r >= 0.5 else float(r)
    return math.copysign(r, x)


def _rint(x):
    return float(np.rint(np.float64(x)))


def round_to_precision(num, precision, mutant=None):
    """src/util.ts:1-4 in float64 (numpy: 1 / 0 and 0 / 0 as IEEE gives them), or one of MUTANTS."""
    rnd = {None: js_round, "old_js_round": _old_js_round, "c_round": _c_round, "rint": _rint, "no_epsilon": js_round}[mutant]
    with np.errstate(all="ignore"):
        rounding = np.float64(rnd(float(np.float64(1.0) / np.float64(precision))))
        v = np.float64(num) if mutant == "no_epsilon" else np.float64(num) + np.float64(EPS)
        return float(np.float64(rnd(float(v * rounding))) / rounding)


def _near(x):
    return (math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf))


def nums(precision):
    """The `num` column of a precision's record, in order, without repeated words."""
    with np.errstate(all="ignore"):
        k = js_round(float(np.float64(1.0) / np.float64(precision)))
    out = [0.0, -0.0, *_near(-EPS), 1.0, -1.0, 0.3, -0.3, 1e300, -1e300, 5e-324, -5e-324]
    if math.isfinite(k) and k != 0.0:
        out += _near(-0.5 / k - EPS) + _near(0.5 / k - EPS)  # the ends of the -0 window (k < 0: the other one is)
        for j in (-3, -2, -1, 0, 1, 2):
            out += _near((j + 0.5) / k) + _near((j + 0.5) / k - EPS)
        out += [0.49999999999999994 / k, -0.49999999999999994 / k]
        for big in (2.0 ** 52, 2.0 ** 52 + 1.0, 2.0 ** 52 + 0.5, 2.0 ** 53, 2.0 ** 53 + 2.0, 2.0 ** 60):
            out += [big / k, -big / k]
    out += [math.inf, -math.inf, math.nan] + [float(NF.bits(p)) for p in NF.PATTERNS]
    seen, rows = set(), []
    for x in out:
        if word(x) not in seen:
            seen.add(word(x))
            rows.append(float(x))
    return rows


def table():
    """[(precision, [num])] of the kind-"round" records."""
    return [(p, nums(p)) for p in PRECISIONS]


def _perms(basic):
    """Both permutations after the variables `basic` {variable: row} entered at those rows (src/simplex.ts:7-12)."""
    pos = np.arange(W + H, dtype=np.int32)
    var = pos.copy()
    for v, row in basic.items():
        col = int(pos[v])
        leaving = int(var[W + row])
        var[W + row], var[col] = v, leaving
        pos[leaving], pos[v] = col, W + row
    return pos, var


def states():
    """Every kind-"solution" input: dicts of label, precision, sign, status, result, col0[H], pos, var."""
    out = []
    for p in PRECISIONS:
        with np.errstate(all="ignore"):
            k = js_round(float(np.float64(1.0) / np.float64(p)))
        kk = k if math.isfinite(k) and k != 0.0 else 1.0
        # A: x1..x5 basic in rows 1..5 at precision, one ulp above and below it, a tie and NaN; x6 is not basic
        colA = np.array([0.0, p, math.nextafter(p, math.inf), math.nextafter(p, -math.inf), 1.5 / kk - EPS, math.nan, 7.0])
        # B: x1, x2, x3 basic in rows 6, 2, 4 at -0.0, 1e300 and another tie; x4..x6 are not basic; row 1 holds a slack
        colB = np.array([0.0, 3.0, 1e300, 5.0, -2.5 / kk - EPS, 9.0, -0.0])
        # C: zeros and a negative value in the basis (a negative precision lets them through `value > precision`)
        colC = np.array([0.0, 0.0, -0.0, -0.5 / kk - EPS, -4e-9, 2.0 ** -40, -EPS])
        A, B = _perms({1: 1, 2: 2, 3: 3, 4: 4, 5: 5}), _perms({1: 6, 2: 2, 3: 4})
        C = _perms({1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6})
        for sign in (1.0, -1.0):
            for tag, col0, (pos, var), result in (("A", colA, A, -0.0), ("A", colA, A, 0.0), ("B", colB, B, 1.5), ("B", colB, B, math.nan),
                                                  ("C", colC, C, -0.0)):
                out.append(dict(label="optimal-%s" % tag, precision=p, sign=sign, status="optimal", result=result, col0=col0, pos=pos, var=var))
            # unbounded: `result` is a position; in A position 6 still holds x6, position 1 the slack that left row 1
            out.append(dict(label="unbounded-structural", precision=p, sign=sign, status="unbounded", result=6.0, col0=colA, pos=A[0], var=A[1]))
            out.append(dict(label="unbounded-slack", precision=p, sign=sign, status="unbounded", result=1.0, col0=colA, pos=A[0], var=A[1]))
            out.append(dict(label="unbounded-position0", precision=p, sign=sign, status="unbounded", result=0.0, col0=colA, pos=A[0], var=A[1]))
            out.append(dict(label="infeasible", precision=p, sign=sign, status="infeasible", result=math.nan, col0=colB, pos=B[0], var=B[1]))
            out.append(dict(label="cycled", precision=p, sign=sign, status="cycled", result=math.nan, col0=colB, pos=B[0], var=B[1]))
    return out


def state_spec(s):
    """A state as JSON data (floats in hex), as the generator hands it to the reference and as a record holds it."""
    return dict(label=s["label"], precision=hexd(s["precision"]), sign=int(s["sign"]), status=s["status"], result=hexd(s["result"]),
                col0=[hexd(x) for x in s["col0"]], pos=[int(x) for x in s["pos"]], var=[int(x) for x in s["var"]])


def dense_x(status, variables):
    """The Solution's `variables` [(index, value)] as a dense x: zeros (NaN for "infeasible" and "cycled") with the listed
    entries written (tests/_np_dense.model_solution)."""
    x = np.full(N, math.nan) if status in ("infeasible", "cycled") else np.zeros(N, np.float64)
    for j, v in variables:
        x[j] = v
    return x


# ---- the family R of the edge machinery (tests/_edges.py): final roundings that end at -0 or NaN ---------------------------
# Same construction as tests/_edges.py: dense-LP(M, N, seed) with values planted by fixed formulas, at every shape of
# E.SHAPES, so that every path of tests/test_edge_paths.py runs them.  The reference's records are
# tests/golden/simplex_rounding_edges.json.gz, with `result_hex` (the result's 64-bit word) beside `result`.
#
#   R0   optimal at 0 pivots: no reduced cost above precision, no right-hand side below -precision, m[0, 0] = -2^-40
#   R1   one pivot: m[0, 0] = +0.0, the one eligible column (cost 2^-20) meets one row with entry 1 and right-hand side
#        2^-20; the final m[0, 0] is 0 - 2^-20 * 2^-20 = -2^-40 exactly
#   R1q  R1 at precision 0.25 with cost 0.5, entry 1, right-hand side 0.25: the final m[0, 0] is -0.125, times the rounding 4
#        the tie -0.5 (less 2^-50): Math.round gives -0
#   R1n  R1 at precision 3.0 with cost 4, entry 4, right-hand side 1: the rounding is Math.round(1 / 3) = 0, the result NaN
#   Rn   many pivots: all but about 30 evenly spaced reduced costs made non-positive, row 0 scaled by 2^-20, the right-hand
#        sides by 2^-k (R_K, chosen per shape on the CPU oracle): "optimal" after at least 8 pivots with the final m[0, 0]
#        inside [-0.5e-8 - 2^-52, -2^-52)
R_FAMILIES = ("R0", "R1", "R1q", "R1n", "Rn")
R_PRECISION = {"R1q": 0.25, "R1n": 3.0}
R1_PLANT = {"R1": (2.0 ** -20, 1.0, 2.0 ** -20), "R1q": (0.5, 1.0, 0.25), "R1n": (4.0, 4.0, 1.0)}  # cost, entry, right-hand side
R_MIN_PIVOTS = {"R0": 0, "R1": 1, "R1q": 1, "R1n": 1, "Rn": 8}
# (M, N) -> k where 16 leaves the final m[0, 0] below the window (tests/test_rounding_records.py asserts the window, the
# status and the pivot count from the reference's records)
R_K = {(600, 2500): 17, (2800, 3300): 18, (900, 7000): 19, (1400, 8192): 19, (2500, 5000): 18, (4300, 4096): 18, (2100, 12345): 20,
       (300, 9000): 20, (600, 16000): 20, (4000, 2000): 17, (200, 20000): 21, (120, 3000): 18, (2300, 4200): 18, (3300, 4200): 18,
       (13000, 2100): 17}
R_K_DEFAULT = 16
R_SEED = 3
R_SEEDS = {("Rn", 300, 200): 4, ("Rn", 60, 50): 4}  # (seed 3: optimal after 7 and 6 pivots)
# one shape per size class of the batch libraries (tests/test_lp_batch.py CLASS_SHAPES): tests/test_rounding_paths.py runs the
# family there against the oracle, which the records pin
R_CLASS_SHAPES = {0: (30, 30), 1: (60, 50), 2: (96, 80), 3: (130, 120), 4: (300, 280)}


def r_options(family, M, N, seed):
    return dict(precision=R_PRECISION.get(family, 1e-8), max_pivots=8192.0, check_cycles=False)


def r_make(family, M, N, seed, layout=None, dense_lp=None):
    """The (M+1) x (N+1) tableau of the family, flat, row-major, float64."""
    from tests import _edges as E
    if dense_lp is None:
        from tests import _oracle
        dense_lp = _oracle.load().dense_lp
    if layout is None:
        layout = E.default_layout(M, N)
    h, w = M + 1, N + 1
    m = dense_lp(M, N, seed)
    A = m.reshape(h, w)
    if family == "R0":
        A[0, 1:] = -np.abs(A[0, 1:])
        A[0, 0] = -2.0 ** -40
    elif family in R1_PLANT:
        cost, entry, rhs = R1_PLANT[family]
        c = E._cols(layout, w, 1)[0]
        q = E._rows(layout, h, 2)[-1]
        A[0, 1:] = -np.abs(A[0, 1:])
        A[0, c] = cost
        A[1:, c] = 0.0
        A[q, c], A[q, 0] = entry, rhs
    elif family == "Rn":
        keep = np.unique(1 + (np.arange(30) * (w - 1)) // 30)
        cost = -np.abs(A[0, 1:])
        cost[keep - 1] = A[0, keep]
        A[0, 1:] = cost * 2.0 ** -20
        A[1:, 0] *= 2.0 ** -R_K.get((M, N), R_K_DEFAULT)
    else:
        raise ValueError(family)
    return m


def r_specs():
    """(family, M, N, seed) of every record of tests/golden/simplex_rounding_edges.json.gz."""
    from tests import _edges as E
    return [(f, M, N, R_SEEDS.get((f, M, N), R_SEED)) for M, N in E.SHAPES for f in R_FAMILIES]


def r_initial(rec, dense_lp=None):
    """The initial tableau of an R record, regenerated; its bytes must be the ones the reference ran on."""
    from tests import _golden as G
    m = r_make(rec["family"], rec["M"], rec["N"], rec["seed"], tuple(rec["layout"]), dense_lp)
    assert G.sha256(m) == rec["init_sha256"], "initial tableau differs from the reference's"
    return m
