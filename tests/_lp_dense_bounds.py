"""Helpers of tests/test_lp_dense_bounds_model.py and tests/test_lp_dense_bounds.py (TEST INFRASTRUCTURE): the calls the tests
of yalps_lpdense_solve_bounds / linprog_batch(lb=, ub=, upper=) / linprog_objective_bounds make, and the three child processes that
make them on the GPU (tests/_lp_dense.py says why children: torch first).  Each child writes everything its calls left behind to
one .npz; the tests compare those files with the C oracle on tests/_np_dense_bounds.py's restatement.

  BCall           LD.Call with bounds: per LP (c, A_ub, b_ub, A_eq, b_eq, lb, ub), one `upper` for the call
  table(oracle)   [BCall]: every call of the child "table" through _native.LpDense with kept tableaux and all eight outputs
  child "table"   the table; none / some / all output pointers; then the plumbing through linprog_batch and linprog_objective_bounds
  child "hist"    under YALPS_LPDENSE_HIST=4: the rerun writes x, the objective and the bound rows' marginals
  hard_table(oracle)  [BCall]: data whose rounding shows (HARD) and hand-made pins, for the order of shift_sum and the read-out
  child "hard"    the hard table, every call at max_pivots = 0 (the start tableau) and with its own options; the public route; views
"""
import math
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _lp_dense as LD
from tests import _np_dense as ND
from tests import _np_dense_bounds as BD

INF = math.inf
SENTINEL = -7.0
OUTPUTS = ("ineqlin", "eqlin", "reduced", "upper")
STATUS_LPS = 2100             # more than class 0's grid of 8 x 256 workgroups
STATUS_BUDGET = 2.0           # max_pivots of the call "statuses": an LP of more pivots ends "cycled"
BOX_N = 723                   # the largest n whose full box (n + 1) x (1 + n) stays inside 4 MiB: 724 x 724 doubles


class BCall(LD.Call):
    def __init__(self, name, lps, upper=True, **options):
        super().__init__(name, [tuple(lp[:5]) for lp in lps], **options)
        self.lbs, self.ubs = [lp[5] for lp in lps], [lp[6] for lp in lps]
        self.has_lb, self.has_ub = self.lbs[0] is not None, self.ubs[0] is not None
        assert all((a is not None) == self.has_lb for a in self.lbs) and all((a is not None) == self.has_ub for a in self.ubs)
        self.upper = upper
        self.idx = BD.upper_set(self.n, upper, self.has_ub)
        self.k = len(self.idx)
        self.h += self.k

    def bounds_stacked(self):
        """(lb [B, n] or None, ub [B, n] or None)"""
        return (np.stack([np.asarray(a, np.float64) for a in self.lbs]) if self.has_lb else None,
                np.stack([np.asarray(a, np.float64) for a in self.ubs]) if self.has_ub else None)

    def oracle_answer(self, oracle, i, flaw=None):
        """flaw: None, or one of BD.FLAWS: the answer of a kernel that had that flaw (WRONG on purpose)."""
        lp, lb, ub = self.lps[i], self.lbs[i], self.ubs[i]
        m = BD.bounded_tableau(*lp, lb=lb, ub=ub, upper=self.idx, maximize=self.maximize, flaw=flaw)
        start = m.copy()
        pos, var = np.arange(self.w + self.h, dtype=np.int32), np.arange(self.w + self.h, dtype=np.int32)
        status, result, npiv, _ = oracle.simplex(m, self.w, self.h, pos, var, precision=self.precision, max_pivots=self.max_pivots,
                                                 check_cycles=self.check)
        col0 = m.reshape(self.h, self.w)[:, 0].copy()
        sign = 1.0 if self.maximize else -1.0
        x, objective = BD.bounded_solution(col0, pos, var, status, result, sign, self.precision, lp[0], lb, flaw=flaw)
        marg = BD.bounded_marginals(m, pos, status, self.n, self.m_ub, self.m_eq, self.k, sign)
        return dict(status=status, result=result, n_pivots=npiv, matrix=m, start=start, col0=col0, pos=pos, var=var, x=x, objective=objective,
                    **dict(zip(OUTPUTS, marg)))


def random_bounds(rng, n, mode):
    """Small integers: negative lower bounds, boxes of width 0 .. 5, and now and then ub = lb - 1 (infeasible)."""
    lb = rng.integers(-3, 3, n).astype(np.float64)
    ub = lb + rng.integers(0, 6, n).astype(np.float64)
    if n and rng.integers(0, 8) == 0:
        ub[rng.integers(0, n)] -= 6.0
    return (lb if mode in ("lb", "both") else None), (ub if mode in ("ub", "both") else None)


def random_lp(rng, n, m_ub, m_eq, mode):
    """Small integers around a point x0 of the box (lb = 0 where the mode has none), so that most LPs are feasible; the box is
    broken now and then, and a variable without a listed upper bound can make the LP unbounded."""
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    lb, ub = random_bounds(rng, n, "both")
    if mode == "ub":
        lb, ub = None, np.abs(ub)
    x0 = (0.0 if lb is None else lb) + ints(0, 3, n)
    A_ub, A_eq = ints(-2, 4, m_ub, n), ints(-2, 4, m_eq, n)
    return (ints(-2, 5, n), A_ub if m_ub else None, A_ub @ x0 + ints(0, 4, m_ub) if m_ub else None, A_eq if m_eq else None,
            A_eq @ x0 if m_eq else None, lb, ub if mode != "lb" else None)


def random_call(name, B, n, m_ub, m_eq, mode="both", upper=True, **options):
    rng = np.random.default_rng([20261101, B, n, m_ub, m_eq, len(mode)])
    return BCall(name, [random_lp(rng, n, m_ub, m_eq, mode) for _ in range(B)], upper, **options)


def boxed_tableau_call(name, oracle, w, h, k, seed=3, **options):
    """A dense LP of the oracle's generator, w - 1 variables and h - 1 - k rows, maximised, with a box on the first k variables
    (lb in eighths around 0, ub = lb + 1/4 .. 1): the tableau is h x w."""
    n, m = w - 1, h - 1 - k
    c, A, b = ND.from_tableau(oracle.dense_lp(m, n, seed), w, m + 1)
    rng = np.random.default_rng([20261102, w, h, k])
    lb = rng.integers(-2, 3, n).astype(np.float64) / 8.0
    ub = lb + rng.integers(2, 9, n).astype(np.float64) / 8.0
    return BCall(name, [(c, A, b, None, None, lb, ub)], upper=tuple(range(k)), maximize=True, **options)


def bound_shapes():
    """(class, w, h) under and over three LDS class bounds: the first (256 lanes on both sides), the one between the 256-lane
    and the 1024-lane forms, and the last (1024 lanes in LDS against the HBM form)."""
    s = LD.bound_shapes()
    return s[:2] + s[4:6] + s[-2:]


def box_call():
    """n = k = BOX_N, no rows: maximise c . x over the box, c of both signs: every variable ends at one of its bounds, and
    the bound rows' marginals are the positive c's -- up to the last lane that has one."""
    rng = np.random.default_rng(20261103)
    c = rng.integers(-4, 5, BOX_N).astype(np.float64)
    c[-1], c[0] = 3.0, 2.0
    lb = rng.integers(-3, 3, BOX_N).astype(np.float64)
    ub = lb + rng.integers(1, 4, BOX_N).astype(np.float64)
    return BCall("box n=k=%d" % BOX_N, [(c, None, None, None, None, lb, ub)], maximize=True)


def statuses_call():
    """2100 LPs of 4 variables of which two are boxed: optimal, infeasible (a box with lb > ub among them), unbounded through an
    unlisted variable, and cycled by a budget of two pivots."""
    return random_call("statuses", STATUS_LPS, 4, 4, 0, upper=(0, 2), maximize=True, max_pivots=STATUS_BUDGET)


def nonfinite_call():
    """lb holding +inf, -inf and NaN, ub holding +inf: taken as they lie."""
    call = random_call("nonfinite bounds", 6, 5, 3, 1)
    for i, (j, v) in enumerate(((0, INF), (1, -INF), (2, math.nan), (3, INF))):
        (call.ubs if i == 3 else call.lbs)[i][j] = v
    return call


def hist_call(oracle):
    """LD.hist_call's four LPs (checkCycles, more pivots than 2 * HIST) with a box on every variable wide enough not to bind early."""
    base = LD.hist_call(oracle)
    rng = np.random.default_rng(20261104)
    lps = []
    for lp in base.lps:
        lb = rng.integers(-2, 3, base.n).astype(np.float64) / 8.0
        lps.append((*lp, lb, lb + 64.0))
    return BCall("hist bounds", lps, maximize=True, check=True)


def names():
    out = ["n=%d" % n for n in (1, 2, 63, 64, 65, 129)]
    out += ["bound rows only", "equalities only", "k=0", "k=1 first", "k=1 last", "lb only", "ub only", "both, check", "both, minimize n=64"]
    out += ["class %d bound %s" % (k, "under" if j % 2 == 0 else "over") for j, (k, w, h) in enumerate(bound_shapes())]
    out += ["HBM odd n 301x280", "aux", "aux check", "box n=k=%d" % BOX_N, "statuses", "nonfinite bounds", "hist bounds clean"]
    return out


def table(oracle):
    R = random_call
    T = [R("n=%d" % n, 3, n, 3, 2, maximize=n % 2 == 1) for n in (1, 2, 63, 64, 65, 129)]
    T += [R("bound rows only", 6, 5, 0, 0, maximize=True), R("equalities only", 6, 9, 0, 4), R("k=0", 6, 5, 4, 1, upper=()),
          R("k=1 first", 6, 5, 4, 1, upper=(0,), maximize=True), R("k=1 last", 6, 5, 4, 1, upper=(4,)), R("lb only", 8, 5, 4, 3, mode="lb"),
          R("ub only", 8, 5, 4, 3, mode="ub", maximize=True), R("both, check", 8, 5, 4, 3, check=True), R("both, minimize n=64", 4, 64, 5, 0)]
    for j, (k, w, h) in enumerate(bound_shapes()):
        assert LB.size_class(w, h) == k + j % 2 and LB.size_class(w, h - 4) == k, (k, w, h)  # (without the 4 bound rows: under)
        T.append(boxed_tableau_call("class %d bound %s" % (k, "under" if j % 2 == 0 else "over"), oracle, w, h, 4))
    assert LB.size_class(280, 301) == 4 and not BS.aux_hbm(280, 301)
    T.append(boxed_tableau_call("HBM odd n 301x280", oracle, 280, 301, 279))
    m_ub, n = LD.AUX_SHAPE
    assert BS.aux_hbm(n + 1, m_ub + 1) and not BS.aux_hbm(n + 1, m_ub + 1 - n)  # (the bound rows make it the aux form)
    T += [boxed_tableau_call("aux" + (" check" if check else ""), oracle, n + 1, m_ub + 1, n, max_pivots=INF, check=check) for check in (False, True)]
    T += [box_call(), statuses_call(), nonfinite_call()]
    clean = hist_call(oracle)
    clean.name = "hist bounds clean"
    T.append(clean)
    assert [c.name for c in T] == names()
    return T


def partial_call():
    return random_call("partial", 8, 5, 4, 3)


PARTIAL = ((), ("upper",), ("ineqlin", "reduced"), OUTPUTS)


def gradient_lp():
    """Data in eighths, a box that binds: minimise c . x, c of both signs, over A_ub x <= b_ub, lb <= x <= ub."""
    e = lambda *v: np.array(v, np.float64) / 8.0
    return (e(-16, 8, -24), np.array([e(8, 16, 8), e(16, 8, 24)]), e(24, 64), None, None, e(-8, 4, -4), e(8, 20, 12))


GRAD_PRECISION, GRAD_H = 1e-8, 2.0 ** -6
GRADIENT_WEIGHTS = (2.0, -0.5, 3.0)


def gradient_call():
    """The gradient LP, the same with another c, and the first again with ub[0] < lb[0] (infeasible)."""
    lp = gradient_lp()
    other = (lp[0] * -1.0, *lp[1:])
    bad = list(lp)
    bad[6] = lp[6].copy()
    bad[6][0] = lp[5][0] - 1.0
    return BCall("gradient rows", [lp, other, tuple(bad)], precision=GRAD_PRECISION)


def difference_call():
    """[lp, then (+h, -h) for every entry of lb, then of ub]: central differences of the objective."""
    lp = gradient_lp()
    out = [lp]
    for op in (5, 6):
        for j in range(3):
            for d in (GRAD_H, -GRAD_H):
                moved = [None if a is None else np.array(a, np.float64) for a in lp]
                moved[op][j] += d
                out.append(tuple(moved))
    return BCall("differences", out, precision=GRAD_PRECISION)


# ------------------------------------------------------------------------------------------------ the hard calls
# Data whose rounding shows: no product a[j] * lb[j] is exact and no two orders of adding them agree for long, so the bits of a
# right-hand side tell THE order of shift_sum from BD.SUM_FLAWS, and the bits of x and of the objective tell the read-out from
# BD.READ_FLAWS.  tests/test_lp_dense_bounds_model.py holds the floors (by call and flaw) that the seeds below were picked for, with
# the oracle alone.
# name: (B, n, m_ub, m_eq, upper or None: no ub, seed, chain, depth, options)
HARD = {
    # class 0: seven operand rows over the four waves of 256 lanes, two trips, the last one partial; lanes 0 and 1 hold three columns
    "hard <256,lds>": (6, 129, 5, 2, (1, 128), 0, 0, 1.0, dict(maximize=True)),
    "hard <256,check,lds>": (6, 129, 5, 2, (1, 128), 0, 0, 1.0, dict(maximize=True, check=True)),
    # one lane with two columns, 64 full lanes, one lane short
    "hard n=65": (6, 65, 5, 2, (1, 64), 5, 0, 1.0, dict(maximize=True)),
    "hard n=64": (6, 64, 5, 2, (1, 63), 0, 0, 1.0, dict(maximize=True)),
    "hard n=63": (6, 63, 5, 2, (1, 62), 0, 0, 1.0, dict(maximize=True)),
    # class 3: seventeen operand rows over the sixteen waves of 1024 lanes
    "hard <1024,lds>": (4, 449, 15, 2, (1, 448), 0, 0, 1.0, dict(maximize=True)),
    "hard <1024,check,lds>": (4, 449, 15, 2, (1, 448), 0, 0, 1.0, dict(maximize=True, check=True)),
    # class 4 without aux: rhs lies in HBM
    "hard <1024> HBM": (3, 1025, 20, 1, (1, 1024), 0, 0, 1.0, dict(maximize=True)),
    "hard <1024,check>": (3, 1025, 20, 1, (1, 1024), 0, 0, 1.0, dict(maximize=True, check=True)),
    # the aux form: every lane holds 128 or 129 columns, the tableau is 4 x 8194.  Three rows end after a few pivots: the chain.  A sum
    # of 8193 products of mean 1 is some 30 times its shift, and the subtraction would round most one-ulp changes away: x0 lies near lb
    "hard aux wide": (3, 8193, 2, 0, (8192,), 0, 12, 2.0 ** -6, dict(maximize=True)),
    # the other sign, and no bound rows
    "hard minimize, lb only": (6, 129, 5, 2, None, 1, 0, 1.0, dict()),
}
HARD_FORMS = {"hard <256,lds>": (0, 0), "hard <256,check,lds>": (0, 0), "hard n=65": (0, 0), "hard n=64": (0, 0), "hard n=63": (0, 0),
              "hard <1024,lds>": (3, 0), "hard <1024,check,lds>": (3, 0), "hard <1024> HBM": (4, 0), "hard <1024,check>": (4, 0),
              "hard aux wide": (4, 1), "hard minimize, lb only": (0, 0)}  # name: (LB.size_class, BS.aux_hbm)
PUBLIC_HARD = ("hard <256,lds>", "hard aux wide")  # once more through linprog_batch(duals=True): only the objective carries the shift there
VIEWS_HARD = "hard <256,lds>"                      # the n = 129 call whose operands are also given as views
PIN_NAMES = ("pins n=65", "pins n=64", "pin -0 objective, lb=0", "pin -0 objective, no lb")
PIN_SHAPE = (30, 29)  # (M, N) of the _rounding family's LP


def hard_lp(rng, n, m_ub, m_eq, has_ub, maximize, chain=0, depth=1.0):
    """lb ~ N(0, 1), ub = lb + 0.25 + 3 U, a point x0 of the box, A = 6 U - 2, b_ub = A_ub x0 + slack, b_eq = A_eq x0.  The first
    row of A_ub is positive (0.5 + U): together with x >= lb it bounds every variable, so the LP is bounded whatever c's signs.
    c = that row * (1 + N(0, 1) / 8), negated for a minimising call: the quotients c[j] / A_ub[0, j] lie close together, and the
    pivot rule (largest reduced cost first, not largest quotient) changes its mind many times.
    chain: that many columns, spread at random, whose first-row entries fall by thirds while their quotients rise, and whose
    other entries are negative: they enter one after the other, whatever else the LP holds (a tableau of three rows is
    otherwise done after a handful of pivots)."""
    lb = rng.standard_normal(n)
    ub = lb + 0.25 + 3.0 * rng.random(n)  # (depth: how far into the box x0 may lie; the right-hand sides shrink with it)
    x0 = lb + (ub - lb) * depth * rng.random(n)
    A_ub, A_eq = rng.random((m_ub, n)) * 6.0 - 2.0, rng.random((m_eq, n)) * 6.0 - 2.0
    A_ub[0] = 0.5 + rng.random(n)
    c = A_ub[0] * (1.0 + rng.standard_normal(n) / 8.0)
    if chain:
        cols, t = np.sort(rng.choice(n - 1, chain, replace=False)), np.arange(1, chain + 1)
        A_ub[0, cols] = 3.0 ** -t * (1.0 + 0.01 * rng.random(chain))
        A_ub[1:, cols] = -(1.0 + rng.random((m_ub - 1, chain)))
        c[cols] = A_ub[0, cols] * (2.0 + 0.1 * t)
    b_ub = A_ub @ x0 + 0.125 * rng.random(m_ub)
    return (c if maximize else -c, A_ub, b_ub, A_eq if m_eq else None, A_eq @ x0 if m_eq else None, lb, ub if has_ub else None)


def hard_call(name, B, n, m_ub, m_eq, upper, seed=0, chain=0, depth=1.0, **options):
    rng = np.random.default_rng([20261201, n, m_ub, m_eq, seed])
    lps = [hard_lp(rng, n, m_ub, m_eq, upper is not None, bool(options.get("maximize")), chain, depth) for _ in range(B)]
    call = BCall(name, lps, upper if upper is not None else True, **options)
    if name in HARD_FORMS:
        assert (LB.size_class(call.w, call.h), int(BS.aux_hbm(call.w, call.h))) == HARD_FORMS[name], (name, call.w, call.h)
    return call


def pin_lp(n, a, lb, b):
    """One A_ub row `a` {column: value} over zeros with the right-hand side b; minimise the sum of x over x >= lb."""
    row = np.zeros((1, n))
    for j, v in a.items():
        row[0, j] = v
    return (np.ones(n), row, np.array([b], np.float64), None, None, np.asarray(lb, np.float64), None)


# what the pins' right-hand side (cell (1, 0) of the start tableau) is, and what the flaw named beside it makes of it
PINS_65 = ((0.5, "left to right", -0.5), (0.0, "fused", -2.0 ** -60), (-INF, "left to right", 0.25 - 1.5e308), (-0.0, None, None),
           (0.0, "lanes of 32", -1.0))
PINS_64 = ((-1.0, "fold upward", 0.0), (0.0, "fold upward", -1.0))


def pin_calls(oracle):
    """Hand-made rows whose shift has one known canonical value and one known wrong one (PINS_65, PINS_64, in order), lb given:
      n = 65  1e16 at column 0, -1e16 at column 1, 1 at column 64, lb = 1, b = 0.5: lane 0 loses the 1, the shift is 0.0
              1 * -(1 + 2^-29) at column 0 and (1 + 2^-30)^2 at column 64: the rounded product cancels exactly, the fused one not
              1.5e308 at columns 0 and 64, -1.5e308 at column 1, lb = 1: lane 0 overflows, the shift is +inf; b = 0.25
              a = 1, lb all -0.0, b = -0.0: every product is -0.0, but the sums start from +0.0: -0.0 - +0.0 stays -0.0
              1e16, -1e16, 1 at columns 0, 32, 64: lane 0 adds columns 0 and 64 first, the 1 is lost; 32 lanes would keep it
      n = 64  1e16, -1e16, 1 at columns 0, 32, 16: lanes 0 and 32 meet first, the 1 survives; and 1e16, 1, -1e16: it does not
    and one LP of tests/_rounding.py's family R1, minimised: its objective is -0.0 without lb and, through the one addition of
    shift_sum(c, 0) = +0.0, +0.0 with lb = 0."""
    from tests import _rounding as RD
    one, e = np.ones(65), 1.0 + 2.0 ** -30
    l = one.copy()
    l[0], l[64] = -(1.0 + 2.0 ** -29), e
    p65 = [pin_lp(65, {0: 1e16, 1: -1e16, 64: 1.0}, one, 0.5), pin_lp(65, {0: 1.0, 64: e}, l, 0.0),
           pin_lp(65, {0: 1.5e308, 1: -1.5e308, 64: 1.5e308}, one, 0.25), pin_lp(65, dict(enumerate(one)), -0.0 * one, -0.0),
           pin_lp(65, {0: 1e16, 32: -1e16, 64: 1.0}, one, 0.0)]
    p64 = [pin_lp(64, {0: 1e16, 32: -1e16, 16: 1.0}, np.ones(64), 0.0), pin_lp(64, {0: 1e16, 32: 1.0, 16: -1e16}, np.ones(64), 0.0)]
    M, N = PIN_SHAPE
    m = RD.r_make("R1", M, N, RD.R_SEED, dense_lp=oracle.dense_lp).reshape(M + 1, N + 1)
    assert m[0:1, 0].view(np.int64)[0] == 0
    lp = (-m[0, 1:], m[1:, 1:].copy(), m[1:, 0].copy(), None, None)  # (minimised: row 0 is -1 * c, the same words)
    assert np.array_equal(ND.dense_tableau(*lp).view(np.int64), m.ravel().view(np.int64))
    out = [BCall(PIN_NAMES[0], p65), BCall(PIN_NAMES[1], p64), BCall(PIN_NAMES[2], [(*lp, np.zeros(N), None)]),
           BCall(PIN_NAMES[3], [(*lp, None, np.full(N, 64.0))], upper=())]
    return out


def hard_names():
    return list(HARD) + list(PIN_NAMES)


def hard_table(oracle):
    T = [hard_call(name, *shape[:-1], **shape[-1]) for name, shape in HARD.items()]
    T += pin_calls(oracle)
    assert [c.name for c in T] == hard_names()
    return T


def at_budget_0(call):
    """The same call with max_pivots = 0: simplex stops in front of the first pivot ("cycled"), the kept tableau is the start tableau."""
    import copy
    out = copy.copy(call)
    out.name, out.max_pivots = call.name + " @0", 0.0
    return out


_answers = {}


def hard_answers(oracle, call, flaw=None):
    """[oracle_answer(i, flaw)] of a call of the hard table, computed once per process (both test modules ask for them)."""
    key = (call.name, call.max_pivots, flaw)
    if key not in _answers:
        _answers[key] = [call.oracle_answer(oracle, i, flaw) for i in range(len(call.lps))]
    return _answers[key]


def differing(a, b):
    """How many words of two float64 arrays differ, all NaNs counted as one value."""
    from tests import _golden as G
    return int(np.count_nonzero(G.canon(np.atleast_1d(a)).view(np.int64) != G.canon(np.atleast_1d(b)).view(np.int64)))


def discrimination(oracle, call):
    """{flaw: (cells, shifts, words)} of a call of the hard table, the oracle's answer under each of BD.FLAWS against the canonical
    one: how many right-hand-side cells (column 0) of the start tableaux differ, for how many LPs shift_sum(c, lb) differs, and how
    many words of x and of the objective differ."""
    refs = hard_answers(oracle, call)
    out = {}
    for flaw in BD.FLAWS:
        bad = hard_answers(oracle, call, flaw)
        col0 = lambda r: r["start"].reshape(call.h, call.w)[:, 0]
        cells = sum(differing(col0(a), col0(b)) for a, b in zip(refs, bad))
        shifts = sum(differing(BD.shift_sum(lp[0], lb), BD.shift_sum_as(lp[0], lb, flaw)) for lp, lb in zip(call.lps, call.lbs)) if call.has_lb else 0
        answer = sum(differing(a["x"], b["x"]) + differing(a["objective"], b["objective"]) for a, b in zip(refs, bad))
        out[flaw] = (cells, shifts, answer)
    return out


def hard_views(torch, call):
    """The n = 129 call's operands as views: A_ub and A_eq transposed (a column stride that is not 1), lb every other element of a
    wider tensor; (views, copies), each (c, A_ub, b_ub, A_eq, b_eq, lb, ub)."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c, A_ub, b_ub, A_eq, b_eq = call.stacked()
    lb, ub = call.bounds_stacked()
    B, n = lb.shape
    A_ub_t, A_eq_t = dev(A_ub.transpose(0, 2, 1)), dev(A_eq.transpose(0, 2, 1))
    lb_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda")
    lb_wide[:, ::2] = dev(lb)
    views = (dev(c), A_ub_t.transpose(1, 2), dev(b_ub), A_eq_t.transpose(1, 2), dev(b_eq), lb_wide[:, ::2], dev(ub))
    assert views[1].stride()[1:] == (1, call.m_ub) and views[3].stride()[1:] == (1, call.m_eq) and views[5].stride() == (2 * n, 2)
    copies = tuple(dev(a) for a in (c, A_ub, b_ub, A_eq, b_eq, lb, ub))
    return views, copies


# ------------------------------------------------------------------------------------------------ the children

def _device(torch, call):
    from yalps_amd import tensors
    ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
    bnd = [None if a is None else torch.from_numpy(a).cuda() for a in call.bounds_stacked()]
    operands = tuple(tensors._strides(t, True, k in (1, 3)) for k, t in enumerate(ops))
    bounds = [None if t is None else (tensors._strides(t, True, False) or (None, 0, 0, 0)) for t in bnd]
    return ops, bnd, operands, bounds


def run_call(torch, handle, call, want=OUTPUTS):
    """One BCall through LpDense.solve with kept tableaux, all outputs pre-filled with SENTINEL, the pointers of `want` passed."""
    B, n = len(call.lps), call.n
    ops, bnd, operands, bounds = _device(torch, call)
    full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    x, objective = full((B, n), torch.float64), full((B,), torch.float64)
    status, pivots = full((B,), torch.int32), full((B,), torch.int64)
    marg = dict(ineqlin=full((B, call.m_ub), torch.float64), eqlin=full((B, call.m_eq), torch.float64), reduced=full((B, n), torch.float64),
                upper=full((B, call.k), torch.float64))
    ptr = lambda t: t.data_ptr() if t.numel() else None
    handle.solve(B, n, call.m_ub, call.m_eq, operands, maximize=call.maximize, precision=call.precision, max_pivots=call.max_pivots,
                 check_cycles=call.check, keep_tableaux=True, x=ptr(x), objective=ptr(objective), status=ptr(status), pivots=ptr(pivots),
                 lb=bounds[0], ub=bounds[1], upper=call.idx, **{("upper_out" if k == "upper" else k): ptr(marg[k]) for k in want})
    sols = [handle.solution(i) for i in range(B)]
    info = handle.info()
    after = [None if t is None else t.cpu().numpy() for t in ops + bnd]
    unchanged = all(a is None or LB.same_words(a, b, canonical_nan=False) for a, b in zip(after, call.stacked() + list(call.bounds_stacked())))
    out = dict(x=x.cpu().numpy(), objective=objective.cpu().numpy(), status=status.cpu().numpy(), pivots=pivots.cpu().numpy(),
               col0=np.stack([s[0] for s in sols]), pos=np.stack([s[1] for s in sols]), var=np.stack([s[2] for s in sols]),
               tableau=np.stack([handle.tableau(i) for i in range(B)]), launches=np.int64(info["launches"]), reruns=np.int64(info["reruns"]),
               kernels=np.array(" ".join(k["kernel"] for k in info["kernels"])), classes=np.array([k["class"] for k in info["kernels"]], np.int64),
               aux=np.array([k["aux"] for k in info["kernels"]], np.int64), grids=np.array([k["grid"] for k in info["kernels"]], np.int64),
               unchanged=np.bool_(unchanged))
    out.update({k: t.cpu().numpy() for k, t in marg.items()})
    return out


def answer(out):
    """A LinprogBatch / LinprogDuals / LinprogBoundDuals as numpy arrays."""
    return {("reduced" if k == "reduced_costs" else k): t.detach().cpu().numpy() for k, t in zip(out._fields, out)}


def views_inputs():
    """B = 6, n = 5, m_ub = 4, m_eq = 2 with per-LP bounds (the views test) and with shared ones (the stride-0 test)."""
    rng = np.random.default_rng(20261105)
    call = random_call("views", 6, 5, 4, 2, upper=(1, 3, 4))
    lb, ub = random_bounds(rng, 5, "both")
    shared = BCall("shared", [(*lp, lb, ub) for lp in call.lps], upper=(1, 3, 4))
    return call, shared


def plumbing(torch, out):
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def put(tag, d):
        out.update({"%s/%s" % (tag, k): v for k, v in d.items()})

    # no bounds: the bits and the kernels of yalps_lpdense_solve_duals
    call = partial_call()
    ops = [dev(a) for a in call.stacked()]
    stats = {}
    plain = tensors.linprog_batch(*ops, duals=True, stats=stats)
    out["plain/type"] = np.array(type(plain).__name__)
    put("plain", answer(plain))
    out["plain/kernels"] = np.array(" ".join(k["kernel"] for k in stats["kernels"]))
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    B, n = len(call.lps), call.n
    bufs = dict(x=(B, n), objective=(B,), ineqlin=(B, call.m_ub), eqlin=(B, call.m_eq), reduced=(B, n))
    bufs = {k: torch.full(s, SENTINEL, dtype=torch.float64, device="cuda") for k, s in bufs.items()}
    status, pivots = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    operands = tuple(tensors._strides(t, True, k in (1, 3)) for k, t in enumerate(ops))
    L = nat.lpdense_lib()
    import ctypes as C
    descs = nat._dense_operands(operands)
    ms = C.c_float()
    nat.lpdense_check(L.yalps_lpdense_solve_duals(handle.handle, B, n, call.m_ub, call.m_eq, *(C.byref(o) for o in descs), 0, 1e-8, 8192.0, 0, 0,
                                                  bufs["x"].data_ptr(), bufs["objective"].data_ptr(), status.data_ptr(), pivots.data_ptr(),
                                                  bufs["ineqlin"].data_ptr(), bufs["eqlin"].data_ptr(), bufs["reduced"].data_ptr(), C.byref(ms)))
    put("plain abi", dict({k: t.cpu().numpy() for k, t in bufs.items()}, status=status.cpu().numpy(), pivots=pivots.cpu().numpy()))
    out["plain abi/kernels"] = np.array(" ".join(k["kernel"] for k in handle.info()["kernels"]))

    # refusals: a host pointer for lb, ub or upper_out, by name, nothing launched, nothing written
    call = random_call("refusal", 3, 2, 2, 1)
    _, bnd, operands, bounds = _device(torch, call)
    host = np.zeros((3, 2))
    hostop = (host.ctypes.data, 2, 1, 0)
    up = torch.full((3, 2), SENTINEL, dtype=torch.float64, device="cuda")
    messages = []
    for name in ("lb", "ub", "upper_out"):
        kw = dict(lb=bounds[0], ub=bounds[1], upper=call.idx, upper_out=up.data_ptr())
        kw[name] = host.ctypes.data if name == "upper_out" else hostop
        try:
            handle.solve(3, 2, 2, 1, operands, **kw)
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    out["refusal/messages"] = np.array(messages)
    out["refusal/untouched"] = np.bool_(bool((up == SENTINEL).all().item()) and not host.any())
    put("refusal/after", run_call(torch, handle, call))
    handle.close()

    # shared bounds: [n] tensors (a batch stride of 0) against [B, n] copies
    call, shared = views_inputs()
    ops = [dev(a) for a in shared.stacked()]
    lb, ub = (dev(a) for a in shared.bounds_stacked())
    put("shared", answer(tensors.linprog_batch(*ops, lb=lb[0].clone(), ub=ub[0].clone(), upper=shared.upper, duals=True)))
    put("shared copies", answer(tensors.linprog_batch(*ops, lb=lb, ub=ub, upper=shared.upper, duals=True)))

    # views: lb every other element of a wider tensor, ub a transposed slice behind a storage offset
    ops = [dev(a) for a in call.stacked()]
    lb, ub = call.bounds_stacked()
    B, n = lb.shape
    lb_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda")
    lb_wide[:, ::2] = dev(lb)
    ub_t = torch.full((n + 2, B + 1), -9.0, dtype=torch.float64, device="cuda")
    ub_t[2:, 1:] = dev(ub.T)
    views = (lb_wide[:, ::2], ub_t[2:, 1:].t())
    assert views[0].stride() == (2 * n, 2) and views[1].stride() == (1, B + 1) and views[1].storage_offset() == 2 * (B + 1) + 1
    put("views", answer(tensors.linprog_batch(*ops, lb=views[0], ub=views[1], upper=call.upper, duals=True)))
    put("views copies", answer(tensors.linprog_batch(*ops, lb=dev(lb), ub=dev(ub), upper=call.upper, duals=True)))
    out["views/unchanged"] = np.bool_(bool((lb_wide[:, 1::2] == -9.0).all().item()) and bool((ub_t[:2] == -9.0).all().item()))

    # the producer of lb on a side stream, directly before the call on that stream
    side = torch.cuda.Stream()
    half = dev(lb) * 0.5
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big @ big * 2.0 ** -11  # (work in front of the producer: every entry stays 1.0)
        made = half * 2.0 + big[:B, :n] - 1.0
        put("stream", answer(tensors.linprog_batch(*ops, lb=made, ub=dev(ub), upper=call.upper, duals=True)))
    out["stream/lb"] = made.cpu().numpy()
    del side

    # B = 0
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    stats = {}
    empty = tensors.linprog_batch(z(0, 3), z(0, 2, 3), z(0, 2), lb=z(0, 3), ub=z(3), upper=(0, 2), duals=True, stats=stats)
    out["empty/shapes"] = np.array([d for t in empty for d in t.shape], np.int64)
    out["empty/type"] = np.array(type(empty).__name__)
    out["empty/launches"] = np.int64(stats["launches"])

    # linprog_objective_bounds: every operand batched and requiring grad, one row infeasible; then ub shared
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_()
    call = gradient_call()
    ops = [None if a is None else leaf(a) for a in call.stacked()]
    lb, ub = (leaf(a) for a in call.bounds_stacked())
    objective, duals = tensors.linprog_objective_bounds(*ops, lb=lb, ub=ub, precision=call.precision)
    assert objective.grad_fn is not None and not any(t.requires_grad for t in duals)
    objective.backward(torch.tensor(GRADIENT_WEIGHTS, dtype=torch.float64, device="cuda"))
    put("gradient rows", answer(duals))
    for name, t in zip(("c", "A_ub", "b_ub", "lb", "ub"), (ops[0], ops[1], ops[2], lb, ub)):
        out["gradient rows/grad_%s" % name] = t.grad.cpu().numpy()
    ops = [None if a is None else leaf(a) for a in call.stacked()]
    lb, ub = leaf(call.bounds_stacked()[0]), leaf(call.ubs[0])
    objective, duals = tensors.linprog_objective_bounds(*ops, lb=lb, ub=ub, upper=(0, 2), precision=call.precision)
    objective.backward(torch.tensor(GRADIENT_WEIGHTS, dtype=torch.float64, device="cuda"))
    put("gradient shared", answer(duals))
    out["gradient shared/grad_ub"], out["gradient shared/grad_lb"] = ub.grad.cpu().numpy(), lb.grad.cpu().numpy()
    call = difference_call()
    got = tensors.linprog_batch(*[None if a is None else dev(a) for a in call.stacked()], lb=dev(call.bounds_stacked()[0]),
                                ub=dev(call.bounds_stacked()[1]), precision=call.precision)
    put("differences", answer(got))


def child_table(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import _native as nat
    out = {}
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in table(_oracle.load()):
            out.update({"%s/%s" % (call.name, k): v for k, v in run_call(torch, handle, call).items()})
        for want in PARTIAL:
            out.update({"partial %s/%s" % ("+".join(want) or "none", k): v for k, v in run_call(torch, handle, partial_call(), want).items()})
    finally:
        handle.close()
    plumbing(torch, out)
    np.savez(path, **out)


def child_hist(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import os
    assert os.environ.get("YALPS_LPDENSE_HIST") == str(LD.HIST)
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import tensors
    call = hist_call(_oracle.load())
    stats = {}
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    lb, ub = call.bounds_stacked()
    out = answer(tensors.linprog_batch(*[dev(a) for a in call.stacked()], lb=dev(lb), ub=dev(ub), maximize=call.maximize, check_cycles=True,
                                       stats=stats, duals=True))
    out.update(reruns=np.int64(stats["reruns"]), passes=np.int64(1 + max(k["pass"] for k in stats["kernels"])),
               kernels=np.array(" ".join(k["kernel"] for k in stats["kernels"])))
    np.savez(path, **out)


def child_hard(path):
    """Every call of hard_table twice through _native.LpDense with kept tableaux -- with max_pivots = 0 ("<name> @0": the kept
    tableau is the start tableau) and with its own options -- then two of them through linprog_batch(duals=True), and the n = 129
    call through views."""
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    out = {}
    T = hard_table(_oracle.load())
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in T:
            for c in (at_budget_0(call), call):
                out.update({"%s/%s" % (c.name, k): v for k, v in run_call(torch, handle, c).items()})
    finally:
        handle.close()
    by_name = {c.name: c for c in T}
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for name in PUBLIC_HARD:
        call, stats = by_name[name], {}
        lb, ub = call.bounds_stacked()
        got = tensors.linprog_batch(*[dev(a) for a in call.stacked()], lb=dev(lb), ub=dev(ub), upper=call.upper, maximize=call.maximize,
                                    check_cycles=call.check, duals=True, stats=stats)
        out.update({"%s public/%s" % (name, k): v for k, v in answer(got).items()})
        out["%s public/kernels" % name] = np.array(" ".join(k["kernel"] for k in stats["kernels"]))
    call = by_name[VIEWS_HARD]
    views, copies = hard_views(torch, call)
    for tag, ops in (("hard views", views), ("hard views copies", copies)):
        got = tensors.linprog_batch(*ops[:5], lb=ops[5], ub=ops[6], upper=call.upper, maximize=call.maximize, duals=True)
        out.update({"%s/%s" % (tag, k): v for k, v in answer(got).items()})
    np.savez(path, **out)


if __name__ == "__main__":
    {"table": child_table, "hist": child_hist, "hard": child_hard}[sys.argv[1]](sys.argv[2])
