"""Helpers of tests/test_dense_queue_model.py and tests/test_dense_queue.py (TEST INFRASTRUCTURE): calls of linprog_batch's library
in which one workgroup takes several LPs, in every form of the three dense LP kernels, and the child processes that make them on
the GPU under YALPS_LPDENSE_CUS / _PER_CU (tests/_lp_dense.py says why children: torch first).  (milp_batch's root pass has the
same two hooks; tests/test_dense_queue.py runs tests/_milp_dense.py's `mix` child under them.)

A call holds ITEMS = 7 items of one shape that end differently, in an order in which each one's leftovers would show in the next:

  0  finite, "optimal"
  1  a NaN in b_ub; with bounds also cells of +-1.5e308 over lb = 1, so that one row's shift sum is +inf (under b_ub = +inf: the
     right-hand side is a NaN) and another's -inf (the right-hand side is +inf); it ends as the oracle says
  2  finite, "optimal", other data
  3  "infeasible": one right-hand side negated and scaled, x5 + x6 >= 1024 b[0], so that phase 1 pivots before it finds out
  4  "unbounded"; in the free family through a twin, so that x holds -inf
  5  "cycled" by the call's budget, which is 3 pivots less than this item needs (the items 0, 2, 3, 4, 6 end within it)
  6  finite, "optimal", other data

  lp_calls()      [QCall]: one call per (family, form), 3 x 10: the classes 1, 2, 3 just over the class bounds, the HBM form at
                  301 x 280 and the aux form at 8163 x 31, each without and with checkCycles.  A QCall is an LF.FCall (tests/_lp_dense_free.py):
                  the plain family has neither bounds nor free variables, the bounded one a box with `upper` a strict subset.
  LP_PICKS        the seven seeds and the budget of every data set, found once by `python -m tests._dense_queue pick`;
                  tests/test_dense_queue_model.py asserts with the oracle that they give the endings above
  answer_from     the oracle's answer from ANY start tableau and permutations: the canonical one, or what a stale workgroup
                  would have started from (STALE)
  child "lp"      every LP call through _native.LpDense with kept tableaux and all eight outputs, under the grid the test sets
                  (measured on one MI355X: the two grid children together 5.8 - 6.3 s with torch's start, the history child
                  2.7 - 2.9 s; the heaviest calls, the aux ones, 0.55 s each in the test: far from the minute at which the child
                  would have to be split by family)
  child "lphist"  the checkCycles calls once more under YALPS_LPDENSE_HIST=4
  child "unset"   two LPs of class 3 with no hook set
  milp_calls()    30 MILP calls, one per (family, form) again (see "the MILP calls" below); MILP_PICKS as LP_PICKS
  child "milp"    every MILP call through _native.MilpDense with a trace, under the hooks the test sets (measured: three such
                  children together 15.3 s, the heaviest call 0.87 s in the test)
  child "milphist"  the checkCycles MILP calls under YALPS_MILPDENSE_HIST=4 (5.3 s)
"""
import math
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _lp_dense as LD
from tests import _lp_dense_free as LF
from tests import _np_dense as ND
from tests import _np_dense_free as FD

INF = math.inf
ITEMS = 7
OPTIMAL, NONFINITE, INFEASIBLE, UNBOUNDED, CYCLED = (0, 2, 6), 1, 3, 4, 5
BUDGET_SHORT = 3              # the budget is this many pivots less than item CYCLED needs
HIST = 4                      # YALPS_LPDENSE_HIST of the child "lphist"
GRIDS = (1, 2)                # _CUS of the two runs of every call, with _PER_CU = 1
FAMILIES = ("plain", "bounded", "free")
LP_KERNEL = {"plain": "lp_dense_kernel", "bounded": "lp_dense_bounds_kernel", "free": "lp_dense_free_kernel"}
HUGE = 1.5e308
WORDS = ("x", "objective") + LF.OUTPUTS + ("col0", "matrix")  # the doubles a comparison looks at; with status, n_pivots, pos, var


def forms():
    """{form: (w, h, size class, aux)}: the smallest shapes of the project's tables that select each form above class 0."""
    shapes = LD.bound_shapes()
    out = {}
    for tag, j in (("c1", 1), ("c2", 3), ("c3", 5)):  # "over bound 0", "over bound 1", "over bound 2"
        k, w, h = shapes[j]
        out[tag] = (w, h, k + 1, 0)
    out["hbm"] = (280, 301, 4, 0)   # odd n, half-padded last unit
    m_ub, n = LD.AUX_SHAPE
    out["aux"] = (n + 1, m_ub + 1, 4, 1)
    for tag, (w, h, cls, aux) in out.items():
        assert (LB.size_class(w, h), int(BS.aux_hbm(w, h))) == (cls, aux if cls == 4 else 0), (tag, w, h)
    return out


def spelling(kernel, cls, check):
    return "%s<%d%s%s>" % (kernel, 1024 if cls >= 3 else 256, ",check" if check else "", ",lds" if cls < 4 else "")


# (family, form): (the seeds of the seven items, the call's max_pivots) -- `python -m tests._dense_queue pick` prints this table
LP_PICKS = {
    ("plain", "c1"): ((10, 3, 6, 7, 8, 1, 9), 33),
    ("plain", "c2"): ((8, 1, 6, 3, 5, 11, 7), 29),
    ("plain", "c3"): ((6, 3, 4, 8, 9, 2, 1), 103),
    ("plain", "hbm"): ((9, 8, 1, 2, 3, 10, 11), 364),
    ("plain", "aux"): ((3, 11, 7, 2, 9, 8, 10), 72),
    ("bounded", "c1"): ((8, 2, 3, 9, 10, 4, 5), 17),
    ("bounded", "c2"): ((5, 2, 6, 10, 7, 11, 1), 52),
    ("bounded", "c3"): ((9, 8, 2, 7, 10, 1, 5), 147),
    ("bounded", "hbm"): ((34, 20, 39, 37, 9, 35, 3), 555),   # (of the candidates 1 .. 40: most of this shape's LPs cycle for good)
    ("bounded", "aux"): ((5, 3, 7, 6, 11, 4, 10), 64),
    ("free", "c1"): ((5, 4, 9, 7, 10, 3, 11), 37),
    ("free", "c2"): ((10, 9, 11, 8, 4, 7, 6), 56),
    ("free", "c3"): ((1, 4, 3, 10, 9, 6, 5), 201),
    ("free", "hbm"): ((35, 15, 2, 9, 46, 29, 34), 566),       # (of 1 .. 40, likewise; item 4: the first seed above 40 that ends in time)
    ("free", "aux"): ((11, 10, 4, 9, 7, 2, 8), 81),
}


class QCall(LF.FCall):
    """An LF.FCall that remembers its family and form, and the oracle's canonical answers."""

    def __init__(self, family, form, check, lps, **options):
        w, h, cls, aux = forms()[form]
        super().__init__("%s %s%s" % (family, form, " check" if check else ""), lps, check=check, maximize=True, **options)
        assert (self.w, self.h) == (w, h), (self.name, self.w, self.h)
        self.family, self.form, self.cls, self.aux = family, form, cls, aux
        self.kernel = spelling(LP_KERNEL[family], cls, check)
        self._refs = {}

    def oracle_answer(self, oracle, i, flaw=None):
        if flaw is not None:
            return super().oracle_answer(oracle, i, flaw)
        if i not in self._refs:
            self._refs[i] = super().oracle_answer(oracle, i)
        return self._refs[i]


def layout(family, form):
    """(n, generator rows, m_ub, free, upper) of a family's LPs at a form's shape: one equality, so h = 1 + m_ub + 2 + k."""
    w, h = forms()[form][:2]
    f, k = (2, 2) if family == "free" else (0, 2) if family == "bounded" else (0, 0)
    n, m_ub = w - 1 - f, h - 3 - k
    free = (0, n - 1) if f else ()                       # each behind a guard row -x[j] <= GUARD, the last rows of A_ub
    upper = (0, 1) if family == "free" else (1, n - 2) if family == "bounded" else ()  # a strict subset; (0: a free variable)
    return n, m_ub - f, m_ub, free, upper


def base_lp(oracle, family, form, seed):
    """One finite LP of the oracle's generator (coefficients in [0, 1), right-hand sides of n / 4 and more, maximised): its last
    generated row is the equality, through the point x0 = lb + 1/8, which all inequalities admit; lb in eighths, a box of 1/4 .. 1."""
    n, gen, m_ub, free, upper = layout(family, form)
    c, A, b = ND.from_tableau(oracle.dense_lp(gen + 1, n, seed), n + 1, gen + 2)
    A_ub, b_ub, a_eq = A[:-1], b[:-1], A[-1:].copy()
    rng = np.random.default_rng([20270201, n, m_ub, seed])
    lb = rng.integers(-2, 2, n).astype(np.float64) / 8.0
    ub = lb + rng.integers(2, 9, n).astype(np.float64) / 8.0
    if family == "plain":
        lb, ub = None, None
    if free:
        guard = np.zeros((len(free), n))
        guard[np.arange(len(free)), list(free)] = -1.0
        A_ub, b_ub = np.vstack([A_ub, guard]), np.concatenate([b_ub, np.full(len(free), LF.GUARD)])
    x0 = (np.zeros(n) if lb is None else lb) + 0.125
    return [c.copy(), A_ub.copy(), b_ub.copy(), a_eq, a_eq @ x0, lb, ub]


def item_lp(oracle, family, form, item, seed):
    """Item `item` of a call: base_lp(seed), bent to its ending."""
    lp = base_lp(oracle, family, form, seed)
    c, A_ub, b_ub, a_eq, b_eq, lb, ub = lp
    n, gen, m_ub, free, upper = layout(family, form)
    if item == NONFINITE:
        b_ub[1] = math.nan
        if lb is not None:  # columns 3 and 4 are neither free nor listed in `upper`.  Row 2: inf - (+inf), a NaN that no ratio test
            A_ub[2, 3:5], A_ub[3, 3:5] = HUGE, -HUGE  # takes, where -inf would end the LP in front of its first pivot; row 3: +inf
            lb[3:5], ub[3:5] = 1.0, 2.0
            b_ub[2] = INF
    elif item == INFEASIBLE:  # row 0 as x5 + x6 >= 1024 b[0], which the other rows exclude: phase 1 pivots before it finds out
        A_ub[0], b_ub[0] = 0.0, -1024.0 * b_ub[0]
        A_ub[0, 5:7] = -1.0
    elif item == UNBOUNDED:
        x0 = (np.zeros(n) if lb is None else lb) + 0.125
        if free:  # the last variable is free: held from above now, wanted small, in no equality: its twin is unbounded
            j = free[-1]
            A_ub[:, j], c[j], a_eq[0, j] = 0.0, -64.0, 0.0  # (no row but its own: phase 1 cannot bring the twin in; phase 2 takes it first)
            A_ub[m_ub - 1, j] = 1.0
        else:     # variable 2 (not in `upper`): every row lets it grow
            A_ub[:, 2], a_eq[0, 2] = -A_ub[:, 2], 0.0
        lp[4] = a_eq @ x0
    return tuple(lp)


def lp_call(oracle, family, form, check, picks=None):
    seeds, budget = (picks or LP_PICKS)[family, form]
    n, gen, m_ub, free, upper = layout(family, form)
    lps = [item_lp(oracle, family, form, item, seed) for item, seed in enumerate(seeds)]
    return QCall(family, form, check, lps, upper=upper if upper else True, free=free, max_pivots=float(budget))


def lp_names():
    return ["%s %s%s" % (family, form, " check" if check else "") for family in FAMILIES for form in forms() for check in (False, True)]


def lp_calls(oracle):
    out = [lp_call(oracle, family, form, check) for family in FAMILIES for form in forms() for check in (False, True)]
    assert [c.name for c in out] == lp_names()
    return out


def lp_spellings():
    """The kernel spellings the LP calls are to run, over all calls: 3 families x 6 forms."""
    return {spelling(LP_KERNEL[family], cls, check) for family in FAMILIES for _, _, cls, _ in forms().values() for check in (False, True)}


# ------------------------------------------------------------------------------------------------ stale state
# What a workgroup that took item k + 1 after item k would start from if its fill left something of k behind (WRONG on purpose,
# the project's FLAWS practice): the oracle's answer from such a start must differ from the canonical one, or the call's data could
# not tell a kernel with that flaw from a right one.
#   "rhs"    column 0 of the rows 1 .. h - 1 not rewritten: k's final right-hand sides
#   "perm"   the permutations not reset: k's final positionOfVariable / variableAtPosition
#   "zeros"  the cells the fill GENERATES as +0.0 -- cell (0, 0), and the zeros of the bound rows -- not written: k's final cells
#            (In the plain family that is cell (0, 0) alone.  The padding columns of the pitch and the HBM / aux workspace behind
#            the tableau -- prow, colbuf -- are NOT modelled: the oracle's tableau has neither.  Only the GPU test's word-for-word
#            comparison of the kept matrix, column 0 and the marginals, which read row 0 of that workspace, can see those.)
STALE = ("rhs", "perm", "zeros")


def answer_from(oracle, call, i, start, pos, var):
    """call.oracle_answer(i)'s dict, from the flat start tableau and the permutations given (all three are left alone)."""
    m, pos, var = np.array(start, np.float64), np.array(pos, np.int32), np.array(var, np.int32)
    lp, lb = call.lps[i], call.lbs[i]
    status, result, npiv, _ = oracle.simplex(m, call.w, call.h, pos, var, precision=call.precision, max_pivots=call.max_pivots,
                                             check_cycles=call.check)
    col0 = m.reshape(call.h, call.w)[:, 0].copy()
    x, objective = FD.free_solution(col0, pos, var, status, result, 1.0, call.precision, lp[0], lb, call.fidx)
    marg = FD.free_marginals(m, pos, status, call.n, call.m_ub, call.m_eq, call.k, call.fidx, 1.0)
    return dict(status=status, result=result, n_pivots=npiv, matrix=m, start=np.array(start, np.float64), col0=col0, pos=pos, var=var, x=x,
                objective=objective, **dict(zip(LF.OUTPUTS, marg)))


def stale_start(call, prev, ref, flaw):
    """(start, pos, var) of an item whose canonical answer is `ref`, after an item that ended as `prev`, under `flaw`."""
    w, h = call.w, call.h
    start, left = ref["start"].reshape(h, w).copy(), prev["matrix"].reshape(h, w)
    identity = np.arange(w + h, dtype=np.int32)
    pos, var = identity, identity
    if flaw == "rhs":
        start[1:, 0] = left[1:, 0]
    elif flaw == "perm":
        pos, var = prev["pos"], prev["var"]
    else:
        assert flaw == "zeros", flaw
        start[0, 0] = left[0, 0]
        rows = slice(h - call.k, h)
        made = start[rows, 1:].view(np.int64) == 0  # (+0.0: the cells beside the 1.0 and the twin's -1.0)
        start[rows, 1:][made] = left[rows, 1:][made]
    return start.ravel(), pos, var


def words_differ(a, b):
    """How many of the compared words of two answers differ (all NaNs one value)."""
    n = int(a["status"] != b["status"]) + int(a["n_pivots"] != b["n_pivots"])
    n += int(np.count_nonzero(a["pos"] != b["pos"])) + int(np.count_nonzero(a["var"] != b["var"]))
    return n + sum(LF.differing(a[k], b[k]) for k in WORDS)


# ------------------------------------------------------------------------------------------------ picking the data

def pick(oracle, family, form, candidates=range(1, 12)):
    """(seeds, budget) for LP_PICKS: the candidate that needs most pivots becomes item CYCLED, the shortest ones the rest."""
    n, gen, m_ub, free, upper = layout(family, form)
    need = {}
    for seed in candidates:  # (a generated LP may cycle for good: 3000 pivots end the try, and the candidate is dropped)
        ref = lp_call(oracle, family, form, False, {(family, form): ((seed,) * ITEMS, 3000.0)}).oracle_answer(oracle, 0)
        if ref["status"] == "optimal":
            need[seed] = ref["n_pivots"]
    order = sorted(need, key=lambda s: (need[s], s))
    longest = order.pop()
    seeds = [None] * ITEMS
    seeds[CYCLED] = longest
    for item, seed in zip((0, 2, 6, NONFINITE, INFEASIBLE, UNBOUNDED), order):
        seeds[item] = seed
    return tuple(seeds), need[longest] - BUDGET_SHORT


# ------------------------------------------------------------------------------------------------ the MILP calls
# One call per (family, form) again: seven MILPs of one shape with an equality row and two integer variables (the last ones; in the
# free family the last one is free as well, so a twin is cut), from the families' own generators (tests/_milp_dense_bounds.py,
# tests/_milp_dense_free.py: data whose rounding shows), in queue order
#   0, 2, 4, 6  roots that branch          1  a root that is integral (its integer variables cost -1000: they stay at their bounds)
#   3  a root that is infeasible (its first row, which is positive, below -1e6)
#   5  a root that cycles by the call's budget, 3 pivots less than it needs
# MILP_PICKS: which of the generator's MILP_CANDIDATES each item is, and the budget -- `python -m tests._dense_queue pickmilp`.
MILP_ROOT = {"plain": "milp_dense_root_kernel", "bounded": "milp_dense_bounds_root_kernel", "free": "milp_dense_free_root_kernel"}
MILP_EPILOGUE = {"plain": "milp_dense_solution_kernel<256>", "bounded": "milp_dense_bounds_solution_kernel<256>",
                 "free": "milp_dense_free_solution_kernel<256>"}
MILP_CANDIDATES = 12
MILP_ITERATIONS = 8.0
BRANCH, INTEGRAL, M_INFEASIBLE, M_CYCLED = (0, 2, 4, 6), 1, 3, 5
MILP_PICKS = {
    ("plain", "c1"): ((4, 0, 10, 1, 9, 3, 11), 74),
    ("plain", "c2"): ((4, 0, 8, 3, 1, 2, 11), 118),
    ("plain", "c3"): ((3, 1, 0, 2, 9, 11, 6), 302),
    ("plain", "hbm"): ((11, 1, 5, 0, 8, 10, 2), 1586),
    ("plain", "aux"): ((7, 0, 9, 1, 3, 4, 10), 160),
    ("bounded", "c1"): ((9, 1, 3, 0, 2, 11, 4), 56),
    ("bounded", "c2"): ((1, 0, 8, 3, 6, 5, 2), 146),
    ("bounded", "c3"): ((7, 0, 8, 1, 9, 2, 3), 313),
    ("bounded", "hbm"): ((5, 0, 6, 1, 8, 2, 4), 1714),
    ("bounded", "aux"): ((8, 0, 5, 1, 10, 9, 3), 172),
    ("free", "c1"): ((9, 0, 5, 2, 1, 8, 6), 63),
    ("free", "c2"): ((6, 1, 3, 2, 10, 0, 4), 114),
    ("free", "c3"): ((3, 0, 4, 1, 7, 2, 5), 185),
    ("free", "hbm"): ((9, 0, 10, 2, 7, 8, 1), 1680),
    ("free", "aux"): ((6, 0, 8, 1, 10, 11, 4), 123),
}


def milp_candidates(family, form, check=False, max_pivots=8192.0, picks=None):
    """The family's call of MILP_CANDIDATES MILPs at the form's shape (picks None), or the seven of `picks`, bent to their endings."""
    from tests import _milp_dense_bounds as MDB
    from tests import _milp_dense_free as MF
    from tests import _np_milp_dense as NM
    w, h = forms()[form][:2]
    name = "milp %s %s%s" % (family, form, " check" if check else "")
    opts = dict(check=check, max_pivots=max_pivots, max_iterations=MILP_ITERATIONS)
    K = MILP_CANDIDATES
    f, k = (2, 2) if family == "free" else (0, 2) if family == "bounded" else (0, 0)
    n, gen = w - 1 - f, h - 1 - k - f   # (f guard rows under the generator's; no equality: with one most of these LPs cycle for good)
    ints, free = [n - 2, n - 1], [0, n - 2]
    lps = []
    for seed in range(1, K + 1):  # BS.packing's MILP, written densely
        (c, A, b, _, _), _ = NM.packing_dense(gen, n, 2, 100 * w + seed, 0.3 if forms()[form][3] else 0.6)
        rng = np.random.default_rng([20270302, w, h, seed])  # (MDB.boxed's box: lb in sixteenths, in quarters below zero at an integer variable)
        lb = rng.integers(0, 4, n).astype(np.float64) / 16.0
        lb[ints] = rng.integers(-7, 1, len(ints)).astype(np.float64) * 0.25
        ub = lb + 3.0 + rng.integers(0, 8, n) * 0.25
        A_ub, b_ub = A, b
        if f:  # (MF.mix_call's way: the free variables are wanted small and held by whole guards -x[j] <= 2)
            c = c.copy()
            c[free] *= -1.0
            guards = np.zeros((f, n))
            guards[np.arange(f), free] = -1.0
            A_ub, b_ub = np.concatenate([A_ub, guards]), np.concatenate([b_ub, np.full(f, 2.0)])
        lps.append((c, A_ub, b_ub, None, None, lb, ub))
    if family == "plain":
        make = lambda chosen: NM.Call(name, [lp[:5] for lp in chosen], integers=ints, maximize=True, **opts)
    elif family == "bounded":
        make = lambda chosen: MDB.NB.BCall(name, chosen, (0, 1), integers=ints, binaries=[], maximize=True, **opts)
    else:
        make = lambda chosen: MF.NF.FCall(name, chosen, (0, 1), free, integers=ints, binaries=[], maximize=True, **opts)
    if picks is None:
        return make(lps), lps, ints
    chosen = []
    for item, k in enumerate(picks):
        lp = [None if a is None else np.array(a, np.float64) for a in lps[k]]
        if item == INTEGRAL:
            lp[0][ints] = -1000.0
        elif item == M_INFEASIBLE:
            lp[2][0] = -1e6
        chosen.append(tuple(lp))
    call = make(chosen)
    call.family, call.form, call.cls, call.aux = family, form, forms()[form][2], forms()[form][3]
    assert (call.w, call.h) == (w, h) and len(call.ints) == 2, (name, call.w, call.h)
    tree = LB.size_class(call.w, call.hmax)
    call.root_kernel, call.tree_kernel = spelling(MILP_ROOT[family], call.cls, check), spelling("milp_tree_kernel", tree, check)
    call.tree_cls = tree
    return call


def milp_call(family, form, check, table=None):
    picks, budget = (table or MILP_PICKS)[family, form]
    return milp_candidates(family, form, check, float(budget), picks)


def milp_names():
    return ["milp %s %s%s" % (family, form, " check" if check else "") for family in FAMILIES for form in forms() for check in (False, True)]


def milp_calls():
    out = [milp_call(family, form, check) for family in FAMILIES for form in forms() for check in (False, True)]
    assert [c.name for c in out] == milp_names()
    return out


def milp_model(family):
    import importlib
    return importlib.import_module("tests." + {"plain": "_np_milp_dense", "bounded": "_np_milp_dense_bounds", "free": "_np_milp_dense_free"}[family])


_ROWS = {}


def milp_rows(nat, oracle, call):
    """The oracle-driven search's rows of a MILP call (the family's `expected`), computed once per process."""
    if call.name not in _ROWS:
        _ROWS[call.name] = milp_model(call.family).expected(nat, oracle, call)
    return _ROWS[call.name]


def milp_spellings():
    roots = {spelling(MILP_ROOT[f], cls, check) for f in FAMILIES for _, _, cls, _ in forms().values() for check in (False, True)}
    trees = {spelling("milp_tree_kernel", cls, check) for _, _, cls, _ in forms().values() for check in (False, True)}
    return roots, trees


def pick_milp(nat, oracle, family, form):
    """(the seven candidates, the budget): the branching candidate whose root needs most pivots becomes item M_CYCLED, the four
    shortest branching ones the items BRANCH; the first of the rest whose bent root is integral within the budget item INTEGRAL."""
    call, lps, ints = milp_candidates(family, form)
    expected = milp_model(family).expected
    rows = expected(nat, oracle, call)
    branch = [k for k, r in enumerate(rows) if r["nodes"] > 0 and r["root_pivots"] > 0]
    longest = max(branch, key=lambda k: (rows[k]["root_pivots"], -k))
    budget = rows[longest]["root_pivots"] - BUDGET_SHORT
    short = sorted((k for k in branch if k != longest and rows[k]["root_pivots"] <= budget), key=lambda k: (rows[k]["root_pivots"], k))[:4]
    rest = [k for k in range(len(lps)) if k not in short and k != longest]
    assert len(short) == 4 and len(rest) >= 2, (family, form, len(short), len(rest))
    for a in rest:
        picks = [None] * ITEMS
        for item, k in zip(BRANCH, short):
            picks[item] = k
        picks[M_CYCLED], picks[INTEGRAL], picks[M_INFEASIBLE] = longest, a, next(k for k in rest if k != a)
        got = expected(nat, oracle, milp_candidates(family, form, False, float(budget), picks))
        if got[INTEGRAL]["status"] == "optimal" and got[INTEGRAL]["nodes"] == 0:
            return tuple(picks), budget
    raise AssertionError((family, form, "no candidate gives an integral root"))


# ------------------------------------------------------------------------------------------------ the children

def _launch_info(info, items="lps"):
    K = info["kernels"]
    return dict(q_kernels=np.array(" ".join(k["kernel"] for k in K)), q_items=np.array([k.get(items, k.get("trees", -1)) for k in K], np.int64),
                q_grids=np.array([k["grid"] for k in K], np.int64), q_passes=np.array([k["pass"] for k in K], np.int64),
                q_hist_caps=np.array([k["hist_cap"] for k in K], np.int64), q_classes=np.array([k["class"] for k in K], np.int64),
                q_aux=np.array([k.get("aux", 0) for k in K], np.int64), q_reruns=np.int64(info["reruns"]),
                q_rerun_ids=np.array(info.get("rerun_lps", []), np.int64), q_rerun_trees=np.array(info.get("rerun_trees", []), np.int64))


def _torch_first():
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    return torch


def child_lp(path, only_check=False):
    torch = _torch_first()
    from tests import _oracle
    from yalps_amd import _native as nat
    out = {}
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in lp_calls(_oracle.load()):
            if only_check and not call.check:
                continue
            got = LF.run_call(torch, handle, call)
            got.update(_launch_info(handle.info()))
            out.update({"%s/%s" % (call.name, k): v for k, v in got.items()})
    finally:
        handle.close()
    np.savez(path, **out)


def child_lphist(path):
    import os
    assert os.environ.get("YALPS_LPDENSE_HIST") == str(HIST)
    child_lp(path, only_check=True)


def child_unset(path):
    """No hook set: a B = 2 call of class 3 runs on a grid of 2."""
    torch = _torch_first()
    from tests import _oracle
    from yalps_amd import _native as nat
    call = lp_call(_oracle.load(), "plain", "c3", False)
    call.lps, call.lbs, call.ubs = call.lps[:2], call.lbs[:2], call.ubs[:2]
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        got = LF.run_call(torch, handle, call)
        got.update(_launch_info(handle.info()))
    finally:
        handle.close()
    np.savez(path, **got)


def child_milp(path, only_check=False):
    """Every MILP call through _native.MilpDense with a trace (the families' own run_call), under the hooks the test sets."""
    torch = _torch_first()
    from tests import _milp_dense as MD
    from tests import _milp_dense_bounds as MDB
    from tests import _milp_dense_free as MF
    from yalps_amd import _native as nat
    run = {"plain": MD.run_call, "bounded": MDB.run_call, "free": MF.run_call}
    out = {}
    handle = nat.MilpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in milp_calls():
            if only_check and not call.check:
                continue
            got = run[call.family](torch, handle, call)
            got.update(_launch_info(handle.info()))
            out.update({"%s/%s" % (call.name, k): v for k, v in got.items()})
    finally:
        handle.close()
    np.savez(path, **out)


def child_milphist(path):
    import os
    assert os.environ.get("YALPS_MILPDENSE_HIST") == str(HIST)
    child_milp(path, only_check=True)


def _print_picks():
    from tests import _oracle
    oracle = _oracle.load()
    for family in FAMILIES:
        for form in forms():
            print("    (%r, %r): %r," % (family, form, pick(oracle, family, form)), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "pick":
        _print_picks()
    elif sys.argv[1] == "pickmilp":
        from tests import _oracle
        from yalps_amd import _native
        for family in FAMILIES:
            for form in forms():
                print("    (%r, %r): %r," % (family, form, pick_milp(_native, _oracle.load(), family, form)), flush=True)
    else:
        {"lp": child_lp, "lphist": child_lphist, "unset": child_unset, "milp": child_milp, "milphist": child_milphist}[sys.argv[1]](sys.argv[2])
