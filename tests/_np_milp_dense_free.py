"""Helpers of tests/test_milp_dense_free_model.py and tests/test_milp_dense_free.py (TEST INFRASTRUCTURE): milp_batch_free(free=)
restated in numpy and driven by the C oracle.  Nothing is restated twice: the split is tests/_np_dense_free.py's (FD: free_tableau,
equivalent_model, free_solution), the effective lower bound of the other variables, the bound rows and BCall are
tests/_np_milp_dense_bounds.py's (NB), the binary rows, the search and Call are tests/_np_milp_dense.py's (NM).  What is new here:

  free_set           `free`, or with True every variable that is not binary; naming a binary variable is refused (rule 3)
  effective_lower    NB.effective_lower with +0.0 at every free variable, integer or not: no ceil, lb is not read (rule 2)
  integer_columns    the n_int columns 1 + j in ascending j, then the twin columns of the free integer variables in ascending j
                     (rule 4)
  free_milp_tableau  FD.free_tableau with l_eff, then NM's binary rows widened by f zeros
  equivalent_model   FD.equivalent_model in x', "integers" naming the variables and the twins q<j> of the free integer ones
  FCall              NB.BCall with `free`: width 1 + n + f, hmax = h + 2 * n_int_eff
  expected           NM.expected on the split tableau, moved back by FD.free_solution
  FLAWS              the mutants, by name (WRONG on purpose): FCall.flawed takes them
Shares no code with the product.
"""
import copy
import math

import numpy as np

from tests import _np_dense as ND
from tests import _np_dense_free as FD
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB

# Wrong on purpose: what a kernel, or a host side, that misses one of the documented rules would compute.
#   "twin not integer"                 the twins of the free integer variables are left out of the integer columns: q is never branched on
#   "ceil at a free integer"           l_eff = ceil(lb[j]) at a free integer variable (a kind byte that wins over the twin)
#   "lb read at a free variable"       l_eff as if no variable were free: lb[j], ceil(lb[j]) at an integer one
#   "twins first in the integer list"  the twin columns in front of the columns 1 + j: a tie between a p and a q goes the other way
#   "binary row with a twin cell"      binary row q carries -1.0 in the column of twin q (a generated row told from a bound row by
#                                      its ordinal alone)
#   "hmax without the twins' cuts"     hmax = h + 2 * n_int: the expected ANSWER cannot change -- the oracle-driven search has no
#                                      slices -- but the size class of the tree kernel, which the GPU table compares by name, can
#   "sum of halves", "twin +inf"       FD's read-out flaws, applied to the best tableau
BUILD_FLAWS = ("twin not integer", "ceil at a free integer", "lb read at a free variable", "twins first in the integer list",
               "binary row with a twin cell", "hmax without the twins' cuts")
READ_FLAWS = ("sum of halves", "twin +inf")
FLAWS = BUILD_FLAWS + READ_FLAWS
SHAPE_ONLY = ("hmax without the twins' cuts",)


def free_set(n, free, bins):
    if free is True:
        return tuple(j for j in range(n) if j not in bins)
    fidx = FD.free_set(n, free)
    if set(fidx) & set(bins):
        raise ValueError("free names a binary variable")
    return fidx


def effective_lower(lb, n, ints, bins, fidx, flaw=None):
    low = NB.effective_lower(lb, n, ints, bins)
    if low is None or flaw == "lb read at a free variable":
        return low
    for j in fidx:
        if not (flaw == "ceil at a free integer" and j in ints):
            low[j] = 0.0
    return low


def integer_columns(n, ints, fidx, flaw=None):
    own = [j + 1 for j in ints]
    twins = [1 + n + t for t, j in enumerate(fidx) if j in ints]
    if flaw == "twin not integer":
        return own
    return twins + own if flaw == "twins first in the integer list" else own + twins


def free_milp_tableau(lp, lb=None, ub=None, upper=True, free=(), integers=(), binaries=(), maximize=False, flaw=None):
    """(flat row-major matrix, w, h, integer columns)"""
    assert flaw is None or flaw in FLAWS, flaw
    n, m_ub, m_eq = ND.shape_of(*lp)
    ints, bins = NM.sets_of(n, integers, binaries)
    idx = NB.bound_rows(n, upper, ub is not None, bins)
    fidx = free_set(n, free, bins)
    f, w = len(fidx), 1 + n + len(fidx)
    low = effective_lower(lb, n, ints, bins, fidx, flaw)
    # (FD zeroes lb at the free variables itself; its flaw "lb read" is how a low that is not zero there gets through)
    keep = "lb read" if flaw in ("ceil at a free integer", "lb read at a free variable") else None
    rows = FD.free_tableau(*lp, lb=low, ub=ub, upper=idx, free=fidx, maximize=maximize, flaw=keep)
    extra = np.zeros((len(bins), w), np.float64)
    for q, j in enumerate(bins):
        extra[q, 0] = extra[q, j + 1] = 1.0
        if flaw == "binary row with a twin cell" and q < f:
            extra[q, 1 + n + q] = -1.0
    return np.concatenate([rows, extra.ravel()]), w, 1 + m_ub + 2 * m_eq + len(idx) + len(bins), integer_columns(n, ints, fidx, flaw)


def equivalent_model(lp, lb=None, ub=None, upper=True, free=(), integers=(), binaries=(), maximize=False):
    n = len(lp[0])
    ints, bins = NM.sets_of(n, integers, binaries)
    idx = NB.bound_rows(n, upper, ub is not None, bins)
    fidx = free_set(n, free, bins)
    model = FD.equivalent_model(*lp, lb=effective_lower(lb, n, ints, bins, fidx), ub=ub, upper=idx, free=fidx, maximize=maximize)
    own = [j for j in ints if j not in bins]
    if own:
        model["integers"] = ["x%d" % j for j in own] + ["q%d" % j for j in fidx if j in own]
    if bins:
        model["binaries"] = ["x%d" % j for j in bins]
    return model


def explicit_milp_operands(lp, lb=None, ub=None, upper=True, free=(), integers=(), binaries=()):
    """The route a caller had: (the boundless operands in n + f variables, the integer variables with the twins, the row order
    that gives free_milp_tableau).  FD.explicit_operands appends the negated columns; its lb' and ub' then go through
    NB.explicit_milp_operands, which puts the unit rows under A_ub; the unit row of a free variable gets its -1.0 at the twin
    (p - q <= ub is no bound of the wider problem, it is a row with two coefficients)."""
    n = len(lp[0])
    ints, bins = NM.sets_of(n, integers, binaries)
    idx = NB.bound_rows(n, upper, ub is not None, bins)
    fidx = free_set(n, free, bins)
    low = effective_lower(lb, n, ints, bins, fidx)
    c, A_ub, b_ub, A_eq, b_eq, lb2, ub2, _ = FD.explicit_operands(*lp, lb=low, ub=ub, upper=idx, free=fidx)
    wide_ints = list(ints) + [n + t for t, j in enumerate(fidx) if j in ints]
    # (low is final: it goes in as a continuous lb, so NB's ceil must not touch it -- hence no integers in this inner call)
    ops, rows = NB.explicit_milp_operands((c, A_ub, b_ub, A_eq, b_eq), lb2, ub2, idx, (), ())
    m_ub, m_eq = ND.shape_of(*lp)[1:]
    for t, j in enumerate(idx):
        if j in fidx:
            ops[1][m_ub + t, n + fidx.index(j)] = -1.0
    first = 1 + m_ub + len(idx) + 2 * m_eq
    return ops, wide_ints, rows + list(range(first, first + len(bins)))


class FCall(NB.BCall):
    """NB.BCall with free variables: each MILP (c, A_ub, b_ub, A_eq, b_eq, lb, ub), lb / ub None for all or for none."""

    def __init__(self, name, lps, upper=True, free=(), flaw=None, **options):
        super().__init__(name, lps, upper, flaw=None, **options)
        self.free = free
        self.fidx = free_set(self.n, free, self.bins)
        self.f = len(self.fidx)
        self.int_twins = len(set(self.fidx) & set(self.ints))
        self.n_int_eff = len(self.ints) + self.int_twins
        self.w += self.f
        self.h_no_twins = self.hmax
        self.hmax += 2 * self.int_twins
        self.flaw = flaw

    def lows(self):
        return [effective_lower(lb, self.n, self.ints, self.bins, self.fidx, self.flaw) for lb in self.lbs]

    def tableau(self, i):
        return free_milp_tableau(self.lps[i], self.lbs[i], self.ubs[i], self.idx, self.fidx, self.integers, self.binaries, self.maximize,
                                 flaw=self.flaw)

    def models(self):
        return [equivalent_model(lp, lb, ub, self.idx, self.fidx, self.integers, self.binaries, self.maximize)
                for lp, lb, ub in zip(self.lps, self.lbs, self.ubs)]

    def flawed(self, flaw):
        """The call as a kernel, or a host side, with that flaw (one of FLAWS) would answer it: WRONG on purpose."""
        assert flaw in FLAWS, flaw
        out = copy.copy(self)
        out.flaw = flaw
        if flaw == "hmax without the twins' cuts":
            out.hmax = self.h_no_twins
        return out


def expected(nat, oracle, call, arena=None, arena_max=None):
    """NM.expected's rows of the search on the split tableau -- "x_split" (n + f values) and "objective_shifted" keep what it read
    -- with x and objective moved back by FD.free_solution: x[j] = v(p) - v(q) at a free variable, + l_eff, objective +
    shift_sum(c, l_eff)."""
    wide = copy.copy(call)
    wide.n = call.n + call.f  # (NM.expected reads solution() off a tableau of width n + 1)
    rows = NM.expected(nat, oracle, wide, arena=arena, arena_max=arena_max)
    sign = 1.0 if call.maximize else -1.0
    read = call.flaw if call.flaw in READ_FLAWS else ("lb read" if call.flaw in ("ceil at a free integer", "lb read at a free variable") else None)
    for row, lp, low in zip(rows, call.lps, call.lows()):
        status = row["status"]
        if status == "timedout":
            status = "optimal" if not math.isnan(row["result"]) else "infeasible"
        row["x_split"], row["objective_shifted"] = row["x"], row["objective"]
        row["x"], row["objective"] = FD.free_solution(row["col0"], row["pos"], row["var"], status, row["result"], sign, call.precision, lp[0],
                                                      lb=low, free=call.fidx, flaw=read)
        row["low"] = low
    return rows
