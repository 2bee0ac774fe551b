"""Helpers of tests/test_milp_dense_bounds_model.py and tests/test_milp_dense_bounds.py (TEST INFRASTRUCTURE): milp_batch(lb=,
ub=, upper=) restated in numpy and driven by the C oracle.  Nothing is restated twice: the bounded rows are
tests/_np_dense_bounds.py's (BD: shift_sum, bounded_tableau, equivalent_model, bounded_solution and the flaws), the binary rows,
the integer columns and the search are tests/_np_milp_dense.py's (NM: Call, expected).  What is new here is the three rules:

  effective_lower      l_eff: lb at a continuous variable, ceil(lb) at an integer one, +0.0 at a binary one (lb is not read there)
  bound_rows           the k variables with a bound row: `upper`, or with True every variable that is not binary; naming a binary
                       variable is refused
  bounded_milp_tableau BD.bounded_tableau with l_eff for lb, then NM's binary rows: linprog_batch's rows, the bound rows, the binary
                       rows
  equivalent_model     BD.equivalent_model in x' = x - l_eff, plus "integers" / "binaries"
  BCall                NM.Call with bounds: per MILP (c, A_ub, b_ub, A_eq, b_eq, lb, ub), one `upper` for the call
  expected             NM.expected on the bounded tableau, then x and objective moved back by BD.bounded_solution
Shares no code with the product.
"""
import copy
import math

import numpy as np

from tests import _np_dense as ND
from tests import _np_dense_bounds as BD
from tests import _np_milp_dense as NM


def effective_lower(lb, n, ints, bins):
    """ints: the ascending union of both sets (NM.sets_of)."""
    if lb is None:
        return None
    out = np.array(lb, np.float64).reshape(n)
    for j in ints:
        v = float(out[j])
        if math.isfinite(v):  # (NaN and the infinities pass through)
            up = float(math.ceil(v))
            out[j] = math.copysign(0.0, v) if up == 0.0 else up  # (IEEE ceil keeps the sign: ceil(-0.5) is -0.0; Python's gives 0)
    for j in bins:
        out[j] = 0.0
    return out


def bound_rows(n, upper, has_ub, bins):
    if upper is True:
        return tuple(j for j in range(n) if j not in bins) if has_ub else ()
    idx = BD.upper_set(n, upper, has_ub)
    if set(idx) & set(bins):
        raise ValueError("upper names a binary variable")
    return idx


def bounded_milp_tableau(lp, lb=None, ub=None, upper=True, integers=(), binaries=(), maximize=False, flaw=None):
    """(flat row-major matrix, w, h, integer columns)"""
    n, m_ub, m_eq = ND.shape_of(*lp)
    ints, bins = NM.sets_of(n, integers, binaries)
    idx = bound_rows(n, upper, ub is not None, bins)
    low = effective_lower(lb, n, ints, bins)
    rows = BD.bounded_tableau(*lp, lb=low, ub=ub, upper=idx, maximize=maximize, flaw=flaw)
    w = n + 1
    extra = np.zeros((len(bins), w), np.float64)
    for q, j in enumerate(bins):
        extra[q, 0] = extra[q, j + 1] = 1.0
    return np.concatenate([rows, extra.ravel()]), w, 1 + m_ub + 2 * m_eq + len(idx) + len(bins), [j + 1 for j in ints]


def equivalent_model(lp, lb=None, ub=None, upper=True, integers=(), binaries=(), maximize=False):
    n = len(lp[0])
    ints, bins = NM.sets_of(n, integers, binaries)
    idx = bound_rows(n, upper, ub is not None, bins)
    model = BD.equivalent_model(*lp, lb=effective_lower(lb, n, ints, bins), ub=ub, upper=idx, maximize=maximize)
    name = lambda given: True if given is True else ["x%d" % int(j) for j in given]
    if integers is True or len(integers):
        model["integers"] = name(integers)
    if binaries is True or len(binaries):
        model["binaries"] = name(binaries)
    return model


def explicit_milp_operands(lp, lb=None, ub=None, upper=True, integers=(), binaries=()):
    """The route a caller had: BD.explicit_operands with l_eff (unit rows under A_ub, every b shifted); and the row order of NM's
    tableau of those operands that gives bounded_milp_tableau: (operands, rows)."""
    n, m_ub, m_eq = ND.shape_of(*lp)
    ints, bins = NM.sets_of(n, integers, binaries)
    idx = bound_rows(n, upper, ub is not None, bins)
    ops = BD.explicit_operands(*lp, lb=effective_lower(lb, n, ints, bins), ub=ub, upper=idx)
    k = len(idx)
    first = 1 + m_ub + k + 2 * m_eq
    return ops, BD.explicit_rows(m_ub, m_eq, k) + list(range(first, first + len(bins)))


class BCall(NM.Call):
    """NM.Call whose MILPs carry bounds: each (c, A_ub, b_ub, A_eq, b_eq, lb, ub), lb / ub None for all or for none."""

    def __init__(self, name, lps, upper=True, flaw=None, **options):
        super().__init__(name, [tuple(lp[:5]) for lp in lps], **options)
        self.lbs, self.ubs = [lp[5] for lp in lps], [lp[6] for lp in lps]
        self.has_lb, self.has_ub = self.lbs[0] is not None, self.ubs[0] is not None
        assert all((a is not None) == self.has_lb for a in self.lbs) and all((a is not None) == self.has_ub for a in self.ubs)
        self.upper, self.flaw = upper, flaw
        self.exact = True  # (a generator of data whose rounding shows says otherwise)
        self.idx = bound_rows(self.n, upper, self.has_ub, self.bins)
        self.k = len(self.idx)
        self.h += self.k
        self.hmax += self.k

    def bounds_stacked(self):
        return (np.stack([np.asarray(a, np.float64) for a in self.lbs]) if self.has_lb else None,
                np.stack([np.asarray(a, np.float64) for a in self.ubs]) if self.has_ub else None)

    def lows(self):
        return [effective_lower(lb, self.n, self.ints, self.bins) for lb in self.lbs]

    def tableau(self, i):
        return bounded_milp_tableau(self.lps[i], self.lbs[i], self.ubs[i], self.idx, self.integers, self.binaries, self.maximize,
                                    flaw=self.flaw)

    def roots(self, oracle):
        sign = 1.0 if self.maximize else -1.0
        return [NM.DenseRoot(oracle, *self.tableau(i), sign, self.options) for i in range(len(self.lps))]

    def models(self):
        return [equivalent_model(lp, lb, ub, self.idx, self.integers, self.binaries, self.maximize)
                for lp, lb, ub in zip(self.lps, self.lbs, self.ubs)]

    def flawed(self, flaw):
        """The call as a kernel with that flaw (one of BD.FLAWS) would answer it: WRONG on purpose."""
        out = copy.copy(self)
        out.flaw = flaw
        return out


def expected(nat, oracle, call, arena=None, arena_max=None):
    """NM.expected's rows of the search in x'; x and objective moved back (x = x' + l_eff, objective = objective' +
    shift_sum(c, l_eff), one addition each whatever the status), x' and objective' kept as "x_shifted" / "objective_shifted"."""
    rows = NM.expected(nat, oracle, call, arena=arena, arena_max=arena_max)
    sign = 1.0 if call.maximize else -1.0
    for row, lp, low in zip(rows, call.lps, call.lows()):
        status = row["status"]
        if status == "timedout":
            status = "optimal" if not math.isnan(row["result"]) else "infeasible"
        row["x_shifted"], row["objective_shifted"] = row["x"], row["objective"]
        row["x"], row["objective"] = BD.bounded_solution(row["col0"], row["pos"], row["var"], status, row["result"], sign, call.precision,
                                                         lp[0], low, flaw=call.flaw)
        row["low"] = low
    return rows
