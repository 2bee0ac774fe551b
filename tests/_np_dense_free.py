"""Helpers of tests/test_lp_dense_free_model.py and tests/test_lp_dense_free.py (TEST INFRASTRUCTURE): the free variables of
linprog_batch(free=) restated in plain numpy, beside tests/_np_dense.py and tests/_np_dense_bounds.py, whose restatements of the
boundless and of the bounded call they extend.

  free_set           `free` (True: all n; (), False, None: none; else 0-based indices) as the ascending tuple of the call
  effective_lower    l_eff: lb with +0.0 at every free variable, where lb is not read (None without lb)
  free_tableau       what DenseFreeJob::fill writes: bounded_tableau with l_eff for lb, then one twin column per free variable
                     behind the n originals, ascending: the IEEE negation of the variable's own cell in every operand row, -1.0 in
                     the variable's bound row, +0.0 in every other bound row
  explicit_operands  the route a caller had: every operand with the negated columns appended, lb and ub extended by +0.0 / nothing
  equivalent_model   the bounded model in x', plus q<j> per free variable behind all x<j>: the negated coefficient of every
                     constraint x<j> lists, and -c[j]
  free_solution      what DenseFreeJob::after writes: x[j] = v(p) - v(q), each v dense_solution's rule on its own column, then
                     + l_eff[j] where lb is given; objective = objective' + shift_sum(c, l_eff)
  free_marginals     (ineqlin, eqlin, reduced, upper): the rows' formulas with w = 1 + n + f; reduced[j] of a free variable
                     s * (cost_nb(1 + j) - cost_nb(twin)) + 0.0
  identity_residuals how far an optimal answer is from
                         reduced = c - A_ub^T ineqlin - A_eq^T eqlin - scatter(upper)
                         objective = ineqlin . b_ub + eqlin . b_eq + upper . ub + reduced . l_eff
  FLAWS              the mutants, by name (WRONG on purpose): free_tableau(flaw=), free_solution(flaw=) and free_marginals(flaw=)
                     take them
Shares no code with the product.
"""
import math

import numpy as np

from tests import _np_dense as ND
from tests import _np_dense_bounds as BD
from tests import _np_dense_duals as DD

NAN = float("nan")

# Wrong on purpose (TEST INFRASTRUCTURE, as tests/_np_dense_bounds.py's FLAWS): what a kernel that misses the documented build, or the
# documented read-out, would compute.
#   "second product"          row 0 of a twin as (-1) * sign * c[j], a second product, where the canonical cell is the negation of
#                             the cell sign * c[j].  IEEE multiplication by -1 IS the negation of every value that is not a NaN,
#                             and of a NaN it may keep the sign the negation flips -- which no comparison here looks at (all NaNs
#                             count as one value).  So this mutant has the canonical words on every call: UNTELLABLE, and the
#                             model test asserts exactly that.
#   "both equality rows"      the twin holds -A_eq[k, j] in both rows of an equality pair (the second row is not negated back)
#   "positive zero"           a twin zero written as +0.0 where the negation gives -0.0
#   "lb read"                 lb read at a free variable: l_eff = lb everywhere
#   "sum over twins"          shift_sum over the n + f columns of the tableau, a twin taking part with the cell of the twin and the
#                             lb entry of its variable, read as it lies.  (With the twin's +0.0 in that place every added product
#                             is a zero and the sum keeps its bits whatever the order: that form cannot be told from the canonical
#                             one by any input, so the mutant is the one a column-blind kernel would be.)
#   "sum of halves"           x = v(p) + v(q)
#   "subtract first"          the subtraction made before the rounding: d = value(p) - value(q), x = round(d) where |d| > precision
#   "twin +inf"               an unbounded twin reported as +inf at its variable
#   "reduced without twin"    reduced[j] of a free variable by the formula of any other variable
#   "bound row without -1"    +0.0 in the twin's cell of the bound row of a free variable
BUILD_FLAWS = ("second product", "both equality rows", "positive zero", "lb read", "sum over twins", "bound row without -1")
READ_FLAWS = ("sum of halves", "subtract first", "twin +inf", "reduced without twin")
FLAWS = BUILD_FLAWS + READ_FLAWS
UNTELLABLE = ("second product",)


def free_set(n, free):
    if free is True:
        return tuple(range(n))
    if free is False or free is None:
        return ()
    idx = tuple(int(j) for j in free)
    if len(set(idx)) != len(idx) or any(not 0 <= j < n for j in idx):
        raise ValueError("free: duplicate or out-of-range index")
    return tuple(sorted(idx))


def effective_lower(lb, fidx, flaw=None):
    if lb is None:
        return None
    low = np.array(lb, np.float64)
    if flaw != "lb read":
        low[list(fidx)] = 0.0
    return low


def _shift(a, low, lb, fidx, flaw):
    """shift_sum(a, l_eff) over the n originals; under "sum over twins" over the n + f columns."""
    if flaw == "sum over twins":
        a = np.asarray(a, np.float64)
        return BD.shift_sum(np.concatenate([a, -a[list(fidx)]]), np.concatenate([low, np.asarray(lb, np.float64)[list(fidx)]]))
    return BD.shift_sum(a, low)


def free_tableau(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, lb=None, ub=None, upper=True, free=(), maximize=False, flaw=None):
    """The flat row-major (1 + m_ub + 2 m_eq + k) x (1 + n + f) matrix.  flaw: None, or one of FLAWS (a read-out flaw changes
    nothing here)."""
    assert flaw is None or flaw in FLAWS, flaw
    n, m_ub, m_eq = ND.shape_of(c, A_ub, b_ub, A_eq, b_eq)
    idx, fidx = BD.upper_set(n, upper, ub is not None), free_set(n, free)
    f, h0 = len(fidx), 1 + m_ub + 2 * m_eq
    low = effective_lower(lb, fidx, flaw)
    base = BD.bounded_tableau(c, A_ub, b_ub, A_eq, b_eq, lb=low, ub=ub, upper=idx, maximize=maximize).reshape(h0 + len(idx), n + 1)
    m = np.zeros((h0 + len(idx), 1 + n + f), np.float64)
    m[:, :n + 1] = base
    sign = np.float64(1.0 if maximize else -1.0)
    with np.errstate(all="ignore"):
        if flaw == "sum over twins" and lb is not None:
            for i in range(m_ub):
                m[1 + i, 0] = np.float64(b_ub[i]) - _shift(np.asarray(A_ub, np.float64).reshape(m_ub, n)[i], low, lb, fidx, flaw)
            for k in range(m_eq):
                v = np.float64(b_eq[k]) - _shift(np.asarray(A_eq, np.float64).reshape(m_eq, n)[k], low, lb, fidx, flaw)
                m[1 + m_ub + 2 * k, 0], m[2 + m_ub + 2 * k, 0] = v, -v
        for t, j in enumerate(fidx):
            col = -base[:h0, 1 + j]  # the negation of the cell, whatever the row made of the operand
            if flaw == "second product":
                col[0] = np.float64(-1.0) * sign * np.float64(c[j])
            if flaw == "both equality rows":
                for k in range(m_eq):
                    col[1 + m_ub + 2 * k] = col[2 + m_ub + 2 * k] = -np.float64(np.asarray(A_eq, np.float64).reshape(m_eq, n)[k, j])
            if flaw == "positive zero":
                col = col + 0.0
            m[:h0, 1 + n + t] = col
            if j in idx and flaw != "bound row without -1":
                m[h0 + idx.index(j), 1 + n + t] = -1.0
    return m.ravel()


def explicit_operands(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, lb=None, ub=None, upper=True, free=()):
    """(c', A_ub', b_ub, A_eq', b_eq, lb', ub', upper) of the bounded LP in n + f variables that a caller had to build: the negated
    columns of the free variables appended to c, A_ub and A_eq, lb extended by +0.0 (and +0.0 at the free variables themselves),
    ub by entries `upper` does not list.  Its bounded_tableau is free_tableau but for the -1.0 of a bound row of a free variable."""
    n, m_ub, m_eq = ND.shape_of(c, A_ub, b_ub, A_eq, b_eq)
    idx, fidx = BD.upper_set(n, upper, ub is not None), list(free_set(n, free))
    cat = lambda a: None if a is None else np.concatenate([np.asarray(a, np.float64).reshape(-1, n), -np.asarray(a, np.float64).reshape(-1, n)[:, fidx]], axis=1)
    low = effective_lower(lb, fidx)
    return (cat(c).ravel(), cat(A_ub), b_ub, cat(A_eq), b_eq, None if low is None else np.concatenate([low, np.zeros(len(fidx))]),
            None if ub is None else np.concatenate([np.asarray(ub, np.float64), np.zeros(len(fidx))]), idx)


def equivalent_model(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, lb=None, ub=None, upper=True, free=(), maximize=False):
    n, m_ub, m_eq = ND.shape_of(c, A_ub, b_ub, A_eq, b_eq)
    idx, fidx = BD.upper_set(n, upper, ub is not None), free_set(n, free)
    model = BD.equivalent_model(c, A_ub, b_ub, A_eq, b_eq, lb=effective_lower(lb, fidx), ub=ub, upper=idx, maximize=maximize)
    for j in fidx:
        model["variables"]["q%d" % j] = {key: -value for key, value in model["variables"]["x%d" % j].items()}
    return model


def _value(col0, pos, w, column, precision, raw=False):
    row = int(pos[column]) - w
    value = float(col0[row]) if row >= 0 else 0.0
    if raw:
        return value
    return ND.round_to_precision(value, precision) if value > precision else 0.0


def free_solution(col0, pos, var, status, result, sign, precision, c, lb=None, free=(), flaw=None):
    """(x[n], objective) of one LP from what simplex left on the (1 + n + f)-wide tableau.  flaw: None or one of FLAWS."""
    assert flaw is None or flaw in FLAWS, flaw
    n = len(c)
    fidx = free_set(n, free)
    f, w = len(fidx), 1 + n + len(fidx)
    twin = {j: 1 + n + t for t, j in enumerate(fidx)}
    low = effective_lower(lb, fidx, flaw)
    with np.errstate(all="ignore"):
        if status == "optimal":
            x = np.zeros(n, np.float64)
            for j in range(n):
                x[j] = _value(col0, pos, w, 1 + j, precision)
                if j in twin:
                    q = _value(col0, pos, w, twin[j], precision)
                    x[j] = np.float64(x[j]) + q if flaw == "sum of halves" else np.float64(x[j]) - q
                    if flaw == "subtract first":
                        d = float(np.float64(_value(col0, pos, w, 1 + j, precision, raw=True)) - np.float64(_value(col0, pos, w, twin[j], precision, raw=True)))
                        x[j] = ND.round_to_precision(d, precision) if abs(d) > precision else 0.0
            objective = -sign * result
        elif status == "unbounded":
            x = np.zeros(n, np.float64)
            v = int(var[int(result)])
            for j in range(n):
                p = np.float64(math.inf if v == 1 + j else 0.0)
                if j in twin:
                    q = np.float64(math.inf if v == twin[j] else 0.0)
                    p = p + q if flaw == "twin +inf" else p - q
                x[j] = p
            objective = sign * math.inf
        else:
            x, objective = np.full(n, NAN), NAN
        if low is not None:
            x = x + low
            objective = float(np.float64(objective) + _shift(c, low, lb, fidx, flaw))
    return x, objective


def free_marginals(matrix, pos, status, n, m_ub, m_eq, k, free, sign, flaw=None):
    """(ineqlin[m_ub], eqlin[m_eq], reduced[n], upper[k]) from the final (1 + m_ub + 2 m_eq + k) x (1 + n + f) matrix; NaN rows unless
    the LP ended optimal."""
    if status != "optimal":
        return tuple(np.full(s, NAN) for s in (m_ub, m_eq, n, k))
    fidx = free_set(n, free)
    w = 1 + n + len(fidx)
    row0, s = np.asarray(matrix, np.float64)[:w], np.float64(sign)

    def y(r):
        p = int(pos[w + r])
        return np.float64(-DD.cost(row0, p) if p < w else 0.0)

    def cost_nb(v):
        p = int(pos[v])
        return np.float64(DD.cost(row0, p) if p < w else 0.0)

    first = 1 + m_ub + 2 * m_eq
    with np.errstate(all="ignore"):
        ineqlin = np.array([s * y(1 + i) + 0.0 for i in range(m_ub)], np.float64)
        eqlin = np.array([s * (y(1 + m_ub + 2 * e) - y(2 + m_ub + 2 * e)) + 0.0 for e in range(m_eq)], np.float64)
        upper = np.array([s * y(first + t) + 0.0 for t in range(k)], np.float64)
        reduced = np.zeros(n, np.float64)
        for j in range(n):
            if j in fidx and flaw != "reduced without twin":
                reduced[j] = s * (cost_nb(1 + j) - cost_nb(1 + n + fidx.index(j))) + 0.0
            else:
                reduced[j] = s * cost_nb(1 + j) + 0.0
    return ineqlin, eqlin, reduced, upper


def identity_residuals(lp, lb, ub, idx, free, objective, ineqlin, eqlin, reduced, upper):
    """BD.identity_residuals with the effective lower bound in lb's place."""
    n = len(lp[0])
    return BD.identity_residuals(lp, effective_lower(lb, free_set(n, free)), ub, idx, objective, ineqlin, eqlin, reduced, upper)
