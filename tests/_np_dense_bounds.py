"""Helpers of tests/test_lp_dense_bounds_model.py and tests/test_lp_dense_bounds.py (TEST INFRASTRUCTURE): the bounds of
linprog_batch(lb=, ub=, upper=) restated in plain numpy, beside tests/_np_dense.py, whose restatement of the boundless call
they extend.

  shift_sum          sum of a[j] * l[j] in THE canonical order: every product rounded on its own; 64 partial sums p[k], each
                     starting from +0.0 and adding the products of the columns j = k (mod 64) in ascending j; then
                     p[k] += p[k + s] for k < s, s = 32, 16, 8, 4, 2, 1; the value is p[0].  It depends on nothing but a and l.
  shift_sum_lanes    the same order stated a second time, lane by lane; fma: a * b + c rounded once, in rationals
  flawed_shift_sum   WRONG on purpose, by the names of SUM_FLAWS; bounded_tableau(flaw=) and bounded_solution(flaw=) take those and
                     READ_FLAWS: the mutants the hard calls of tests/_lp_dense_bounds.py are shown to reject
  upper_set          `upper` (True: all n; else 0-based indices) as the ascending tuple of the call, refusing what the call refuses
  bounded_tableau    what DenseJob<true>::fill writes: dense_tableau with column 0 of every operand row moved by the row's
                     shift_sum with lb (one subtraction; none at all without lb), and below the equality rows one row per
                     listed variable, ascending: ub[j] - lb[j] (or ub[j]) in column 0, 1.0 in the variable's column, +0.0 elsewhere
  explicit_operands  the route a caller had: the unit rows stacked under A_ub, b shifted with shift_sum
  explicit_rows      the row order of explicit_operands' dense_tableau that gives bounded_tableau (the unit rows go last)
  equivalent_model   the model in x' = x - lb: u0.. {"max"}, e0.. {"equal"}, then h<j> {"max": ub[j] - lb[j]} in which variable j
                     alone has a coefficient, 1
  bounded_solution   what DenseJob<true>::after writes: dense_solution, then x = x' + lb and objective = objective' +
                     shift_sum(c, lb), one addition each, whatever the status
  bounded_marginals  (ineqlin, eqlin, reduced, upper): dense_marginals' formulas, `upper` being ineqlin's on the bound rows
  identity_residuals how far an optimal answer is from
                         reduced = c - A_ub^T ineqlin - A_eq^T eqlin - scatter(upper)
                         objective = ineqlin . b_ub + eqlin . b_eq + upper . ub + reduced . lb
Shares no code with the product.
"""
import math
from fractions import Fraction

import numpy as np

from tests import _np_dense as ND
from tests import _np_dense_duals as DD

NAN = float("nan")
LANES = 64


def shift_sum(a, l):
    a, l = np.asarray(a, np.float64).reshape(-1), np.asarray(l, np.float64).reshape(-1)
    assert a.size == l.size
    p = [np.float64(0.0)] * LANES
    with np.errstate(all="ignore"):
        for j in range(a.size):
            p[j % LANES] = p[j % LANES] + a[j] * l[j]
        s = LANES // 2
        while s:
            for k in range(s):
                p[k] = p[k] + p[k + s]
            s //= 2
    return np.float64(p[0])


def shift_sum_lanes(a, l):
    """THE order once more, sharing no line with shift_sum: lane k's list of columns k, k + 64, .. summed on its own, then the
    list of 64 halved until one value is left."""
    a, l = [float(v) for v in np.asarray(a, np.float64).reshape(-1)], [float(v) for v in np.asarray(l, np.float64).reshape(-1)]
    assert len(a) == len(l)
    with np.errstate(all="ignore"):
        v = []
        for k in range(LANES):
            p = np.float64(0.0)
            for j in range(k, len(a), LANES):
                p = p + np.float64(a[j]) * np.float64(l[j])
            v.append(p)
        while len(v) > 1:
            half = len(v) // 2
            v = [v[k] + v[k + half] for k in range(half)]
    return np.float64(v[0])


def fma(a, b, c):
    """a * b + c rounded once, in rationals (CPython's int / int is correctly rounded); IEEE's rules where they are not enough:
    anything that is not finite, an exact zero, an overflow."""
    a, b, c = float(a), float(b), float(c)
    with np.errstate(all="ignore"):
        if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
        if a == 0.0 or b == 0.0:
            return float(np.float64(a) * np.float64(b) + np.float64(c))  # (+-0 + c: exact, and the zero's sign is the addition's)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        return 0.0  # (two non-zero terms that cancel: +0.0 under round-to-nearest)
    try:
        return float(exact)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


# Wrong on purpose (TEST INFRASTRUCTURE, as tests/_sens_table.py's FLAWS): what a kernel that misses the documented order, or the
# documented read-out, would compute.  tests/test_lp_dense_bounds_model.py shows that the hard calls of tests/_lp_dense_bounds.py
# tell every one of them from the canonical statement.
SUM_FLAWS = ("left to right", "fused", "fold upward", "lanes of 32")
READ_FLAWS = ("round after add", "objective rounded last", "dot")
FLAWS = SUM_FLAWS + READ_FLAWS


def flawed_shift_sum(a, l, flaw):
    """shift_sum WRONG on purpose, by name:
      "left to right"  one running sum from +0.0 in ascending j
      "fused"          THE order with every p + a[j] * l[j] as one fused multiply-add (the product is not rounded on its own)
      "fold upward"    THE lanes folded by 1, 2, 4, .. 32 (p += shfl_down(p, s) in every lane at once)
      "lanes of 32"    32 partial sums over j = k (mod 32), folded by 16, .. 1"""
    assert flaw in SUM_FLAWS, flaw
    a, l = np.asarray(a, np.float64).reshape(-1), np.asarray(l, np.float64).reshape(-1)
    assert a.size == l.size
    with np.errstate(all="ignore"):
        if flaw == "left to right":
            s = np.float64(0.0)
            for j in range(a.size):
                s = s + a[j] * l[j]
            return np.float64(s)
        lanes = 32 if flaw == "lanes of 32" else LANES
        p = [np.float64(0.0)] * lanes
        for j in range(a.size):
            p[j % lanes] = np.float64(fma(a[j], l[j], p[j % lanes])) if flaw == "fused" else p[j % lanes] + a[j] * l[j]
        steps = [1 << t for t in range(lanes.bit_length() - 1)]
        for s in (steps if flaw == "fold upward" else steps[::-1]):
            p = [p[k] + p[k + s] if k + s < lanes else p[k] for k in range(lanes)]
    return np.float64(p[0])


def shift_sum_as(a, l, flaw=None):
    """shift_sum, or its flawed form where `flaw` names one of SUM_FLAWS (a read-out flaw leaves the sums alone)."""
    assert flaw is None or flaw in FLAWS, flaw
    return flawed_shift_sum(a, l, flaw) if flaw in SUM_FLAWS else shift_sum(a, l)


def upper_set(n, upper, has_ub=True):
    if upper is True:
        return tuple(range(n)) if has_ub else ()
    idx = tuple(int(j) for j in upper)
    if len(set(idx)) != len(idx) or any(not 0 <= j < n for j in idx):
        raise ValueError("upper: duplicate or out-of-range index")
    return tuple(sorted(idx))


def bounded_tableau(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, lb=None, ub=None, upper=True, maximize=False, flaw=None):
    """flaw: None, or one of FLAWS -- a sum flaw replaces every shift_sum, a read-out flaw changes nothing here."""
    n, m_ub, m_eq = ND.shape_of(c, A_ub, b_ub, A_eq, b_eq)
    idx = upper_set(n, upper, ub is not None)
    w, h0 = n + 1, 1 + m_ub + 2 * m_eq
    m = np.zeros((h0 + len(idx), w), np.float64)
    m[:h0] = ND.dense_tableau(c, A_ub, b_ub, A_eq, b_eq, maximize).reshape(h0, w)
    with np.errstate(all="ignore"):
        if lb is not None:
            for i in range(m_ub):
                m[1 + i, 0] = np.float64(b_ub[i]) - shift_sum_as(np.asarray(A_ub, np.float64).reshape(m_ub, n)[i], lb, flaw)
            for k in range(m_eq):
                v = np.float64(b_eq[k]) - shift_sum_as(np.asarray(A_eq, np.float64).reshape(m_eq, n)[k], lb, flaw)
                m[1 + m_ub + 2 * k, 0], m[2 + m_ub + 2 * k, 0] = v, -v
        for t, j in enumerate(idx):
            m[h0 + t, 0] = np.float64(ub[j]) - np.float64(lb[j]) if lb is not None else np.float64(ub[j])
            m[h0 + t, 1 + j] = 1.0
    return m.ravel()


def explicit_operands(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, lb=None, ub=None, upper=True):
    """(c, A_ub', b_ub', A_eq, b_eq') of the boundless LP in x' = x - lb that a caller had to build: len(upper) unit rows under
    A_ub, every right-hand side moved by shift_sum."""
    n, m_ub, m_eq = ND.shape_of(c, A_ub, b_ub, A_eq, b_eq)
    idx = upper_set(n, upper, ub is not None)
    A = np.zeros((m_ub + len(idx), n), np.float64)
    b = np.zeros(m_ub + len(idx), np.float64)
    with np.errstate(all="ignore"):
        for i in range(m_ub):
            A[i] = np.asarray(A_ub, np.float64).reshape(m_ub, n)[i]
            b[i] = np.float64(b_ub[i]) - shift_sum(A[i], lb) if lb is not None else b_ub[i]
        for t, j in enumerate(idx):
            A[m_ub + t, j] = 1.0
            b[m_ub + t] = np.float64(ub[j]) - np.float64(lb[j]) if lb is not None else ub[j]
        be = None
        if m_eq:
            Ae = np.asarray(A_eq, np.float64).reshape(m_eq, n)
            be = np.array([np.float64(b_eq[k]) - shift_sum(Ae[k], lb) if lb is not None else b_eq[k] for k in range(m_eq)], np.float64)
    rows = len(idx) + m_ub
    return np.asarray(c, np.float64), (A if rows else None), (b if rows else None), A_eq, be


def explicit_rows(m_ub, m_eq, k):
    """Row r of bounded_tableau is row explicit_rows(...)[r] of dense_tableau(*explicit_operands(...))."""
    return [0] + list(range(1, 1 + m_ub)) + list(range(1 + m_ub + k, 1 + m_ub + k + 2 * m_eq)) + list(range(1 + m_ub, 1 + m_ub + k))


def equivalent_model(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, lb=None, ub=None, upper=True, maximize=False):
    n, m_ub, m_eq = ND.shape_of(c, A_ub, b_ub, A_eq, b_eq)
    idx = upper_set(n, upper, ub is not None)
    ec, eA, eb, _, ebe = explicit_operands(c, A_ub, b_ub, A_eq, b_eq, lb, ub, upper)
    model = ND.equivalent_model(ec, None if not m_ub else eA[:m_ub], None if not m_ub else eb[:m_ub], A_eq, ebe, maximize)
    for t, j in enumerate(idx):
        model["constraints"]["h%d" % j] = {"max": float(eb[m_ub + t])}
        model["variables"]["x%d" % j]["h%d" % j] = 1.0
    return model


def bounded_solution(col0, pos, var, status, result, sign, precision, c, lb=None, flaw=None):
    """flaw: None, or one of FLAWS -- WRONG on purpose then: a sum flaw replaces shift_sum(c, lb);
      "round after add"         x[j] = roundToPrecision(value + lb[j]) where the reference rounds `value`
      "objective rounded last"  roundToPrecision(objective' + shift_sum(c, lb))
      "dot"                     the objective as np.dot(c, x) of the shifted x
    (the last three on "optimal" alone, and with lb: nothing is added without it)."""
    assert flaw is None or flaw in FLAWS, flaw
    n = len(c)
    x, objective = ND.dense_solution(col0, pos, var, status, result, sign, precision, n)
    if lb is not None:
        low = np.asarray(lb, np.float64)
        with np.errstate(all="ignore"):
            shifted = float(np.float64(objective) + shift_sum_as(c, lb, flaw))
            if flaw == "round after add" and status == "optimal":
                for j in range(n):
                    row = int(pos[j + 1]) - (n + 1)
                    value = np.float64(col0[row]) if row >= 0 else np.float64(0.0)
                    x[j] = ND.round_to_precision(float(value + low[j]), precision) if value > precision else 0.0 + low[j]
            else:
                x = x + low
            if flaw == "objective rounded last" and status == "optimal":
                shifted = ND.round_to_precision(shifted, precision)
            if flaw == "dot" and status == "optimal":
                shifted = float(np.dot(np.asarray(c, np.float64), x))
            objective = shifted
    return x, objective


def bounded_marginals(matrix, pos, status, n, m_ub, m_eq, k, sign):
    """(ineqlin[m_ub], eqlin[m_eq], reduced[n], upper[k]) from the final (1 + m_ub + 2 m_eq + k) x (n + 1) matrix; NaN rows unless
    the LP ended optimal."""
    if status != "optimal":
        return tuple(np.full(s, NAN) for s in (m_ub, m_eq, n, k))
    ineqlin, eqlin, reduced = DD.dense_marginals(matrix, pos, n, m_ub, m_eq, sign)
    w, first = n + 1, 1 + m_ub + 2 * m_eq
    row0, s = np.asarray(matrix, np.float64)[:w], np.float64(sign)
    upper = np.zeros(k, np.float64)
    for t in range(k):
        p = int(pos[w + first + t])
        upper[t] = s * np.float64(-DD.cost(row0, p) if p < w else 0.0) + 0.0
    return ineqlin, eqlin, reduced, upper


def identity_residuals(lp, lb, ub, idx, objective, ineqlin, eqlin, reduced, upper):
    """(|objective - (ineqlin . b_ub + eqlin . b_eq + upper . ub + reduced . lb)|,
    max |reduced - (c - A_ub^T ineqlin - A_eq^T eqlin - scatter(upper))|) of one optimal LP."""
    c, A_ub, b_ub, A_eq, b_eq = lp
    n, m_ub, m_eq = ND.shape_of(*lp)
    value, rc = 0.0, np.asarray(c, np.float64).copy()
    if m_ub:
        value += float(np.dot(ineqlin, b_ub))
        rc -= np.asarray(A_ub, np.float64).reshape(m_ub, n).T @ ineqlin
    if m_eq:
        value += float(np.dot(eqlin, b_eq))
        rc -= np.asarray(A_eq, np.float64).reshape(m_eq, n).T @ eqlin
    for t, j in enumerate(idx):
        value += float(upper[t] * ub[j])
        rc[j] -= upper[t]
    if lb is not None:
        value += float(np.dot(reduced, lb))
    return abs(objective - value), float(np.abs(reduced - rc).max()) if n else 0.0
