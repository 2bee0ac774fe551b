"""Helpers of tests/test_lp_dense_model.py and tests/test_lp_dense.py (TEST INFRASTRUCTURE): lp_dense_kernel's two new steps
restated in numpy, and the model a dense LP stands for.

  dense_tableau     what DenseJob::fill writes: tableauModel's initial matrix of the equivalent model, from c / A_ub / b_ub /
                    A_eq / b_eq of ONE LP
  dense_solution    what DenseJob::after writes: solution()'s answer (src/YALPS.ts:8-50) as a dense x and an objective
  equivalent_model  the model dict: constraints u0.. {"max"}, then e0.. {"equal"}, every variable listing every coefficient
  from_tableau      the other way round: a dense tableau whose cell (0, 0) is +0.0 as the operands of a maximising LP without
                    equalities (any table of tableaux written for the other batch kernels runs through the dense one that way)
"""
import math

import numpy as np

from yalps_amd.solve import round_to_precision

NAN = float("nan")


def shape_of(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None):
    """(n, m_ub, m_eq) of one LP's operands (None: no rows of that kind)."""
    return len(c), 0 if b_ub is None else len(b_ub), 0 if b_eq is None else len(b_eq)


def dense_tableau(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, maximize=False):
    """The flat row-major (1 + m_ub + 2 m_eq) x (n + 1) matrix: row 0 = +0.0, sign * c (a product); rows 1 + i = b_ub[i],
    A_ub[i]; rows 1 + m_ub + 2k and the next = b_eq[k], A_eq[k] and their negations."""
    n, m_ub, m_eq = shape_of(c, A_ub, b_ub, A_eq, b_eq)
    w, h = n + 1, 1 + m_ub + 2 * m_eq
    m = np.zeros((h, w), np.float64)
    m[0, 1:] = np.float64(1.0 if maximize else -1.0) * np.asarray(c, np.float64)
    if m_ub:
        m[1:1 + m_ub, 0] = b_ub
        m[1:1 + m_ub, 1:] = np.asarray(A_ub, np.float64).reshape(m_ub, n)
    if m_eq:
        A = np.asarray(A_eq, np.float64).reshape(m_eq, n)
        b = np.asarray(b_eq, np.float64)
        m[1 + m_ub::2, 0], m[1 + m_ub::2, 1:] = b, A
        m[2 + m_ub::2, 0], m[2 + m_ub::2, 1:] = -b, -A
    return m.ravel()


def dense_solution(col0, pos, var, status, result, sign, precision, n):
    """(x[n], objective) of one LP from what simplex left: column 0, both permutations, status and result."""
    w = n + 1
    if status == "optimal":
        x = np.zeros(n, np.float64)
        for j in range(n):
            row = int(pos[j + 1]) - w
            value = float(col0[row]) if row >= 0 else 0.0
            x[j] = round_to_precision(value, precision) if value > precision else 0.0
        return x, -sign * result
    if status == "unbounded":
        x = np.zeros(n, np.float64)
        v = int(var[int(result)]) - 1
        if 0 <= v < n:
            x[v] = math.inf
        return x, sign * math.inf
    return np.full(n, NAN), NAN


def equivalent_model(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, maximize=False):
    n, m_ub, m_eq = shape_of(c, A_ub, b_ub, A_eq, b_eq)
    constraints = {}
    for i in range(m_ub):
        constraints["u%d" % i] = {"max": float(b_ub[i])}
    for k in range(m_eq):
        constraints["e%d" % k] = {"equal": float(b_eq[k])}
    variables = {}
    for j in range(n):
        coefs = {"obj": float(c[j])}
        coefs.update(("u%d" % i, float(A_ub[i][j])) for i in range(m_ub))
        coefs.update(("e%d" % k, float(A_eq[k][j])) for k in range(m_eq))
        variables["x%d" % j] = coefs
    return {"direction": "maximize" if maximize else "minimize", "objective": "obj", "constraints": constraints, "variables": variables}


def from_tableau(matrix, w, h):
    """(c, A_ub, b_ub) of the maximising LP whose dense_tableau is `matrix` word for word (1.0 * v is v; a NaN stays a NaN)."""
    m = np.asarray(matrix, np.float64).reshape(h, w)
    assert m[0:1, 0].view(np.int64)[0] == 0, "cell (0, 0) must be +0.0"
    return m[0, 1:].copy(), (m[1:, 1:].copy() if h > 1 else None), (m[1:, 0].copy() if h > 1 else None)


def model_solution(sol, n):
    """solve()'s dict for the equivalent model (includeZeroVariables) as (status, x[n], objective)."""
    x = np.full(n, NAN) if sol["status"] in ("infeasible", "cycled") else np.zeros(n, np.float64)
    for key, value in sol["variables"]:
        x[int(key[1:])] = value
    return sol["status"], x, sol["result"]
