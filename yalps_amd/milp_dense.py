"""The host side of tensors.milp_batch (numpy only; nothing here imports torch or touches the GPU): the integer sets of a
call, and the fallback for trees that overflowed on the device -- tableauModel's tableau of one dense MILP (reference
src/tableau.ts:47-137), its cells as the lockstep driver (_native.MilpBatch) takes them, and solution() (src/YALPS.ts:8-50)
of a best tableau as a dense row."""
import math

import numpy as np

from . import _native
from .solve import round_to_precision

NAN = float("nan")


def integer_sets(n, integers=(), binaries=(), who="milp_batch"):
    """(integer list, binary list): ascending 0-based variable indices, the integer list the union of both sets (a variable
    named in both counts once).  `True` names all n variables.  Raises ValueError for a duplicate or an index outside
    0 .. n - 1."""
    sets = []
    for name, given in (("integers", integers), ("binaries", binaries)):
        if given is True:
            sets.append(list(range(n)))
            continue
        if given is False or given is None:
            given = ()
        if isinstance(given, (str, bytes)) or not hasattr(given, "__iter__"):
            raise TypeError("%s: %s must be a sequence of variable indices or True, not %r" % (who, name, given))
        idx = []
        for j in given:
            if isinstance(j, bool) or int(j) != j:
                raise TypeError("%s: %s holds %r; variable indices are integers" % (who, name, j))
            idx.append(int(j))
        bad = [j for j in idx if not 0 <= j < n]
        if bad:
            raise ValueError("%s: %s names variable %d, outside 0 .. %d" % (who, name, bad[0], n - 1))
        if len(set(idx)) != len(idx):
            dup = next(j for k, j in enumerate(idx) if j in idx[:k])
            raise ValueError("%s: %s names variable %d twice" % (who, name, dup))
        sets.append(sorted(idx))
    ints, bins = sets
    return sorted(set(ints) | set(bins)), bins


def largest_node_bytes(n, m_ub, m_eq, n_int, n_bin):
    """8 * w * (h + 2 * n_int): the root's n_bin binary rows and two cuts per integer variable."""
    return 8 * (n + 1) * (1 + m_ub + 2 * m_eq + n_bin + 2 * n_int)


def dense_tableau(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, binaries=(), maximize=False):
    """The flat row-major (1 + m_ub + 2 m_eq + n_bin) x (n + 1) matrix of ONE MILP: row 0 = +0.0, sign * c (a product); rows
    1 + i = b_ub[i], A_ub[i]; rows 1 + m_ub + 2k and the next = b_eq[k], A_eq[k] and their negations; then one row per binary
    variable j in ascending order: column 0 and column j + 1 are 1.0."""
    c = np.asarray(c, np.float64)
    n = c.shape[0]
    m_ub = 0 if b_ub is None else len(b_ub)
    m_eq = 0 if b_eq is None else len(b_eq)
    bins = sorted(int(j) for j in binaries)
    h0 = 1 + m_ub + 2 * m_eq
    m = np.zeros((h0 + len(bins), n + 1), np.float64)
    m[0, 1:] = np.float64(1.0 if maximize else -1.0) * c
    if m_ub:
        m[1:1 + m_ub, 0] = b_ub
        m[1:1 + m_ub, 1:] = np.asarray(A_ub, np.float64).reshape(m_ub, n)
    if m_eq:
        A, b = np.asarray(A_eq, np.float64).reshape(m_eq, n), np.asarray(b_eq, np.float64)
        m[1 + m_ub:h0:2, 0], m[1 + m_ub:h0:2, 1:] = b, A
        m[2 + m_ub:h0:2, 0], m[2 + m_ub:h0:2, 1:] = -b, -A
    for q, j in enumerate(bins):
        m[h0 + q, 0] = m[h0 + q, j + 1] = 1.0
    return m.ravel()


def packed_milp(lp, integers, binaries, maximize, options):
    """One dense MILP as _native.PackedMilps takes it: (width, height, row, col, val, integer columns, sign, options).
    lp = (c, A_ub, b_ub, A_eq, b_eq); integers / binaries as integer_sets returns them."""
    m = dense_tableau(*lp, binaries=binaries, maximize=maximize)
    w = len(lp[0]) + 1
    h = m.size // w
    return (w, h, *_native.dense_cells(m, w, h), [j + 1 for j in integers], 1.0 if maximize else -1.0, options)


def dense_solution(col0, pos, var, status, result, sign, precision, n):
    """(x[n], objective) of one best tableau of width n + 1, as solution() reads it."""
    w = n + 1
    if status == "optimal" or (status == "timedout" and not math.isnan(result)):
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
