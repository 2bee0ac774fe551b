"""The host side of tensors.milp_batch (numpy only; nothing here imports torch or touches the GPU): the integer sets of a
call, and the fallback for trees that overflowed on the device -- tableauModel's tableau of one dense MILP (reference
src/tableau.ts:47-137), its cells as the lockstep driver (_native.MilpBatch) takes them, and solution() (src/YALPS.ts:8-50)
of a best tableau as a dense row.  With variable bounds (milp_batch's lb, ub, upper) the tableau is the bounded one -- the
right-hand sides moved by shift_sum with the effective lower bounds, the bound rows between the equality rows and the binary
rows -- and the dense row is moved back.  With free variables (milp_batch_free's free) it is the split one: one twin column per free
variable behind the n originals, the twins of the free integer variables among the integer columns, and the dense row is
x[j] = v(p) - v(q) there."""
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


def largest_node_bytes(n, m_ub, m_eq, n_int, n_bin, k=0, f=0, int_twins=0):
    """8 * w * (h + 2 * n_int_eff): the root's k bound rows and n_bin binary rows, two cuts per integer COLUMN -- the n_int
    integer variables and the int_twins twins of the free ones among them -- and f twin columns in the width."""
    return 8 * (n + 1 + f) * (1 + m_ub + 2 * m_eq + k + n_bin + 2 * (n_int + int_twins))


SHIFT_LANES = 64


def shift_sum(a, l):
    """sum of a[j] * l[j] in the order the kernels use (lp_dense_kernel.cuh): every product rounded on its own; 64 partial sums,
    each from +0.0 over the columns j = k (mod 64) in ascending j; then p[k] += p[k + s] for k < s, s = 32, 16, 8, 4, 2, 1."""
    a, l = np.asarray(a, np.float64).reshape(-1), np.asarray(l, np.float64).reshape(-1)
    if a.size != l.size:
        raise ValueError("shift_sum: %d coefficients, %d bounds" % (a.size, l.size))
    p = np.zeros(SHIFT_LANES, np.float64)
    with np.errstate(all="ignore"):
        for lo in range(0, a.size, SHIFT_LANES):  # (one round of the lanes: lane k adds column lo + k)
            part = a[lo:lo + SHIFT_LANES] * l[lo:lo + SHIFT_LANES]
            p[:part.size] = p[:part.size] + part
        s = SHIFT_LANES // 2
        while s:
            p[:s] = p[:s] + p[s:2 * s]
            s //= 2
    return np.float64(p[0])


def bound_rows(idx, binaries, everything, who="milp_batch"):
    """The variables with a bound row: `idx` is the ascending list `upper` stands for (tensors._upper_set).  everything (upper
    was True): every variable that is not binary; else the list as it is, and one that names a binary variable is a ValueError
    -- a binary variable has no bound row of its own, its ub is not read."""
    bins = set(int(j) for j in binaries)
    if everything:
        return [j for j in idx if j not in bins]
    named = [j for j in idx if j in bins]
    if named:
        raise ValueError("%s: upper names variable %d, which is binary: a binary variable has no bound row of its own (its ub "
                         "is not read)" % (who, named[0]))
    return list(idx)


def free_set(idx, binaries, everything, who="milp_batch"):
    """The free variables: `idx` is the ascending list `free` stands for (tensors._free_set).  everything (free was True): every
    variable that is not binary; else the list as it is, and one that names a binary variable is a ValueError, as bound_rows
    refuses it -- a binary variable is 0 or 1 and cannot be free."""
    bins = set(int(j) for j in binaries)
    if everything:
        return [j for j in idx if j not in bins]
    named = [j for j in idx if j in bins]
    if named:
        raise ValueError("%s: free names variable %d, which is binary: a binary variable cannot be free" % (who, named[0]))
    return list(idx)


def integer_columns(n, integers, free=()):
    """The tableau's integer columns as the trees take them: 1 + j of the integer variables in ascending j, then the twin
    columns 1 + n + t of the free integer variables in ascending j -- the whole list ascends."""
    ints, fidx = [int(j) for j in integers], sorted(int(j) for j in free)
    return [j + 1 for j in ints] + [1 + n + t for t, j in enumerate(fidx) if j in set(ints)]


def effective_lower(lb, integers=(), binaries=(), free=()):
    """l_eff of ONE MILP: lb[j] at a continuous variable, ceil(lb[j]) at an integer one (IEEE: ceil(-0.5) is -0.0; NaN and the
    infinities pass through), +0.0 at a binary one and at a free one, integer or not, whatever lb holds there.  None without
    lb."""
    if lb is None:
        return None
    l = np.array(lb, np.float64).reshape(-1)
    ints, bins = [int(j) for j in integers], [int(j) for j in binaries]
    with np.errstate(all="ignore"):
        l[ints] = np.ceil(l[ints])
    l[bins] = 0.0
    l[[int(j) for j in free]] = 0.0
    return l


def dense_tableau(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, binaries=(), maximize=False, integers=(), lb=None, ub=None, upper=(),
                  free=()):
    """The flat row-major (1 + m_ub + 2 m_eq + k + n_bin) x (n + 1) matrix of ONE MILP: row 0 = +0.0, sign * c (a product); rows
    1 + i = b_ub[i], A_ub[i]; rows 1 + m_ub + 2k and the next = b_eq[k], A_eq[k] and their negations; then one row per binary
    variable j in ascending order: column 0 and column j + 1 are 1.0.
    Bounds: with lb, column 0 of every operand row is moved by shift_sum(row, l_eff), one subtraction (negated in the second
    row of an equality), l_eff = effective_lower(lb, integers, binaries); and between the equality rows and the binary rows
    come k = len(upper) rows, ascending: ub[j] - l_eff[j] (or ub[j]) in column 0, 1.0 in column j + 1.
    Free variables: the matrix is f = len(free) columns wider; twin t, column 1 + n + t, of the t-th free variable j in ascending
    order holds the IEEE negation of column 1 + j in every operand row, -1.0 in j's bound row, +0.0 in every other generated
    row; l_eff is +0.0 at j."""
    c = np.asarray(c, np.float64)
    n = c.shape[0]
    m_ub = 0 if b_ub is None else len(b_ub)
    m_eq = 0 if b_eq is None else len(b_eq)
    bins = sorted(int(j) for j in binaries)
    idx = sorted(int(j) for j in upper)
    fidx = sorted(int(j) for j in free)
    low = effective_lower(lb, integers, bins, fidx)
    h0 = 1 + m_ub + 2 * m_eq
    hb = h0 + len(idx)
    m = np.zeros((hb + len(bins), n + 1 + len(fidx)), np.float64)
    m[0, 1:n + 1] = np.float64(1.0 if maximize else -1.0) * c
    if m_ub:
        m[1:1 + m_ub, 0] = b_ub
        m[1:1 + m_ub, 1:n + 1] = np.asarray(A_ub, np.float64).reshape(m_ub, n)
    if m_eq:
        A, b = np.asarray(A_eq, np.float64).reshape(m_eq, n), np.asarray(b_eq, np.float64)
        m[1 + m_ub:h0:2, 0], m[1 + m_ub:h0:2, 1:n + 1] = b, A
        m[2 + m_ub:h0:2, 0], m[2 + m_ub:h0:2, 1:n + 1] = -b, -A
    with np.errstate(all="ignore"):
        if low is not None:
            for i in range(m_ub):
                m[1 + i, 0] = m[1 + i, 0] - shift_sum(m[1 + i, 1:n + 1], low)
            for k in range(m_eq):
                v = m[1 + m_ub + 2 * k, 0] - shift_sum(m[1 + m_ub + 2 * k, 1:n + 1], low)
                m[1 + m_ub + 2 * k, 0], m[2 + m_ub + 2 * k, 0] = v, -v
        for t, j in enumerate(idx):
            u = np.float64(np.asarray(ub, np.float64).reshape(-1)[j])
            m[h0 + t, 0] = u - low[j] if low is not None else u
            m[h0 + t, j + 1] = 1.0
            if j in fidx:
                m[h0 + t, 1 + n + fidx.index(j)] = -1.0
    for t, j in enumerate(fidx):
        m[:h0, 1 + n + t] = -m[:h0, 1 + j]
    for q, j in enumerate(bins):
        m[hb + q, 0] = m[hb + q, j + 1] = 1.0
    return m.ravel()


def packed_milp(lp, integers, binaries, maximize, options, lb=None, ub=None, upper=(), free=()):
    """One dense MILP as _native.PackedMilps takes it: (width, height, row, col, val, integer columns, sign, options).
    lp = (c, A_ub, b_ub, A_eq, b_eq); integers / binaries as integer_sets returns them; lb / ub / upper: its bounds
    and free variables (dense_tableau; the integer columns by integer_columns)."""
    m = dense_tableau(*lp, binaries=binaries, maximize=maximize, integers=integers, lb=lb, ub=ub, upper=upper, free=free)
    n = len(lp[0])
    w = n + 1 + len(free)
    h = m.size // w
    return (w, h, *_native.dense_cells(m, w, h), integer_columns(n, integers, free), 1.0 if maximize else -1.0, options)


def dense_solution(col0, pos, var, status, result, sign, precision, n, c=None, low=None, free=()):
    """(x[n], objective) of one best tableau of width n + 1, as solution() reads it.  low (effective_lower's l_eff) and c: the
    answer in x' moved back, x = x' + low and objective = objective' + shift_sum(c, low), one addition each whatever the
    status.  free: the tableau is len(free) columns wider and x[j] of a free variable is v(p) - v(q), one subtraction of the two
    columns' own values -- so an unbounded twin gives -inf -- in front of the addition of low."""
    if low is not None:
        x, objective = dense_solution(col0, pos, var, status, result, sign, precision, n, free=free)
        with np.errstate(all="ignore"):
            return x + np.asarray(low, np.float64), float(np.float64(objective) + shift_sum(c, low))
    if len(free):
        fidx = sorted(int(j) for j in free)
        wide, objective = dense_solution(col0, pos, var, status, result, sign, precision, n + len(fidx))
        x = wide[:n].copy()
        with np.errstate(all="ignore"):
            x[fidx] = wide[fidx] - wide[n:]
        return x, objective
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
