"""Sensitivity analysis of LPs: duals, reduced costs, right-hand-side and objective ranges, read off the final tableau.

The device side is libyalps_lpsens.so (include/yalps_lpsens.h): lp_batch_kernel's solve, and for every LP that ends optimal
five arrays ranged from the final matrix M by the workgroup that solved it (row0, col_up, col_dn, row_lo, row_hi).  This
module maps them to the model's own terms.  Conventions, with s = tabmod.sign, pos the final positionOfVariable, b_r and
k_j the INITIAL M[r,0] and M[0,j] (from the cells; 0 where none was written):

  clamping      col_up, col_dn, row_hi and -row0[c] to >= 0, row_lo to <= 0 -- here only, the native arrays are raw
  row dual      y_r = -row0[pos[w + r]] where the row's slack is non-basic (pos[w + r] < w), else 0
  constraint    first row r: its upper side is row r (upper bound finite), its lower side the next row, or row r where
                there is no upper side.  dual = s * (y_upper - y_lower) = d(objective) / d(bound).
  rhs range     of a row: [b_r - M[i,0], +inf) where its slack is basic in row i, [b_r - col_up[c], b_r + col_dn[c]] where
                it is non-basic in column c.  "upper_range" is that interval for the upper row, "lower_range" the negated,
                swapped interval of the lower row (whose right-hand side is -lower).  Each side is ranged with the other held
                fixed; an `equal` constraint reports both.
  variable j    non-basic in column c: reduced_cost = s * min(row0[c], 0), internal coefficient range (-inf, k_j - row0[c]];
                basic in row i: reduced_cost = 0, internal range [k_j + row_lo[i], k_j + row_hi[i]].  "objective_range" is
                the internal range for s = +1 and the negated, swapped one for s = -1: a range of the model's coefficient.

Inside a range the optimal basis holds: the objective moves by dual * delta for a bound, by delta * value for a coefficient.
"""
import math
import threading

import numpy as np

from . import _native
from .model import tableau_model_with_bounds

INF = math.inf


def ranges_from_tableau(matrix, width, height, precision):
    """(row0, col_up, col_dn, row_lo, row_hi) of a final matrix (flat row-major width * height) on the host, as
    lp_sens_kernel computes them (include/yalps_lpsens.h).  For the LPs above the batch limit, whose matrix comes back from
    the whole-chip kernels; vectorised, one division per entry and pass."""
    M = np.asarray(matrix, np.float64)[:width * height].reshape(height, width)
    body, rhs, obj = M[1:, 1:], M[1:, :1], M[:1, 1:]
    above, below = body > precision, body < -precision
    zero = np.zeros(1)
    with np.errstate(all="ignore"):
        q = rhs / body
        col_up = np.fmin.reduce(np.where(above, q, INF), axis=0, initial=INF)
        col_dn = np.fmin.reduce(np.where(below, -q, INF), axis=0, initial=INF)
        k = obj / body
        row_lo = np.fmax.reduce(np.where(above, k, -INF), axis=1, initial=-INF)
        row_hi = np.fmin.reduce(np.where(below, k, INF), axis=1, initial=INF)
    return (M[0].copy(), np.concatenate([zero, col_up]), np.concatenate([zero, col_dn]), np.concatenate([zero, row_lo]),
            np.concatenate([zero, row_hi]))


def _plus(x):
    """-0.0 -> 0.0"""
    return float(x) + 0.0


def sensitivity_of(tabmod, bounds_info, ranges):
    """The "sensitivity" value of one optimal LP: tabmod as the solve left it (col0 and permutations of the final tableau,
    the cells of the initial one), bounds_info from tableau_model_with_bounds, ranges the five native arrays."""
    t, s = tabmod.tableau, tabmod.sign
    w, h = t.width, t.height
    pos = t.position_of_variable
    row0, col_up, col_dn, row_lo, row_hi = (np.asarray(a, np.float64) for a in ranges)
    cost = np.minimum(row0, 0.0)  # (-row0[c] clamped to >= 0)
    col_up, col_dn, row_hi = np.maximum(col_up, 0.0), np.maximum(col_dn, 0.0), np.maximum(row_hi, 0.0)
    row_lo = np.minimum(row_lo, 0.0)
    row, col, val = t.cells
    b, k = np.zeros(h), np.zeros(w)
    b[row[col == 0]] = val[col == 0]
    k[col[row == 0]] = val[row == 0]

    def side(r):
        """(y_r, the range of row r's right-hand side)"""
        p = int(pos[w + r])
        if p >= w:
            return 0.0, (float(b[r]) - t.rhs(p - w), INF)
        return -float(cost[p]), (float(b[r] - col_up[p]), float(b[r] + col_dn[p]))

    constraints = []
    for key, bound in bounds_info["bounds"].items():
        r = bound["row"]
        entry, y_upper, y_lower = {}, 0.0, 0.0
        if math.isfinite(bound["upper"]):
            y_upper, entry["upper_range"] = side(r)
            r += 1
        if math.isfinite(bound["lower"]):
            y_lower, (lo, hi) = side(r)
            entry["lower_range"] = (_plus(-hi), _plus(-lo))
        constraints.append((key, {"dual": _plus(s * (y_upper - y_lower)), **entry}))

    variables = []
    for j, (key, _) in enumerate(tabmod.variables, start=1):
        p = int(pos[j])
        if p < w:
            reduced, lo, hi = s * float(cost[p]), -INF, float(k[j] - cost[p])
        else:
            reduced, lo, hi = 0.0, float(k[j] + row_lo[p - w]), float(k[j] + row_hi[p - w])
        if s < 0:
            lo, hi = -hi, -lo
        variables.append((key, {"reduced_cost": _plus(reduced), "objective_range": (_plus(lo), _plus(hi))}))
    return {"constraints": constraints, "variables": variables}


_lpsens = None  # the process's LpSens: stream, events and device buffers are kept and grown between calls
_lpsens_lock = threading.Lock()  # (a handle belongs to one thread at a time)


def lpsens_simplex(tableaux, options, stats=None):
    """The batched backend of sensitivity_many: every tableau (built with sparse=True) through ONE yalps_lpsens_solve; column
    0 and the permutations land in the tableaux.  Returns [(status, result, ranges | None)]."""
    global _lpsens
    with _lpsens_lock:
        if _lpsens is None:
            _lpsens = _native.LpSens(0)
        batch = _lpsens
        statuses, results, _, _ = batch.solve(
            [(t.width, t.height, *t.cells, o["precision"], o["maxPivots"], o["checkCycles"]) for t, o in zip(tableaux, options)])
        out = []
        for i, t in enumerate(tableaux):
            t.col0, t.position_of_variable, t.variable_at_position = batch.solution(i)
            out.append((statuses[i], float(results[i]), batch.ranges(i) if statuses[i] == "optimal" else None))
        if stats is not None:
            info = batch.info()
            stats.update(launches=info["launches"], reruns=info["reruns"], kernels=info["kernels"])
    return out


def device_tableau_sensitivity(tableau, opt):
    """The backend for one LP above the batch limit: assembled in HBM from its cells, solved by the whole-chip kernels, the
    final matrix downloaded and ranged on the host (ranges_from_tableau).  Returns (status, result, ranges | None)."""
    ctx = _native.Context(0)
    dev = _native.DeviceTableau(ctx, tableau.width, tableau.height)
    try:
        dev.assemble(tableau.height, *tableau.cells)
        status, result, _, _ = dev.solve(opt["precision"], opt["maxPivots"], opt["checkCycles"])
        matrix, tableau.position_of_variable, tableau.variable_at_position = dev.download()
    finally:
        dev.close()
        ctx.close()
    tableau.col0 = np.ascontiguousarray(matrix[::tableau.width][:tableau.height])
    ranges = ranges_from_tableau(matrix, tableau.width, tableau.height, opt["precision"]) if status == "optimal" else None
    return status, float(result), ranges


def _sensitivity_many_with(batch_backend, large_backend, models, options=None, stats=None):
    """sensitivity_many with its backends as parameters (tests drive the routing and the mapping with the CPU oracle):
    batch_backend(tableaux, options, stats) -> [(status, result, ranges | None)] for the LPs of at most 4 MiB,
    large_backend(tableau, options) -> (status, result, ranges | None) for a larger one; both leave column 0 and the
    permutations of the final tableau in the tableaux they are given."""
    from .solve import _DEFAULTS, NODE_BATCH_MAX_BYTES, solution
    models = list(models)
    opts = list(options) if isinstance(options, (list, tuple)) else [options] * len(models)
    if len(opts) != len(models):
        raise ValueError("sensitivity_many: %d models but %d option sets" % (len(models), len(opts)))
    items, batched, large = [], [], []
    for i, (model, o) in enumerate(zip(models, opts)):
        tabmod, bounds_info = tableau_model_with_bounds(model, sparse=True)
        if tabmod.integers:
            raise ValueError("sensitivity_many: model %d has integer or binary variables; the duals of a branch-and-cut node "
                             "are not the model's" % i)
        opt = dict(_DEFAULTS)
        if o:
            opt.update({k: v for k, v in o.items() if v is not None})
        items.append((tabmod, bounds_info, opt))
        t = tabmod.tableau
        (batched if 8 * t.width * t.height <= NODE_BATCH_MAX_BYTES else large).append(i)
    if stats is not None:
        stats.update(batched=len(batched), large=len(large))
    answers = [None] * len(models)
    if batched:
        results = batch_backend([items[i][0].tableau for i in batched], [items[i][2] for i in batched], stats)
        for i, r in zip(batched, results):
            answers[i] = r
    for i in large:
        answers[i] = large_backend(items[i][0].tableau, items[i][2])
    out = []
    for (tabmod, bounds_info, opt), (status, result, ranges) in zip(items, answers):
        r = solution(tabmod, status, result, opt)
        r["sensitivity"] = sensitivity_of(tabmod, bounds_info, ranges) if status == "optimal" else None
        out.append(r)
    return out


def sensitivity_many(models, options=None, stats=None):
    """[solve(m, o) for m, o in zip(models, options)] -- same "status", "result" and "variables" -- each with a key
    "sensitivity": None unless the status is "optimal", else

      {"constraints": [(key, {"dual", "upper_range"?, "lower_range"?})]   one per merged constraint key, in first-seen order
       "variables":   [(key, {"reduced_cost", "objective_range"})]}       one per variable (column)

    dual is d(objective) / d(bound) in the model's own direction and sign; upper_range / lower_range are the (low, high)
    intervals of the constraint's upper / lower bound over which the optimal basis holds, present where that bound is finite,
    each with the other bound held fixed (an `equal` constraint has both); reduced_cost is what the objective would change
    per unit of a variable that is at zero; objective_range is the (low, high) interval of the variable's own objective
    coefficient over which the basis holds.  The module docstring has the formulas.

    `options` is one dict for all models or one per model.  Models whose tableau is at most 4 MiB go through ONE
    yalps_lpsens_solve, one workgroup per LP, the ranges computed from the final tableau where it lies; a larger LP is solved
    by the whole-chip kernels and its downloaded matrix is ranged on the host.  A model with `integers` or `binaries` raises
    ValueError: the final tableau of a branch-and-cut node carries that node's cuts, and its duals are not the model's.

    stats (a dict, optional) receives "batched" and "large" (models that went each way) and "launches", "reruns" and
    "kernels" of the native call."""
    return _sensitivity_many_with(lpsens_simplex, device_tableau_sensitivity, models, options, stats)


def sensitivity(model, options=None):
    """sensitivity_many([model], options)[0]: solve(model, options)'s dict plus "sensitivity".  ValueError for a model with
    `integers` or `binaries` (the duals of a branch-and-cut node are not the model's)."""
    return sensitivity_many([model], options)[0]
