"""Best-first branch and bound over variable-bound cuts: host-side caller of the hot path,
restating the reference's src/branchAndCut.ts:22-176.  Every node re-solves `root optimal
tableau + cut rows` (:126-127); a node is the tuple of its cuts (sign, variable, value).

_search holds the loop of branchAndCut (:89-176) once.  The three entry points differ only in
how a node gets its status, result and tableau view:
  branch_and_cut          applyCuts into a host buffer, then a simplex callable (the reference's flow);
  branch_and_cut_batched  the popped node and the next-best frontier nodes together on the GPU (NodeBatch);
  branch_and_cut_device   the root stays in HBM, each node is one DeviceTableau.node_solve call.

Queue: the reference uses npm `heap` 0.2.7 (package.json:157), which is a port of Python's
heapq; heapq with an eval-only ordering therefore pops ties in the same order.
"""
import heapq
import math
import time

import numpy as np

from .model import Tableau, TableauModel


class _Branch:
    __slots__ = ("eval", "cuts")

    def __init__(self, ev, cuts):
        self.eval, self.cuts = ev, cuts

    def __lt__(self, other):  # comparator (x, y) => x[0] - y[0], :100
        return self.eval < other.eval


def _js_ceil(x):
    """Math.ceil: -0 for a value in (-1, 0), like std::ceil in milp_host.inc (math.ceil returns the integer 0)."""
    return float(np.ceil(x))


def _cuts_on(variable, value):
    """The cuts that split a node on `variable` (:101-102, :153-154): the upper branch's
    (-1, variable, Math.ceil(value)) and the lower branch's (1, variable, Math.floor(value))."""
    return (-1, variable, _js_ceil(value)), (1, variable, float(math.floor(value)))


def _nothing():
    pass


def apply_cuts(tableau, buf, cuts):
    """:22-61  new tableau = root tableau + one row per cut (sign, variable, value)."""
    matrix, pos, var = buf
    width, height = tableau.width, tableau.height
    n = tableau.matrix.size
    matrix[:n] = tableau.matrix
    for i, (sign, variable, value) in enumerate(cuts):
        r = (height + i) * width
        p = int(tableau.position_of_variable[variable])
        if p < width:
            matrix[r] = sign * value
            matrix[r + 1:r + width] = 0.0
            matrix[r + p] = sign
        else:
            row = (p - width) * width
            matrix[r] = sign * (value - matrix[row])
            matrix[r + 1:r + width] = -sign * matrix[row + 1:row + width]
    length = width + height + len(cuts)
    pos[:width + height] = tableau.position_of_variable
    var[:width + height] = tableau.variable_at_position
    ext = np.arange(width + height, length, dtype=np.int32)
    pos[width + height:length] = ext
    var[width + height:length] = ext
    return Tableau(matrix[:n + width * len(cuts)], width, height + len(cuts), pos[:length], var[:length])


def most_fractional_var(tableau, int_vars):
    """:64-85 (vectorised: the first variable with the strictly largest fractional part)"""
    if not len(int_vars):
        return 0, 0.0, 0.0
    ints = np.asarray(int_vars, np.int64)
    rows = tableau.position_of_variable[ints].astype(np.int64) - tableau.width
    basic = rows >= 0
    if not basic.any():
        return 0, 0.0, 0.0
    col0 = tableau.col0 if tableau.col0 is not None else tableau.matrix[::tableau.width]
    vals = col0[rows[basic]]
    f = np.floor(vals)
    with np.errstate(invalid="ignore"):
        frac = np.abs(vals - np.where(vals - f >= 0.5, f + 1.0, f))  # |val - Math.round(val)|
    frac = np.where(np.isnan(frac), -1.0, frac)  # (NaN never wins a `>` comparison)
    k = int(np.argmax(frac))  # first maximum = the reference's strict `>` scan
    if not frac[k] > 0.0:
        return 0, 0.0, 0.0
    return int(ints[basic][k]), float(vals[k]), float(frac[k])


def _search(tabmod, init_result, options, open_nodes):
    """:89-176 with the node evaluation left to the caller.  open_nodes(branches) runs once the root's
    two branches are queued, before the clock starts, and returns (evaluate, keep, release):
    evaluate(cuts) -> (status, result, tableau view; the view is read only when status is "optimal"),
    keep() runs when the node just evaluated becomes the incumbent, release() runs on every exit.
    Returns (TableauModel of the best tableau, status, result)."""
    tableau, sign, integers = tabmod.tableau, tabmod.sign, tabmod.integers
    precision, max_iterations = options["precision"], options["maxIterations"]
    tolerance, timeout = options["tolerance"], options["timeout"]
    init_variable, init_value, init_frac = most_fractional_var(tableau, integers)
    if init_frac <= precision:
        return tabmod, "optimal", init_result

    branches = []
    upper, lower = _cuts_on(init_variable, init_value)
    heapq.heappush(branches, _Branch(init_result, (upper,)))
    heapq.heappush(branches, _Branch(init_result, (lower,)))
    evaluate, keep, release = open_nodes(branches)
    try:
        optimal_threshold = init_result * (1.0 - sign * tolerance)
        now = lambda: time.time() * 1000.0  # noqa: E731  Date.now()
        stop_time = timeout + now()
        timedout = now() >= stop_time
        solution_found, best_eval, best_tableau, it = False, math.inf, tableau, 0
        while it < max_iterations and branches and best_eval >= optimal_threshold and not timedout:
            br = heapq.heappop(branches)
            relaxed_eval, cuts = br.eval, br.cuts
            if relaxed_eval > best_eval:
                break
            status, result, current = evaluate(cuts)
            if status == "optimal" and result < best_eval:
                variable, value, frac = most_fractional_var(current, integers)
                if frac <= precision:
                    solution_found, best_eval, best_tableau = True, result, current
                    keep()
                else:
                    # :141-154  each branch drops the cuts on `variable` that its new cut supersedes
                    upper, lower = _cuts_on(variable, value)
                    cuts_upper = tuple([c for c in cuts if c[1] != variable or c[0] >= 0]) + (upper,)
                    cuts_lower = tuple([c for c in cuts if c[1] != variable or c[0] < 0]) + (lower,)
                    heapq.heappush(branches, _Branch(result, cuts_upper))
                    heapq.heappush(branches, _Branch(result, cuts_lower))
            timedout = now() >= stop_time
            it += 1
    finally:
        release()

    unfinished = (timedout or it >= max_iterations) and bool(branches) and best_eval >= optimal_threshold
    status = "timedout" if unfinished else ("infeasible" if not solution_found else "optimal")
    return (TableauModel(best_tableau, sign, tabmod.variables, integers), status,
            best_eval if solution_found else math.nan)


def branch_and_cut(simplex, tabmod, init_result, options):
    """:89-176 with the reference's nodes: applyCuts (:22-61) into a host buffer, then
    simplex(tableau, options) -> (status, result).  Returns (TableauModel of the best tableau, status, result)."""
    tableau = tabmod.tableau

    def open_nodes(branches):
        max_extra_rows = len(tabmod.integers) * 2
        matrix_length = tableau.matrix.size + max_extra_rows * tableau.width
        pos_var_length = tableau.position_of_variable.size + max_extra_rows

        buffers = [(np.zeros(matrix_length, np.float64), np.zeros(pos_var_length, np.int32),
                    np.zeros(pos_var_length, np.int32)) for _ in range(2)]  # [candidate, incumbent's] (:104-112)

        def evaluate(cuts):
            current = apply_cuts(tableau, buffers[0], cuts)
            status, result = simplex(current, options)
            return status, result, current

        # :137-139  a new incumbent keeps its buffer: the next node is built in the other one
        return evaluate, buffers.reverse, _nothing

    return _search(tabmod, init_result, options, open_nodes)


def branch_and_cut_batched(tabmod, init_result, options, node_batch, stats=None):
    """branchAndCut (:89-176) with the node LPs evaluated on the GPU in batches (yalps_batch_*):
    whenever the popped node has no result yet, it and the next-best `node_batch - 1` frontier nodes
    are solved together (one workgroup per node, root resident, cuts applied on the device).  A
    node's LP depends only on the root and its cuts, so evaluating it early changes nothing; nodes
    are consumed in exactly the reference's pop order.  Returns what branch_and_cut returns."""
    from . import _native
    tableau, stats = tabmod.tableau, {} if stats is None else stats

    def open_nodes(branches):
        ctx = _native.Context(0)
        batch = _native.NodeBatch(ctx, tableau.width, tableau.height, len(tabmod.integers) * 2, node_batch)
        batch.set_root(tableau.matrix, tableau.position_of_variable, tableau.variable_at_position)
        cache = {}
        stats.update(batches=0, nodes_evaluated=0, nodes_used=0, pivots=0, gpu_ms=0.0)

        def evaluate(cuts):
            if cuts not in cache:
                todo, seen = [cuts], {cuts}
                for br in heapq.nsmallest(node_batch - 1, branches):
                    if br.cuts not in cache and br.cuts not in seen:
                        todo.append(br.cuts)
                        seen.add(br.cuts)
                st, res, piv, heights, ms = batch.solve(todo, options["precision"], options["maxPivots"])
                for i, node in enumerate(todo):
                    view = None
                    if st[i] == "optimal":
                        _, col0, pos, var = batch.download(i, int(heights[i]))
                        view = Tableau(None, tableau.width, int(heights[i]), pos, var, col0)
                    cache[node] = (st[i], float(res[i]), view)
                stats["batches"] += 1
                stats["nodes_evaluated"] += len(todo)
                stats["pivots"] += int(piv.sum())
                stats["gpu_ms"] += ms
            stats["nodes_used"] += 1
            return cache.pop(cuts)

        def release():
            batch.close()
            ctx.close()

        return evaluate, _nothing, release

    return _search(tabmod, init_result, options, open_nodes)


def branch_and_cut_device(tabmod, root, node, init_result, options, stats=None):
    """branchAndCut (:89-176), one node at a time like the reference, but with the root's optimal tableau
    resident in HBM (`root`, a DeviceTableau) and every node built next to it on the device
    (yalps_tableau_apply_cuts into `node`): per node only the cuts go up and column 0 + the permutations come
    back -- what most_fractional_var (:64-85) and solution() read.  `tabmod.tableau` is the root's view
    (col0 + permutations).  Returns what branch_and_cut returns."""
    width, stats = tabmod.tableau.width, {} if stats is None else stats

    def open_nodes(branches):
        stats.update(device_nodes=0)  # (no pivot count on this path: yalps_tableau_node_solve returns status, result, column 0 and the basis only)

        def evaluate(cuts):
            # applyCuts + simplex + column 0 / permutations back: one native call (three launches, one wait)
            status, result, height, col0, pos, var = node.node_solve(root, cuts, options["precision"],
                                                                     options["maxPivots"], options["checkCycles"])
            stats["device_nodes"] += 1
            return status, result, Tableau(None, width, height, pos, var, col0) if status == "optimal" else None

        return evaluate, _nothing, _nothing

    return _search(tabmod, init_result, options, open_nodes)
