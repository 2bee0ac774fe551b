"""A scalar restatement of the reference's branchAndCut (src/branchAndCut.ts:22-176) with one switch per decision site, the
node LPs solved by the C oracle (TEST INFRASTRUCTURE).  Without switches it reproduces the MILP records
(tests/golden/simplex_milp.json.gz) node by node; tests/test_milp_records.py checks that every switch (a mutant) is
rejected by some record, so the records tell a right reading of branchAndCut.ts from each wrong one."""
import hashlib
import heapq
import math
import time

import numpy as np

MUTANTS = {
    "push_lower_first": "the child with the new upper-bound cut is pushed first (:157-158 push cutsUpper, then cutsLower)",
    "break_ge": "relaxedEval >= bestEval breaks (:119 is >)",
    "improve_le": "result <= bestEval is taken (:128 is <)",
    "frac_lt": "frac < precision is integral (:94, :131 are <=)",
    "mfv_last_wins": "the last of equally fractional variables wins (:78 is a strict >)",
    "threshold_sign": "optimalThreshold = initResult * (1 + sign * tolerance) (:105 has a minus)",
    "unfinished_no_timedout": "unfinished without its `timedout ||` term (:166)",
    "unfinished_no_iterations": "unfinished without its `iter >= maxIterations` term (:166)",
    "unfinished_no_empty": "unfinished without its `!branches.empty()` term (:166)",
    "unfinished_no_threshold": "unfinished without its `bestEval >= optimalThreshold` term (:166)",
    "same_var_swapped": "a cut on the branching variable is kept by the other child (:146-147)",
    "ceil_plus_zero": "Math.ceil of a value in (-1, 0) taken as +0 instead of -0 (:103, :155)",
}


def hexd(x):
    return np.float64(x).byteswap().tobytes().hex()  # big-endian bytes, as the generator writes them


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _js_round(x):
    f = math.floor(x)
    return f + 1.0 if x - f >= 0.5 else float(f)


class _Branch:
    __slots__ = ("eval", "cuts")

    def __init__(self, ev, cuts):
        self.eval, self.cuts = ev, cuts

    def __lt__(self, other):  # (x, y) => x[0] - y[0] < 0
        return self.eval - other.eval < 0


def _most_fractional(matrix, width, pos, ints, rules):
    highest, variable, value = 0.0, 0, 0.0
    for v in ints:
        row = int(pos[v]) - width
        if row < 0:
            continue
        val = float(matrix[row * width])
        frac = abs(val - _js_round(val))
        if frac > highest or ("mfv_last_wins" in rules and frac == highest and frac > 0.0):
            highest, variable, value = frac, v, val
    return variable, value, highest


def _apply_cuts(matrix, width, height, pos, var, cuts):
    out = np.zeros(matrix.size + width * len(cuts))
    out[:matrix.size] = matrix
    for i, (sign, v, value) in enumerate(cuts):
        r = (height + i) * width
        p = int(pos[v])
        if p < width:
            out[r] = sign * value
            out[r + p] = sign
        else:
            row = (p - width) * width
            out[r] = sign * (value - out[row])
            out[r + 1:r + width] = -sign * out[row + 1:row + width]
    n = width + height + len(cuts)
    npos = np.arange(n, dtype=np.int32)
    nvar = np.arange(n, dtype=np.int32)
    npos[:width + height], nvar[:width + height] = pos, var
    return out, height + len(cuts), npos, nvar


def branch_and_cut(oracle, root, width, height, pos, var, sign, integers, init_result, options, rules=frozenset()):
    """root / pos / var: the root's optimal tableau.  Returns what a MILP record holds of the run (the nodes, the exit, the
    iteration count, the tableau solution() reads, the status and the result)."""
    precision, max_iterations = options["precision"], options["maxIterations"]
    tolerance, timeout = options["tolerance"], options["timeout"]
    out = dict(nodes=[], exit=None)
    ceil = (lambda x: float(math.ceil(x))) if "ceil_plus_zero" in rules else (lambda x: float(np.ceil(x)))

    def integral(frac):
        return frac < precision if "frac_lt" in rules else frac <= precision

    def best(m, h, p, v):
        out.update(best_height=h, best_col0=sha(m[::width][:h]), best_perm=sha(p[:width + h], v[:width + h]))

    variable, value, frac = _most_fractional(root, width, pos, integers, rules)
    if integral(frac):
        best(root, height, pos, var)
        out.update(exit="integral", iterations=0, status="optimal", result=init_result)
        return out
    branches = []
    first = [_Branch(init_result, [(-1, variable, ceil(value))]), _Branch(init_result, [(1, variable, math.floor(value))])]
    for br in first:
        heapq.heappush(branches, br)
    threshold = init_result * (1.0 + sign * tolerance if "threshold_sign" in rules else 1.0 - sign * tolerance)
    stop = timeout + time.time() * 1000.0
    timedout = time.time() * 1000.0 >= stop
    found, best_eval, it = False, math.inf, 0
    best(root, height, pos, var)
    while it < max_iterations and branches and best_eval >= threshold and not timedout:
        br = heapq.heappop(branches)
        if br.eval > best_eval or ("break_ge" in rules and br.eval >= best_eval):
            out["exit"] = "break"
            break
        m, h, p, v = _apply_cuts(root, width, height, pos, var, br.cuts)
        node = dict(eval=hexd(br.eval), cuts=[[s, x, hexd(c)] for s, x, c in br.cuts], init_sha256=sha(m))
        st, res, npiv, _ = oracle.simplex(m, width, h, p, v, precision=options["precision"],
                                          max_pivots=options["maxPivots"], check_cycles=options["checkCycles"])
        node.update(status=st, result=hexd(res), n_pivots=npiv, final_sha256=sha(m), perm_sha256=sha(p, v))
        out["nodes"].append(node)
        if st == "optimal" and (res < best_eval or ("improve_le" in rules and res == best_eval)):
            variable, value, frac = _most_fractional(m, width, p, integers, rules)
            if integral(frac):
                found, best_eval = True, res
                best(m, h, p, v)
            else:
                upper, lower = [], []
                for cut in br.cuts:
                    if cut[1] == variable:
                        keep_lower = cut[0] < 0 if "same_var_swapped" not in rules else cut[0] > 0
                        (lower if keep_lower else upper).append(cut)
                    else:
                        upper.append(cut)
                        lower.append(cut)
                lower.append((1, variable, math.floor(value)))
                upper.append((-1, variable, ceil(value)))
                children = [_Branch(res, upper), _Branch(res, lower)]
                if "push_lower_first" in rules:
                    children.reverse()
                for c in children:
                    heapq.heappush(branches, c)
        timedout = time.time() * 1000.0 >= stop
        it += 1
    if out["exit"] is None:
        out["exit"] = ("iterations" if not it < max_iterations else "exhausted" if not branches
                       else "threshold" if not best_eval >= threshold else "timeout")
    terms = [timedout or it >= max_iterations, bool(branches), best_eval >= threshold]
    drop = {"unfinished_no_timedout": (0, it >= max_iterations), "unfinished_no_iterations": (0, timedout),
            "unfinished_no_empty": (1, True), "unfinished_no_threshold": (2, True)}
    for name, (k, repl) in drop.items():
        if name in rules:
            terms[k] = repl
    unfinished = all(terms)
    out.update(iterations=it, status="timedout" if unfinished else ("optimal" if found else "infeasible"),
               result=best_eval if found else math.nan)
    return out
