"""Seeded MILP models for the branch-and-cut records (TEST INFRASTRUCTURE).

oracle/tools/gen_golden.py --only milp runs the reference's solve() (src/YALPS.ts -> tableau.ts -> simplex.ts ->
branchAndCut.ts) on every model of `specs()` and writes tests/golden/simplex_milp.json.gz; the tests regenerate each model
from (family, seed, variant) and check its initial-tableau digest first.  Every family is there on purpose:

  ties      integer knapsacks whose value / weight ratios repeat: siblings and cousins share evaluations, so the heap's tie
            order decides which node comes next (branchAndCut.ts:100)
  tol       tolerance > 0, minimise and maximise: the loop ends by the optimal threshold (:105, :112)
  iters     maxIterations 1 .. 12 on two models and 6 / 7 / 22 on a third: "timedout" with and without a solution (NaN result), and the budget met
            on the very iteration the queue empties or the threshold is crossed (the terms of `unfinished`, :166)
  timeout0  timeout 0: timed out before the first pop (:107), the one finite timeout that is deterministic
  intinf    LP feasible, integer infeasible (equalities with an odd right-hand side over even coefficients)
  integral  an integral root: no branching at all (:94-95); seed 2 at precision 0, where frac == precision
  break     a solution found early under a queue of worse evaluations: the `relaxedEval > bestEval` break (:119)
  eqmm      equalities, rows with both min and max, binaries
  deep      two or three integer variables in a thin sliver: deep branching, long cut lists (:141-156)
  full      a face parallel to the objective (dual degenerate optima): the LP can leave an integer variable fractional
            below its own upper cut, so every integer variable gets both cuts and a list reaches 2 * n_integers, the node
            buffers' capacity (:96-97)
  cycles    degenerate nodes (zero right-hand sides) with checkCycles
  negzero   precision 0 / 1e-17: round-off leaves basic values a hair off an integer, and they are branched on
            (a value in (-1, 0) would give the cut value Math.ceil = -0; see NEGZERO_SEEDS)
  mid       roots of 128 KB .. 4 MB: node batches in HBM, the fused resident node one at a time
  big       a root over 4 MB: node_batch 32 falls back to the resident root, one node at a time

Models are JSON data (string keys, insertion-ordered objects): the same dict goes to yalps_amd.model.tableau_model and,
as JSON, to the reference's tableauModel under node.  Random numbers: numpy's legacy RandomState (a frozen stream)."""
import numpy as np

FAMILIES = ("ties", "tol", "iters", "timeout0", "intinf", "integral", "break", "eqmm", "deep", "full", "cycles", "negzero",
            "mid", "big")

# seeds of the negzero family.  Seeds 0 .. 199 were searched with the reference for a -0 cut value and none has one: the
# integer variable that wins mostFractionalVar is never one whose value is a hair below zero.  Precision 0 (every fourth
# seed) makes the root's result NaN (roundToPrecision), so the optimal threshold is NaN and the loop never runs.
NEGZERO_SEEDS = (0, 1, 2, 3, 5)
# seeds of the deep family: the longest trees among seeds 0 .. 39 (16 .. 80 nodes); their cut lists reach 2 * n_integers - 1
DEEP_SEEDS = (2, 6, 13, 27)
# seeds of the full family whose cut lists reach 2 * n_integers (found by searching seeds 0 .. 2999)
FULL_SEEDS = (437,)


def _model(direction, obj, A, rows, ints=(), bins=(), names=None):
    """rows: one constraint dict per row of A ({"max": b} / {"min": b} / {"equal": b} / {"min": a, "max": b})."""
    n = len(obj)
    names = names or ["x%d" % j for j in range(n)]
    variables = {}
    for j in range(n):
        coefs = {"obj": float(obj[j])} if obj[j] != 0 else {}
        for i in range(len(rows)):
            if A[i][j] != 0:
                coefs["c%d" % i] = float(A[i][j])
        variables[names[j]] = coefs
    m = {"direction": direction, "objective": "obj",
         "constraints": {"c%d" % i: {k: float(v) for k, v in rows[i].items()} for i in range(len(rows))},
         "variables": variables}
    if ints:
        m["integers"] = [names[j] for j in ints]
    if bins:
        m["binaries"] = [names[j] for j in bins]
    return m


def _packing(rng, m, n, n_int, density=0.6, lo=1, hi=10, direction="maximize", decimals=None):
    A = rng.randint(lo, hi, size=(m, n)) * (rng.random_sample((m, n)) < density)
    if decimals is not None:
        A = np.round(A + rng.random_sample((m, n)), decimals) * (A != 0)
    b = np.maximum(A.sum(axis=1) * 0.37, 1.0).round(1)
    c = rng.randint(1, 20, size=n).astype(float)
    if direction == "minimize":  # covering: min c.x, A x >= b
        rows = [{"min": b[i]} for i in range(m)]
    else:
        rows = [{"max": b[i]} for i in range(m)]
    ints = sorted(rng.choice(n, size=n_int, replace=False).tolist())
    return _model(direction, c, A, rows, ints)


def make(family, seed, variant=0):
    """(model, options) of one record: options are the keys of the reference's Options that differ from its defaults."""
    rng = np.random.RandomState(1000 * FAMILIES.index(family) + seed)
    if family == "ties":
        n = 6 + seed % 4
        w = rng.randint(2, 9, size=n)
        ratio = rng.choice([2.0, 3.0], size=n)  # two ratios only: equal LP evaluations all over the tree
        A = [w.tolist()] + [[1 if j == k else 0 for j in range(n)] for k in range(n)]
        rows = [{"max": float(w.sum() // 2 + 1)}] + [{"max": float(rng.randint(1, 4))} for _ in range(n)]
        return _model("maximize", (ratio * w).tolist(), A, rows, range(n)), {}
    if family == "tol":
        direction = "minimize" if seed % 2 else "maximize"
        return _packing(rng, 5, 7, 5, direction=direction), {"tolerance": (0.05, 0.2, 0.01)[seed % 3]}
    if family == "iters":  # the models of deep seed 2 (queue empties after 10 nodes), tol seed 4 (threshold after 10) and
        #                    eqmm seed 3 (a solution at node 7, the break after 22)
        model, options = (make("deep", DEEP_SEEDS[0]), make("tol", 4), make("eqmm", 3))[seed]
        return model, dict(options, maxIterations=variant)
    if family == "timeout0":
        return _packing(rng, 4, 6, 4), {"timeout": 0}
    if family == "intinf":
        n = 3 + seed % 3
        a = (2 * rng.randint(1, 4, size=n)).tolist()
        A = [a] + [[1 if j == k else 0 for j in range(n)] for k in range(n)]
        rows = [{"equal": float(2 * rng.randint(2, 6) + 1)}] + [{"max": 6.0} for _ in range(n)]
        return _model("maximize", rng.randint(1, 9, size=n).tolist(), A, rows, range(n)), {}
    if family == "integral":
        n = 5 + seed % 2
        A = [[1 if j == k else 0 for j in range(n)] for k in range(n)] + [[1 if j < n // 2 + 1 else 0 for j in range(n)]]
        rows = [{"max": float(rng.randint(1, 9))} for _ in range(n)] + [{"max": float(rng.randint(3, 12))}]
        return _model("maximize", rng.randint(1, 9, size=n).tolist(), A, rows, range(n)), ({"precision": 0.0} if seed == 2 else {})
    if family == "break":
        return _packing(rng, 6, 8, 8, density=0.8), {}
    if family == "eqmm":
        n = 7
        A = rng.randint(0, 6, size=(5, n))
        x0 = rng.randint(0, 3, size=n)  # a feasible integer point
        s = A @ x0
        rows = [{"equal": float(s[0])}, {"min": float(s[1] - 2), "max": float(s[1] + 3)}, {"min": float(s[2] - 1)},
                {"max": float(s[3] + 2)}, {"min": float(s[4] - 3), "max": float(s[4] + 1)}]
        c = rng.randint(-5, 9, size=n)
        return _model("minimize" if seed % 2 else "maximize", c.tolist(), A.tolist(), rows, ints=range(4), bins=range(4, 6)), {}
    if family == "deep":
        n = 2 + seed % 2
        big = 40 + 17 * seed
        A = [[big, -(big - 1)] + [1] * (n - 2), [-(big - 1), big] + [-1] * (n - 2), [1] * n]
        rows = [{"max": 2.5 + seed % 7}, {"max": 1.5}, {"max": float(30 + 7 * seed)}]
        return _model("maximize", [1.0, 1.0] + [0.5] * (n - 2), A, rows, range(n)), {"maxIterations": 2000}
    if family == "full":  # (its own stream: the seed is the search's)
        rng = np.random.RandomState(seed)
        n, m = 3, 4
        c = rng.randint(1, 5, size=n).astype(float)
        A = rng.randint(-6, 7, size=(m, n)).astype(float)
        b = np.round(rng.random_sample(m) * 20, 1)
        A[0] = c  # the objective's own face
        b[0] = 10.5 + rng.randint(0, 10)
        return _model("maximize", c.tolist(), A.tolist(), [{"max": float(v)} for v in b], range(1 + seed % 2)), {"maxIterations": 400}
    if family == "cycles":
        n = 6
        A = np.zeros((n + 2, n))
        for k in range(n - 1):  # x_k - x_{k+1} <= 0: zero right-hand sides
            A[k, k], A[k, k + 1] = 1, -1
        A[n - 1] = rng.randint(1, 5, size=n)
        A[n] = rng.randint(1, 5, size=n)
        A[n + 1, 0] = 1
        rows = [{"max": 0.0}] * (n - 1) + [{"max": 7.5 + seed}, {"max": 9.5}, {"max": 0.0}]
        return _model("maximize", rng.randint(1, 6, size=n).tolist(), A.tolist(), rows, range(n)), {"checkCycles": True}
    if family == "negzero":  # mixed signs, zero right-hand sides, tenths: basic values that should be 0 come out a hair off
        m, n = 8, 10
        A = np.round((rng.randint(-9, 10, size=(m, n)) + 0.1 * rng.randint(0, 10, size=(m, n))) * (rng.random_sample((m, n)) < 0.6), 1)
        b = np.where(rng.random_sample(m) < 0.5, 0.0, np.round(10 * rng.random_sample(m), 1))
        A[-1] = np.abs(A[-1]) + 1  # a bounded region
        b[-1] = 25.0
        c = np.round(rng.randint(1, 20, size=n) + 0.1 * rng.randint(0, 10, size=n), 1)
        model = _model("maximize", c.tolist(), A.tolist(), [{"max": float(v)} for v in b], range(6))
        return model, {"precision": 0.0 if seed % 4 == 0 else 1e-17, "maxIterations": 60}
    if family == "mid":
        model = _packing(rng, 150, 150, 8, density=0.3)
        return model, dict({"maxIterations": 24}, **({"checkCycles": True} if seed == 1 else {}))
    if family == "big":
        model = _packing(rng, 200, 2700, 2700, density=0.05, decimals=2)
        return model, {"maxIterations": 5}
    raise ValueError(family)


def specs():
    """(family, seed, variant) of every record; variant is maxIterations for the iters family, 0 elsewhere."""
    out = []
    for fam, seeds in (("ties", range(6)), ("tol", range(6)), ("timeout0", range(2)), ("intinf", range(4)),
                       ("integral", range(3)), ("break", range(4)), ("eqmm", range(4)), ("deep", DEEP_SEEDS), ("full", FULL_SEEDS),
                       ("cycles", range(3)), ("negzero", NEGZERO_SEEDS), ("mid", range(2)), ("big", range(1))):
        out += [(fam, s, 0) for s in seeds]
    out += [("iters", s, k) for s in range(2) for k in range(1, 13)] + [("iters", 2, k) for k in (6, 7, 22)]
    return out


def label(family, seed, variant):
    return "%s-s%d" % (family, seed) + ("-i%d" % variant if family == "iters" else "")


# records whose Solution is also recorded with includeZeroVariables the other way
def zero_flip(family, seed, variant):
    return family in ("ties", "eqmm", "iters") and seed % 2 == 0
