"""Helpers of tests/test_milp_dense_model.py and tests/test_milp_dense.py (TEST INFRASTRUCTURE): what libyalps_milpdense.so
computes, restated in numpy and driven by the C oracle -- never by the code under test.

  dense_milp_tableau    what MilpDenseJob::fill writes: tableauModel's initial matrix of the equivalent model (tests/_np_dense.py's
                        rows, then one row per binary variable), and the integer columns
  equivalent_milp_model tests/_np_dense.py::equivalent_model plus "integers" / "binaries" naming the variables
  dense_solution        tests/_np_dense.py::dense_solution, extended for "timedout" (src/YALPS.ts:12)
  Call                  B MILPs of one shape with one set of integer / binary variables and one set of options
  expected              per MILP of a Call: the oracle solves the root from dense_milp_tableau, then the host search rules run
                        with the oracle as node evaluator (tests/_milp_tree.py::run_tree_search); x and objective by
                        dense_solution from the best tableau
"""
import math

import numpy as np

from tests import _milp_batch as MB
from tests import _milp_tree as MT
from tests import _np_dense as ND

NAN, INF = math.nan, math.inf
STATUS = ("optimal", "infeasible", "unbounded", "cycled", "timedout", "overflow")
NODE_LIMIT = 300  # every tree of the tables ends within this many consumed nodes
ARENA_FIRST = 128  # ... and, unless built to force a rerun, fits the first arena


def sets_of(n, integers=(), binaries=()):
    """(ascending union, ascending binaries) of 0-based variable indices; True: all n."""
    ints = list(range(n)) if integers is True else sorted(int(j) for j in integers)
    bins = list(range(n)) if binaries is True else sorted(int(j) for j in binaries)
    return sorted(set(ints) | set(bins)), bins


def dense_milp_tableau(lp, integers=(), binaries=(), maximize=False):
    """(flat row-major matrix, w, h, integer columns): ND.dense_tableau's rows, then per binary variable j in ascending order
    a row with 1.0 in column 0 and in column j + 1; the integer columns are 1 + j over the ascending union of both sets."""
    n, m_ub, m_eq = ND.shape_of(*lp)
    ints, bins = sets_of(n, integers, binaries)
    w, h0 = n + 1, 1 + m_ub + 2 * m_eq
    extra = np.zeros((len(bins), w), np.float64)
    for q, j in enumerate(bins):
        extra[q, 0] = 1.0
        extra[q, j + 1] = 1.0
    m = np.concatenate([ND.dense_tableau(*lp, maximize=maximize), extra.ravel()])
    return m, w, h0 + len(bins), [j + 1 for j in ints]


def equivalent_milp_model(lp, integers=(), binaries=(), maximize=False):
    n = len(lp[0])
    model = ND.equivalent_model(*lp, maximize=maximize)
    name = lambda given: True if given is True else ["x%d" % int(j) for j in given]
    if integers is True or len(integers):
        model["integers"] = name(integers)
    if binaries is True or len(binaries):
        model["binaries"] = name(binaries)
    assert all(k == "x%d" % j for j, k in enumerate(model["variables"])) and len(model["variables"]) == n
    return model


def dense_solution(col0, pos, var, status, result, sign, precision, n):
    """(x[n], objective): "timedout" with a result that is not NaN reads the best tableau as "optimal" does."""
    if status == "timedout":
        status = "optimal" if not math.isnan(result) else "infeasible"
    return ND.dense_solution(col0, pos, var, status, result, sign, precision, n)


class DenseRoot:
    """MB.Root for a tableau given as a matrix: the root LP solved by the oracle, what the search is given, and the tableau its
    nodes are cut from (MB.OracleEvaluator reads matrix, w, h, pos, var and opt)."""

    def __init__(self, oracle, matrix, w, h, int_cols, sign, opt):
        self.opt = MB.options(opt)
        self.w, self.h, self.int_cols, self.sign = w, h, list(int_cols), sign
        self.start = np.array(matrix, np.float64)
        self.matrix = self.start.copy()
        self.pos, self.var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
        self.status, self.result, self.n_pivots, _ = oracle.simplex(
            self.matrix, w, h, self.pos, self.var, precision=self.opt["precision"], max_pivots=self.opt["maxPivots"],
            check_cycles=self.opt["checkCycles"])

    def packed(self):
        return (self.w, self.h, self.status, self.result, self.matrix[::self.w][:self.h].copy(), self.pos, self.var, self.int_cols,
                self.sign, self.opt)


class Call:
    """One call: B MILPs of one shape, each (c, A_ub, b_ub, A_eq, b_eq) in numpy (None: no rows of that kind)."""

    def __init__(self, name, lps, integers=(), binaries=(), maximize=False, precision=1e-8, max_pivots=8192.0, check=False,
                 tolerance=0.0, max_iterations=32768.0):
        self.name, self.lps, self.maximize = name, list(lps), bool(maximize)
        self.integers, self.binaries = integers, binaries
        self.precision, self.max_pivots, self.check = precision, float(max_pivots), bool(check)
        self.tolerance, self.max_iterations = float(tolerance), float(max_iterations)
        self.n, self.m_ub, self.m_eq = ND.shape_of(*self.lps[0])
        assert all(ND.shape_of(*lp) == (self.n, self.m_ub, self.m_eq) for lp in self.lps), name
        self.ints, self.bins = sets_of(self.n, integers, binaries)
        self.w, self.h = self.n + 1, 1 + self.m_ub + 2 * self.m_eq + len(self.bins)
        self.hmax = self.h + 2 * len(self.ints)

    @property
    def options(self):
        return {"precision": self.precision, "maxPivots": self.max_pivots, "checkCycles": self.check, "tolerance": self.tolerance,
                "maxIterations": self.max_iterations}

    def stacked(self):
        """(c [B, n], A_ub [B, m_ub, n], b_ub [B, m_ub], A_eq, b_eq), None where there are no such rows."""
        out = []
        for k, shape in enumerate(((self.n,), (self.m_ub, self.n), (self.m_ub,), (self.m_eq, self.n), (self.m_eq,))):
            rows = self.m_ub if k in (1, 2) else self.m_eq
            out.append(None if k and not rows else np.stack([np.asarray(lp[k], np.float64).reshape(shape) for lp in self.lps]))
        return out

    def roots(self, oracle):
        sign = 1.0 if self.maximize else -1.0
        return [DenseRoot(oracle, *dense_milp_tableau(lp, self.integers, self.binaries, self.maximize), sign, self.options)
                for lp in self.lps]

    def models(self):
        return [equivalent_milp_model(lp, self.integers, self.binaries, self.maximize) for lp in self.lps]


def expected(nat, oracle, call, arena=None, arena_max=None):
    """Per MILP of `call` a dict: status, result, nodes, node_pivots, root_pivots, height, col0, pos, var, x, objective, and
    `trace`, the consumed nodes in pop order as (eval bits, cuts, status, result bits, pivots, height)."""
    roots = call.roots(oracle)
    out, nodes, _, reruns = MT.run_tree_search(nat, oracle, roots, arena=arena, arena_max=arena_max)
    sign = 1.0 if call.maximize else -1.0
    rows = []
    for root, (status, result, height, col0, pos, var, used, _), seq in zip(roots, out, nodes):
        x, objective = dense_solution(col0, pos, var, status, result, sign, call.precision, call.n)
        trace = [(nd["eval"], tuple((int(s), int(v), c) for s, v, c in nd["cuts"]), nd["status"], hex_or_nan(nd["result"]), int(nd["n_pivots"]),
                  root.h + len(nd["cuts"])) for nd in seq]
        rows.append(dict(status=status, result=result, nodes=used, node_pivots=sum(t[4] for t in trace), root_pivots=root.n_pivots,
                         height=height, col0=col0, pos=pos, var=var, x=x, objective=objective, trace=trace, reruns=reruns))
    return rows


def hex_or_nan(h):
    """A number's hex spelling (tests/_bnc.py::hexd) with every NaN spelled "nan"."""
    return "nan" if math.isnan(float(np.frombuffer(bytes.fromhex(h), ">f8")[0])) else h


def words(a):
    """A float64 array's words with every NaN counted as one value."""
    a = np.array(a, np.float64, ndmin=1)
    a[np.isnan(a)] = np.nan
    return a.view(np.int64)


# ------------------------------------------------------------------------------------------------ the MILPs

def packing_dense(m, n, n_int, seed, density=0.6, lo=1, hi=10):
    """tests/_milps.py::_packing written densely: (lp, ascending integer variables) of maximize c . x, A x <= b."""
    rng = np.random.RandomState(seed)
    A = (rng.randint(lo, hi, size=(m, n)) * (rng.random_sample((m, n)) < density)).astype(np.float64)
    b = np.maximum(A.sum(axis=1) * 0.37, 1.0).round(1)
    c = rng.randint(1, 20, size=n).astype(float)
    ints = sorted(rng.choice(n, size=n_int, replace=False).tolist())
    return (c, A, b, None, None), ints


def of_model(model):
    """The dense operands of a model whose rows are all {"max"}, as tests/_milps.py::_packing makes them: (lp, integers)."""
    names = list(model["variables"])
    rows = list(model["constraints"])
    assert all(set(model["constraints"][r]) == {"max"} for r in rows) and model["direction"] == "maximize"
    c = np.array([model["variables"][k].get(model["objective"], 0.0) for k in names], np.float64)
    A = np.array([[model["variables"][k].get(r, 0.0) for k in names] for r in rows], np.float64).reshape(len(rows), len(names))
    b = np.array([model["constraints"][r]["max"] for r in rows], np.float64)
    return (c, A, b, None, None), sorted(names.index(k) for k in model.get("integers", ()))
