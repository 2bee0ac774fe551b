"""An independent statement of every call of the tensor solvers (TEST INFRASTRUCTURE): linprog_batch, linprog_objective_bounds,
milp_batch and milp_batch_free, from the caller's own terms -- c, A_ub, b_ub, A_eq, b_eq, lb, ub, upper, free, integers, binaries,
maximize -- and nothing else.  This module imports nothing from yalps_amd and nothing from tests/_np_*: the other tests show that
the kernels do what tests/_np_*.py wrote down; this one is for whether what they wrote down is the problem the caller stated.

  scipy_lp(group, case)      scipy.optimize.linprog(method="highs") on the stated LP, answered in the caller's direction
  scipy_milp(group, case)    scipy.optimize.milp on the stated MILP
  certificate(...)           the residuals of the optimality conditions of an answer, in the caller's terms; no solver
  unique(group, case, ans)   whether the LP has one x and one dual solution (only such LPs are compared value by value)
  lp_groups(), milp_groups(), ending_groups(kind), generate(group)
                             the groups: cases of one shape and one set of index lists, which one batched call takes
  lp_differences, milp_differences, MEASURED, TOL
                             the comparison of an answer with a recorded one, the measured figures and the bounds made of them
  record                     `python -m tests._independent record` writes tests/golden/independent_{lp,milp}.json.gz: the operands
                             (float64 words as hex; a matrix that a float16 word holds exactly, as those) and HiGHS's answers.
                             Which LPs get in is unique()'s decision; which MILPs, the oracle-driven search's ("optimal" within
                             the budget) -- tests/_independent_models.py is imported for that inside record() alone.  The code
                             under test decides nothing.
  load(kind)                 the recorded groups; needs numpy only (the GPU tests read the files and never import scipy)

A group is a dict: name, family, fn, n, m_ub, m_eq, upper (None: no ub; True; or a list), free (a list, or True), integers,
binaries, maximize, max_iterations, and cases -- each a dict of the seven operands (None where absent) and, once recorded, "answer".
"""
import gzip
import json
import math
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = {"lp": os.path.join(GOLDEN, "independent_lp.json.gz"), "milp": os.path.join(GOLDEN, "independent_milp.json.gz")}
OPERANDS = ("c", "A_ub", "b_ub", "A_eq", "b_eq", "lb", "ub")
MARGINALS = ("ineqlin", "eqlin", "lower", "upper")
TIGHT, MARGIN = 1e-7, 1e-6    # unique(): a slack below TIGHT is tight; slack and marginal have to clear MARGIN on their side
MAX_DROPPED = 0.10            # of the generated LPs of a family
INF = math.inf


# ------------------------------------------------------------------------------------------------ the sets, in the caller's terms

def upper_idx(group):
    """The variables whose ub entry the call reads: none without ub; with True all of them but, in a MILP, the binary ones."""
    if group["upper"] is None:
        return []
    if group["upper"] is True:
        return [j for j in range(group["n"]) if j not in group["binaries"]]
    return sorted(group["upper"])


def free_idx(group):
    if group["free"] is True:
        return [j for j in range(group["n"]) if j not in group["binaries"]]
    return sorted(group["free"])


def bounds_of(group, case):
    """(lower[n], upper[n]) as the documentation states them: a free variable has no lower bound whatever lb holds, a binary
    one lies in [0, 1] whatever lb and ub hold, ub counts at the variables `upper` names, x >= 0 stands where lb is absent."""
    n = group["n"]
    lo = np.zeros(n) if case["lb"] is None else np.array(case["lb"], np.float64)
    hi = np.full(n, INF)
    for j in upper_idx(group):
        hi[j] = case["ub"][j]
    for j in free_idx(group):
        lo[j] = -INF
    for j in group["binaries"]:
        lo[j], hi[j] = 0.0, 1.0
    return lo, hi


# ------------------------------------------------------------------------------------------------ HiGHS

def scipy_lp(group, case):
    from scipy.optimize import linprog
    lo, hi = bounds_of(group, case)
    bounds = [(None if l == -INF else float(l), None if h == INF else float(h)) for l, h in zip(lo, hi)]
    sign = -1.0 if group["maximize"] else 1.0
    kw = dict(A_ub=case["A_ub"], b_ub=case["b_ub"], A_eq=case["A_eq"], b_eq=case["b_eq"], bounds=bounds, method="highs")
    res = linprog(sign * case["c"], **kw)
    if res.status == 4:  # HiGHS's "infeasible or unbounded": presolve off decides, or the case is not kept
        res = linprog(sign * case["c"], options={"presolve": False}, **kw)
    status = {0: "optimal", 2: "infeasible", 3: "unbounded"}.get(res.status, "undecided")
    out = dict(status=status)
    if status == "optimal":
        idx = upper_idx(group)
        out.update(x=np.array(res.x), objective=float(sign * res.fun), ineqlin=sign * np.asarray(res.ineqlin.marginals, np.float64).reshape(-1),
                   eqlin=sign * np.asarray(res.eqlin.marginals, np.float64).reshape(-1), lower=sign * np.asarray(res.lower.marginals, np.float64),
                   upper=sign * np.asarray(res.upper.marginals, np.float64)[idx])
        for k in MARGINALS:
            out[k] = out[k] + 0.0
    return out


def scipy_milp(group, case):
    """HiGHS holds x integral to 1e-6 only, so the recorded objective is c . x with x rounded at the integer variables.

    The HiGHS of scipy 1.15.3 is run twice, with presolve and without, because neither run can be trusted alone on MILPs with
    continuous variables.  With presolve it answers the first hand-made ending -- maximise x0 + x1 / 2 under x0 + x1 <= 4.5,
    x0 - x1 <= 2.25, -1.5 <= x0 <= 3.25, 0.5 <= x1 <= 2.75, x1 integer -- with (3, 1) and 3.5 as "optimal", though (3.25, 1)
    satisfies every row and bound and gives 3.75; without presolve it calls several generated MILPs infeasible, or ends below
    the optimum, where the other run returns a better point.  A returned point that certificate() finds feasible and integral
    proves its objective attainable whatever else the solver says, so the answer is the better of the two such points; without
    any, "infeasible" or "unbounded" where a run says so and the other does not say the opposite (HiGHS's combined "infeasible
    or unbounded" status says neither), else "undecided"."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    lo, hi = bounds_of(group, case)
    n = group["n"]
    whole = sorted(set(group["integers"]) | set(group["binaries"]))
    integrality = np.zeros(n)
    integrality[whole] = 1
    cons = []
    if case["A_ub"] is not None:
        cons.append(LinearConstraint(case["A_ub"], -np.inf, case["b_ub"]))
    if case["A_eq"] is not None:
        cons.append(LinearConstraint(case["A_eq"], case["b_eq"], case["b_eq"]))
    sign = -1.0 if group["maximize"] else 1.0
    names, points = [], []
    for presolve in (True, False):
        res = milp(sign * case["c"], constraints=cons, integrality=integrality, bounds=Bounds(lo, hi), options={"presolve": presolve})
        names.append({0: "optimal", 2: "infeasible", 3: "unbounded"}.get(res.status, "undecided"))
        if res.status == 0:
            x = np.array(res.x)
            x[whole] = np.round(x[whole])
            objective = float(case["c"] @ x)
            if certificate(group, case, x, objective, whole=whole)["primal"] <= MARGIN:
                points.append((sign * objective, x, objective))
    if points:
        _, x, objective = min(points, key=lambda p: p[0])
        return dict(status="optimal", x=x, objective=objective)
    decided = {name for name in names if name in ("infeasible", "unbounded")}
    return dict(status=decided.pop() if len(decided) == 1 else "undecided")


# ------------------------------------------------------------------------------------------------ the certificate

def certificate(group, case, x, objective, marginals=None, whole=()):
    """The residuals of an answer in the caller's terms, each a non-negative number that is 0 for an exact optimal answer:
    "primal" (rows and bounds), "objective" (|objective - c . x|), "integral" (distance from a whole number at `whole`), and
    with marginals = (ineqlin, eqlin, lower, upper): "sign" (a marginal on the wrong side for the direction; at a free variable
    any `lower` at all), "reduced" (lower against c - A_ub^T y - A_eq^T z - scatter(upper)) and "slackness" (marginal times slack)."""
    x = np.asarray(x, np.float64)
    lo, hi = bounds_of(group, case)
    slack_ub = case["b_ub"] - case["A_ub"] @ x if case["A_ub"] is not None else np.zeros(0)
    gap_eq = case["A_eq"] @ x - case["b_eq"] if case["A_eq"] is not None else np.zeros(0)
    top = lambda a: float(np.max(a)) if np.size(a) else 0.0
    out = dict(primal=max(top(-slack_ub), top(np.abs(gap_eq)), top(lo - x), top(x - hi), 0.0),
               objective=abs(float(objective) - float(case["c"] @ x)),
               integral=top(np.abs(x[list(whole)] - np.round(x[list(whole)]))))
    if marginals is None:
        return out
    y, z, lower, upper = (np.asarray(a, np.float64) for a in marginals)
    idx = upper_idx(group)
    s = -1.0 if group["maximize"] else 1.0  # minimising: a looser row or upper bound lowers the objective, a looser lower bound too
    fr = free_idx(group)
    held = [j for j in range(group["n"]) if j not in fr]
    out["sign"] = max(top(s * y), top(s * upper), top(-s * lower[held]), top(np.abs(lower[fr])), 0.0)
    reduced = np.array(case["c"], np.float64)
    if y.size:
        reduced = reduced - case["A_ub"].T @ y
    if z.size:
        reduced = reduced - case["A_eq"].T @ z
    scatter = np.zeros(group["n"])
    scatter[idx] = upper
    out["reduced"] = top(np.abs(lower - (reduced - scatter)))
    out["slackness"] = max(top(np.abs(y * slack_ub)), top(np.abs(lower[held] * (x - lo)[held])), top(np.abs(upper * (hi - x)[idx])), 0.0)
    return out


def unique(group, case, answer):
    """True where exactly n constraints or bounds are tight at x, each with a marginal beyond MARGIN, and every other one is slack
    by more than MARGIN with a marginal below TIGHT: a non-degenerate vertex with a non-degenerate dual, so one x and one y."""
    if answer["status"] != "optimal":
        return False
    x = answer["x"]
    lo, hi = bounds_of(group, case)
    held = [j for j in range(group["n"]) if lo[j] > -INF]
    idx = upper_idx(group)
    pairs = []
    if case["A_ub"] is not None:
        pairs += list(zip(case["b_ub"] - case["A_ub"] @ x, answer["ineqlin"]))
    if case["A_eq"] is not None:
        pairs += list(zip(np.abs(case["A_eq"] @ x - case["b_eq"]), answer["eqlin"]))
    pairs += list(zip((x - lo)[held], answer["lower"][held])) + list(zip((hi - x)[idx], answer["upper"]))
    tight = 0
    for slack, marginal in pairs:
        if slack < TIGHT and abs(marginal) > MARGIN:
            tight += 1
        elif not (slack > MARGIN and abs(marginal) < TIGHT):
            return False
    return tight == group["n"] and all(abs(answer["lower"][j]) < TIGHT for j in free_idx(group))


# ------------------------------------------------------------------------------------------------ the comparison

# The largest |host model - recorded HiGHS answer| over the recorded cases, per family and size and per quantity, and under "own ..."
# the largest certificate residual of the host model's own answer -- measured by tests/test_independent_model.py, which prints them
# and fails if one is exceeded, rounded up to two digits.  x and the objective are rounded to precision = 1e-8, which alone is
# up to 5e-9; the marginals are not rounded.  The residuals "own primal", "own objective" and "own slackness" are those of an x
# rounded to 1e-8 in rows whose coefficients sum to tens (small) or hundreds (large).  The endings are exact in binary.
MEASURED = {
    ("LP plain", "small"): {"x": 5e-09, "objective": 5e-09, "ineqlin": 4e-14, "eqlin": 2.4e-14, "lower": 3.9e-14, "upper": 0.0,
                            "own primal": 3.2e-08, "own objective": 7.3e-08, "own sign": 0.0, "own reduced": 8.6e-14, "own slackness": 6.3e-08},
    ("LP plain", "large"): {"x": 5e-09, "objective": 5.1e-09, "ineqlin": 1.2e-10, "eqlin": 3.1e-12, "lower": 1.4e-09, "upper": 0.0,
                            "own primal": 1.7e-07, "own objective": 2.7e-06, "own sign": 0.0, "own reduced": 2.1e-11, "own slackness": 2.1e-07},
    ("LP bounded", "small"): {"x": 5e-09, "objective": 5e-09, "ineqlin": 4.5e-14, "eqlin": 3.3e-14, "lower": 2.8e-14, "upper": 2e-14,
                              "own primal": 3.2e-08, "own objective": 1.1e-07, "own sign": 0.0, "own reduced": 7.9e-14, "own slackness": 4.4e-08},
    ("LP bounded", "large"): {"x": 5e-09, "objective": 4.6e-09, "ineqlin": 1.3e-11, "eqlin": 9.1e-13, "lower": 9.7e-11, "upper": 4.7e-11,
                              "own primal": 1.7e-07, "own objective": 3.8e-06, "own sign": 0.0, "own reduced": 2.7e-11, "own slackness": 2.1e-07},
    ("LP free", "small"): {"x": 5e-09, "objective": 5e-09, "ineqlin": 1.3e-13, "eqlin": 1.4e-13, "lower": 1.1e-13, "upper": 4.5e-13,
                           "own primal": 3.7e-08, "own objective": 9.7e-08, "own sign": 2.3e-16, "own reduced": 1.6e-13, "own slackness": 7.5e-08},
    ("LP free", "large"): {"x": 5.1e-09, "objective": 4e-09, "ineqlin": 3.5e-11, "eqlin": 3.4e-12, "lower": 5.6e-10, "upper": 2.3e-10,
                           "own primal": 2.2e-07, "own objective": 5.1e-06, "own sign": 5.6e-15, "own reduced": 3.5e-11, "own slackness": 2.4e-07},
    ("endings", "small"): {"x": 0.0, "objective": 0.0, "ineqlin": 0.0, "eqlin": 0.0, "lower": 0.0, "upper": 0.0, "own primal": 0.0,
                           "own objective": 0.0, "own sign": 0.0, "own reduced": 0.0, "own slackness": 0.0, "own integral": 0.0},
    ("MILP plain", "small"): {"objective": 5e-09, "own primal": 2.9e-08, "own objective": 1.1e-08, "own integral": 0.0},
    ("MILP plain", "large"): {"objective": 1.9e-09, "own primal": 8.6e-08, "own objective": 1.7e-08, "own integral": 0.0},
    ("MILP bounded", "small"): {"objective": 5e-09, "own primal": 2.7e-08, "own objective": 1.5e-08, "own integral": 0.0},
    ("MILP bounded", "large"): {"objective": 1.4e-09, "own primal": 1.3e-07, "own objective": 2.3e-08, "own integral": 0.0},
    ("MILP free", "small"): {"objective": 4.9e-09, "own primal": 2.2e-08, "own objective": 1.1e-08, "own integral": 0.0},
    ("MILP free", "large"): {"objective": 3.7e-09, "own primal": 2.4e-08, "own objective": 2.2e-08, "own integral": 0.0},
}
# Each bound is twice the measured figure: the factor covers another HiGHS build or BLAS.  The GPU tests use the same bounds -- the
# device equals the host model bit for bit, which the other tests of each function show.
TOL = {key: {q: 2.0 * v for q, v in row.items()} for key, row in MEASURED.items()}


def tolerance(group):
    return TOL[(group["family"], bucket(group))]


def bucket(group):
    """Tolerances are kept per family and per size: "small" (n <= 8) and "large" (the lanes' shapes and the kernel forms)."""
    return "small" if group["n"] <= 8 else "large"


def lp_differences(group, case, got, want):
    """{quantity: the largest |got - want|} of an LP answer against the recorded one -- inf for another status or a non-finite
    entry -- and, prefixed "own ", the certificate's residuals of `got` itself."""
    if got["status"] != want["status"]:
        return {"status": INF}
    if want["status"] != "optimal":
        return {}
    out = {}
    for k in ("x", "objective") + MARGINALS:
        d = np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64))
        out[k] = (float(np.max(d)) if np.isfinite(d).all() else INF) if d.size else 0.0
    cert = certificate(group, case, got["x"], got["objective"], [got[k] for k in MARGINALS])
    out.update({"own " + k: (v if math.isfinite(v) else INF) for k, v in cert.items() if k != "integral"})
    return out


def milp_differences(group, case, got, want):
    """The same for a MILP: the objective against the recorded one, and the certificate of got's own x -- rows, bounds,
    integrality at the integer and binary variables, objective = c . x."""
    if got["status"] != want["status"]:
        return {"status": INF}
    if want["status"] != "optimal":
        return {}
    d = abs(float(got["objective"]) - want["objective"])
    cert = certificate(group, case, got["x"], got["objective"], whole=sorted(set(group["integers"]) | set(group["binaries"])))
    out = {"objective": d if math.isfinite(d) else INF}
    out.update({"own " + k: (v if math.isfinite(v) else INF) for k, v in cert.items()})
    return out


def merged(into, diffs):
    for k, v in diffs.items():
        into[k] = max(into.get(k, 0.0), v)
    return into


def within(diffs, tol):
    """Every difference at or below its bound; a quantity without a bound (a status that differs) fails."""
    return all(k in tol and v <= tol[k] for k, v in diffs.items())


# ------------------------------------------------------------------------------------------------ the generators

def _matrix(rng, m, n, grain):
    """Entries of -2 .. 4: continuous, or for the large shapes in steps of `grain` (the file stays small; b and c stay continuous)."""
    if grain is None:
        return rng.uniform(-2.0, 4.0, (m, n))
    a = rng.integers(int(-2 / grain), int(4 / grain) + 1, (m, n)).astype(np.float64) * grain
    return a * (rng.random((m, n)) < 0.25) + 0.0 if m > 1000 else a  # (the tall shapes: three entries of four are zero)


def _rhs(b, grain):
    """The right-hand sides of a large shape in steps of 2^-24: generic still, and half the words in the file."""
    return b if grain is None else np.round(b * 2.0 ** 24) / 2.0 ** 24


def lp_case(rng, group, grain=None):
    """A generic LP with an optimum: feasible at a point x0 inside every row and bound (negative at some free variables), and c
    made from non-negative multipliers of some rows and bounds, so that its dual is feasible too.  What the call must not read
    holds a value that would change the answer if it were read: lb at a free variable lies above x0, ub at a variable `upper`
    does not list lies below the lower bound."""
    n, m_ub, m_eq = group["n"], group["m_ub"], group["m_eq"]
    idx, fr = upper_idx(group), free_idx(group)
    held = [j for j in range(n) if j not in fr]
    lb = rng.uniform(-2.0, 1.0, n) if group["has_lb"] else None
    low = np.zeros(n) if lb is None else lb.copy()
    x0 = low + rng.uniform(0.25, 2.0, n)
    x0[fr] = rng.normal(0.0, 2.0, len(fr))
    ub = None
    if group["upper"] is not None:
        ub = low - 1.0
        ub[fr] = x0[fr] - 1.0
        ub[idx] = x0[idx] + rng.uniform(0.25, 2.0, len(idx))
    if lb is not None:
        lb[fr] = x0[fr] + rng.uniform(0.5, 1.5, len(fr))
    A_ub = _matrix(rng, m_ub, n, grain)
    b_ub = _rhs(A_ub @ x0 + rng.uniform(0.1, 1.0, m_ub), grain)
    A_eq = _matrix(rng, m_eq, n, grain) if m_eq else None
    # n multipliers in all -- the equalities', and n - m_eq of rows and bounds picked at random, one bound per variable at the
    # most: c is a generic point of a cone of full dimension, so the optimum is one vertex (fewer would leave a face of optima)
    g = A_eq.T @ rng.normal(0.0, 1.0, m_eq) if m_eq else np.zeros(n)
    bound = [j for j in range(n) if j in held or j in idx]
    for t in rng.permutation(m_ub + len(bound))[:n - m_eq]:
        if t < m_ub:
            g += A_ub[t] * rng.uniform(0.5, 2.0)
            continue
        j = bound[t - m_ub]
        if j in idx and (j not in held or rng.random() < 0.5):
            g[j] += rng.uniform(0.5, 2.0)  # u >= 0 of x <= ub
        else:
            g[j] -= rng.uniform(0.5, 2.0)  # r >= 0 of x >= lb
    c = g if group["maximize"] else -g
    return dict(c=c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=None if A_eq is None else _rhs(A_eq @ x0, grain), lb=lb, ub=ub)


def milp_case(rng, group, grain=None):
    """A generic MILP around a point x0 that is whole where it has to be.  Maximised objectives are positive and the first row is
    positive, so that with the lower bounds it holds every variable; minimised ones are their negation.  lb is fractional at the
    integer variables, and where two of them are not free the objective pushes the last of those down onto it.  Every second free
    variable is pushed down too and each is held by a guard row -x[j] <= d[j], d whole at an integer variable (a free integer
    variable held at a fraction starts the documented chain that ends at max_iterations).  group["twin"]: the first free integer
    variable gets c = 0 and a guard at a fraction -- its optimum is a negative integer that only a cut on the twin reaches."""
    n, m_ub, m_eq = group["n"], group["m_ub"], group["m_eq"]
    ints, bins = sorted(group["integers"]), sorted(group["binaries"])
    idx, fr = upper_idx(group), free_idx(group)
    m_gen = m_ub - len(fr)
    lb = rng.uniform(-1.5, 1.5, n) if group["has_lb"] else None
    low = np.zeros(n) if lb is None else lb.copy()
    low[ints] = np.ceil(low[ints])
    low[bins] = 0.0
    low[fr] = 0.0
    width = rng.uniform(1.25, 4.25, n)
    x0 = low + width * rng.random(n)
    x0[ints] = low[ints] + rng.integers(0, 2, len(ints))
    x0[bins] = rng.integers(0, 2, len(bins))
    ub = None
    if group["upper"] is not None:
        ub = low - 1.0
        ub[idx] = (low + width)[idx]
    A = _matrix(rng, m_gen, n, grain)
    if m_gen:
        A[0] = rng.uniform(0.5, 1.5, n)
    if m_gen > 1000:  # (among thousands of rows one would hold a free integer variable at a fraction: they leave it alone)
        A[1:, [j for j in fr if j in ints]] = 0.0
    b = _rhs(A @ x0 + rng.random(m_gen), grain)
    c = rng.uniform(0.5, 1.5, n)
    own = [j for j in ints if j not in fr]
    if lb is not None and (len(own) >= 2 or group.get("twin")):  # (the others are pushed up against the rows: those are the fractions the trees branch on)
        c[own[-1]] *= -1.0
    c[fr[::2]] *= -1.0
    drop = np.array([1.0 + t % 3 if j in ints else 0.5 + rng.random() for t, j in enumerate(fr)])
    if group.get("twin"):
        j = next(j for j in fr if j in ints)
        c[j] = 0.0
        drop[fr.index(j)] += 0.5
    guards = np.zeros((len(fr), n))
    guards[np.arange(len(fr)), fr] = -1.0
    A_eq = _matrix(rng, m_eq, n, grain) if m_eq else None
    if not group["maximize"]:
        c = -c
    return dict(c=c, A_ub=np.concatenate([A, guards]), b_ub=np.concatenate([b, drop - low[fr]]), A_eq=A_eq,
                b_eq=None if A_eq is None else A_eq @ x0, lb=lb, ub=ub)


def _group(name, family, fn, n, m_ub, m_eq, has_lb=False, upper=None, free=(), integers=(), binaries=(), maximize=False, B=16, grain=None,
           max_iterations=None, twin=False):
    return dict(name=name, family=family, fn=fn, n=n, m_ub=m_ub, m_eq=m_eq, has_lb=has_lb, upper=upper if upper in (None, True) else list(upper),
                free=free if free is True else list(free),
                integers=list(integers), binaries=list(binaries), maximize=maximize, B=B, grain=grain, max_iterations=max_iterations, twin=twin)


LANES = (63, 64, 65, 129)     # the lanes of shift_sum go round at 64


def lp_groups():
    """The LP groups, not yet generated.  The large shapes are the geometry of tests/_lp_dense_free.py and
    tests/_milp_dense_free.SHAPES (h x w of the tableau): 100 x 99, the LDS form at 1024 lanes; 160 x 152, the HBM form; 8170 x 31,
    the aux form."""
    P, Bd, F, fn = "LP plain", "LP bounded", "LP free", "linprog_batch"
    G = [_group("plain n=3", P, fn, 3, 4, 0), _group("plain n=5 eq max", P, fn, 5, 4, 1, maximize=True),
         _group("plain n=8 eq", P, fn, 8, 6, 2), _group("plain n=6 max", P, fn, 6, 5, 0, maximize=True),
         _group("plain 100x99", P, fn, 98, 99, 0, maximize=True, B=2, grain=1.0 / 16),
         _group("plain 160x152", P, fn, 151, 155, 2, B=1, grain=1.0 / 16),
         _group("plain 8170x31", P, fn, 30, 8169, 0, maximize=True, B=1, grain=1.0 / 8),
         _group("bounded n=4 subset max", Bd, fn, 4, 4, 0, True, (0, 2), maximize=True),
         _group("bounded n=7 subset eq", Bd, fn, 7, 5, 2, True, (1, 2, 6)),
         _group("bounded n=5 ub alone eq max", Bd, fn, 5, 4, 1, False, True, maximize=True),
         _group("bounded n=6 lb alone", Bd, fn, 6, 5, 0, True),
         _group("bounded n=3 box eq", Bd, fn, 3, 3, 1, True, True),
         _group("bounded n=63", Bd, fn, 63, 8, 1, True, tuple(range(0, 63, 5)), maximize=True, B=2),
         _group("bounded n=65", Bd, fn, 65, 8, 0, True, True, B=2),
         _group("bounded 100x99", Bd, fn, 98, 93, 1, True, (0, 1, 2, 97), B=2, grain=1.0 / 16),
         _group("bounded 160x152", Bd, fn, 151, 153, 0, True, tuple(range(6)), maximize=True, B=1, grain=1.0 / 16),
         _group("bounded 8170x31", Bd, fn, 30, 8164, 1, True, (0, 1, 29), B=1, grain=1.0 / 8),
         _group("free n=5 box", F, fn, 5, 4, 0, True, True, (1, 4)),
         _group("free n=6 in upper eq max", F, fn, 6, 5, 2, True, (0, 2, 5), (2, 3), maximize=True),
         _group("free n=4 no bounds eq max", F, fn, 4, 5, 1, free=(0, 3), maximize=True),
         _group("free n=3 all free", F, fn, 3, 5, 0, free=True),
         _group("free n=8 all free box eq max", F, fn, 8, 7, 1, True, (0, 3, 4), True, maximize=True),
         _group("free n=64", F, fn, 64, 8, 1, True, tuple(range(1, 64, 7)), (0, 8, 63), B=2),
         _group("free n=129", F, fn, 129, 9, 0, True, True, (0, 64, 128), maximize=True, B=2),
         _group("free 100x99", F, fn, 92, 95, 0, True, (0, 1, 2, 91), (0, 17, 35, 54, 72, 91), maximize=True, B=2, grain=1.0 / 16),
         _group("free 160x152", F, fn, 144, 151, 1, True, (0, 1, 2, 3, 4, 143), (0, 24, 48, 71, 95, 119, 143), B=1, grain=1.0 / 16),
         _group("free 8170x31", F, fn, 26, 8166, 0, True, (0, 1, 25), (0, 8, 17, 25), maximize=True, B=1, grain=1.0 / 8)]
    return G


def milp_groups():
    P, Bd, F = "MILP plain", "MILP bounded", "MILP free"
    kw = dict(maximize=True, B=24, max_iterations=400)
    G = [_group("milp n=4", P, "milp_batch", 4, 3, 0, integers=(0, 2), binaries=(1,), **kw),
         _group("milp n=6 eq", P, "milp_batch", 6, 4, 1, integers=(0, 3, 5), binaries=(2,), **kw),
         _group("milp n=8 min", P, "milp_batch", 8, 5, 0, integers=(1, 4, 6, 7), binaries=(0, 3), **dict(kw, maximize=False)),
         _group("milp 100x99", P, "milp_batch", 98, 98, 0, integers=(96, 97), binaries=(0,), **dict(kw, B=2, max_iterations=200, grain=1.0 / 16)),
         _group("bounded milp n=4 subset", Bd, "milp_batch", 4, 3, 0, True, (0, 2), integers=(0, 3), binaries=(1,), **kw),
         _group("bounded milp n=6 eq", Bd, "milp_batch", 6, 4, 1, True, True, integers=(0, 3, 5), binaries=(2,), **kw),
         _group("bounded milp n=7 ub alone min", Bd, "milp_batch", 7, 4, 0, False, True, integers=(1, 4, 6), binaries=(0,), **dict(kw, maximize=False)),
         _group("bounded milp n=5 lb alone", Bd, "milp_batch", 5, 4, 0, True, integers=(0, 2, 4), **kw),
         _group("bounded milp 160x152", Bd, "milp_batch", 151, 155, 0, True, (0, 1, 2, 3), integers=(149, 150),
                **dict(kw, B=2, max_iterations=200, grain=1.0 / 16)),
         _group("free milp n=5", F, "milp_batch_free", 5, 5, 0, True, True, (0, 1), integers=(0, 3, 4), **kw),
         _group("free milp n=6 eq", F, "milp_batch_free", 6, 6, 1, True, (0, 3, 5), (0, 1, 4), integers=(0, 3, 4, 5), binaries=(2,), **kw),
         _group("free milp n=5 all free min", F, "milp_batch_free", 5, 8, 0, free=True, integers=(0, 3), binaries=(2,), **dict(kw, maximize=False)),
         _group("free milp n=4 twin", F, "milp_batch_free", 4, 4, 0, True, True, (0, 1), integers=(0, 3), twin=True, **dict(kw, B=48)),
         _group("free milp 8170x31", F, "milp_batch_free", 26, 8165, 0, True, (0, 1, 2, 3), (0, 8, 23, 24), integers=(23, 25),
                **dict(kw, B=2, max_iterations=200, grain=1.0 / 16))]
    return G


def _seed(group):
    return [20270201, group["n"], group["m_ub"], group["m_eq"], sum(map(ord, group["name"]))]


def generate(group):
    """The group with its B generated cases."""
    rng = np.random.default_rng(_seed(group))
    make = lp_case if group["fn"] == "linprog_batch" else milp_case
    out = {k: v for k, v in group.items() if k not in ("B", "grain")}
    out["generated"] = group["B"]
    out["cases"] = [make(rng, group, group["grain"]) for _ in range(group["B"])]
    return out


def _hand(name, fn, rows, **sets):
    """A hand-made group: rows of (c, A_ub, b_ub, lb, ub)."""
    f = lambda v: None if v is None else np.array(v, np.float64)
    n, m_ub = len(rows[0][0]), len(rows[0][2])
    g = _group(name, "endings", fn, n, m_ub, 0, has_lb=rows[0][3] is not None, B=len(rows), **sets)
    out = {k: v for k, v in g.items() if k not in ("B", "grain")}
    out["generated"] = len(rows)
    out["cases"] = [dict(c=f(c), A_ub=f(A), b_ub=f(b), A_eq=None, b_eq=None, lb=f(lb), ub=f(ub)) for c, A, b, lb, ub in rows]
    return out


def ending_groups(kind):
    """The endings by hand, two variables and two rows each, maximised: x0 + x1 <= 4.5 and x0 - x1 <= 2.25 around the box
    [-1.5, 3.25] x [0.5, 2.75].  Row 0 of each group is the feasible, bounded one; then
      "crossed"   infeasible by ub[0] < lb[0];        "rows"      infeasible by x0 + x1 <= 4.5 against -x0 - x1 <= -5
      "free"      unbounded through the free x0, which the objective pushes down and nothing holds
      "unlisted"  unbounded through x1, whose ub `upper` does not list, once the first row no longer holds it (in the LP the objective
                  pulls at x1 hardest, so its own column is the one the simplex finds unbounded)."""
    A, b, lb, ub = [[1.0, 1.0], [1.0, -1.0]], [4.5, 2.25], [-1.5, 0.5], [3.25, 2.75]
    fn = "linprog_batch" if kind == "lp" else "milp_batch_free"
    sets = dict(maximize=True) if kind == "lp" else dict(maximize=True, integers=(1,), max_iterations=50)
    bounded = [([1.0, 0.5], A, b, lb, ub),
               ([1.0, 0.5], A, b, lb, [-1.75, 2.75]),                               # crossed
               ([1.0, 0.5], [[1.0, 1.0], [-1.0, -1.0]], [4.5, -5.0], lb, [9.0, 9.0])]     # rows
    freed = [([-1.0, 0.5], [[1.0, 1.0], [-1.0, 1.0]], b, lb, ub),                   # -x0 + x1 <= 2.25 holds x0 from below
             ([-1.0, 0.5], A, b, lb, ub)]                                           # free: nothing holds x0 from below
    pull = [0.5, 1.0] if kind == "lp" else [1.0, 0.5]  # (HiGHS decides the MILP "unbounded" with the second objective only)
    unlisted = [(pull, A, b, lb, ub),
                (pull, [[1.0, 0.0], [1.0, -1.0]], b, lb, ub)]                       # unlisted: x1 goes up for ever
    return [_hand("endings bounded", fn if kind == "lp" else "milp_batch", bounded, upper=True, **sets),
            _hand("endings free", fn, freed, upper=(1,), free=(0,), **sets),
            _hand("endings unlisted", fn if kind == "lp" else "milp_batch", unlisted, upper=(0,), **sets)]


# ------------------------------------------------------------------------------------------------ the files

def _pack(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a, "<f8")
    half = a.astype("<f2")  # (the large shapes' matrices lie on a grain that a narrower word holds exactly: a smaller file)
    if a.size > 2048 and np.array_equal(half.astype("<f8"), a) and not np.signbit(a[a == 0.0]).any():
        return {"shape": list(a.shape), "type": "<f2", "hex": half.tobytes().hex()}
    return {"shape": list(a.shape), "type": "<f8", "hex": a.tobytes().hex()}


def _unpack(d):
    if d is None:
        return None
    return np.frombuffer(bytes.fromhex(d["hex"]), d["type"]).astype(np.float64).reshape(d["shape"])


def _pack_answer(ans):
    return {k: (v if isinstance(v, (str, int)) else float(v).hex() if np.ndim(v) == 0 else _pack(v)) for k, v in ans.items()}


def _unpack_answer(d):
    return {k: (v if k in ("status", "nodes") else float.fromhex(v) if isinstance(v, str) else _unpack(v)) for k, v in d.items()}


def dump(groups, path):
    doc = []
    for g in groups:
        h = {k: v for k, v in g.items() if k != "cases"}
        h["cases"] = [dict({k: _pack(case[k]) for k in OPERANDS}, answer=_pack_answer(case["answer"])) for case in g["cases"]]
        doc.append(h)
    with gzip.GzipFile(path, "wb", compresslevel=9, mtime=0) as fh:
        fh.write(json.dumps(doc, sort_keys=True).encode())


def load(kind):
    with gzip.open(PATHS[kind], "rb") as fh:
        doc = json.loads(fh.read().decode())
    for g in doc:
        g["cases"] = [dict({k: _unpack(case[k]) for k in OPERANDS}, answer=_unpack_answer(case["answer"])) for case in g["cases"]]
    return doc


def stacked(group):
    """The seven operands of the group's one batched call: [B, ...] arrays, None where absent."""
    return [None if group["cases"][0][k] is None else np.stack([case[k] for case in group["cases"]]) for k in OPERANDS]


def solved_lp(group):
    """The generated group with HiGHS's answers, the LPs that are not unique() dropped (the endings keep every case that HiGHS decides)."""
    kept = []
    for case in group["cases"]:
        ans = scipy_lp(group, case)
        if (group["family"] == "endings" and ans["status"] != "undecided") or unique(group, case, ans):
            kept.append(dict(case, answer=ans))
    return dict(group, cases=kept, dropped=group["generated"] - len(kept))


def record():
    from tests import _independent_models as IM
    lps = [solved_lp(generate(g)) for g in lp_groups()] + [solved_lp(g) for g in ending_groups("lp")]
    dump(lps, PATHS["lp"])
    milps = []
    for g in [generate(g) for g in milp_groups()] + ending_groups("milp"):
        rows = IM.milp_rows(g)
        kept = []
        for case, row in zip(g["cases"], rows):
            ans = scipy_milp(g, case)
            if g["family"] == "endings" and ans["status"] != "undecided":
                kept.append(dict(case, answer=dict(ans, nodes=int(row["nodes"]))))
            elif row["status"] == "optimal" and ans["status"] != "undecided":
                kept.append(dict(case, answer=dict(ans, nodes=int(row["nodes"]))))
        milps.append(dict(g, cases=kept, dropped=g["generated"] - len(kept)))
    dump(milps, PATHS["milp"])
    for kind, groups in (("lp", lps), ("milp", milps)):
        for g in groups:
            print("%-5s %-36s generated %3d kept %3d" % (kind, g["name"], g["generated"], len(g["cases"])))
        print(kind, os.path.getsize(PATHS[kind]), "bytes")


if __name__ == "__main__":
    if sys.argv[1:] != ["record"]:
        sys.exit("usage: python -m tests._independent record")
    record()
