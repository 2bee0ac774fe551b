"""Helpers of tests/test_lp_dense_duals_model.py and tests/test_lp_dense_duals.py (TEST INFRASTRUCTURE): the marginals
DenseJob::after writes, restated in plain numpy from a final tableau, next to sensitivity() of the equivalent model.

  dense_marginals      (ineqlin[m_ub], eqlin[m_eq], reduced[n]) of ONE LP that ended optimal, from its final matrix and
                       positionOfVariable: include/yalps_lpdense.h's formulas, element by element
  marginals_of         the same for any status: NaN rows unless "optimal"
  model_marginals      the "dual" / "reduced_cost" values sensitivity() gives for tests/_np_dense.py::equivalent_model, as the
                       same three arrays
  identity_residuals   how far an answer is from  objective = ineqlin . b_ub + eqlin . b_eq  and
                       reduced = c - A_ub^T ineqlin - A_eq^T eqlin
  objective_gradients  linprog_objective's backward formulas for one LP
  both_slacks_lp       an equality LP that ends with both slacks of an equality out of the basis
Shares no code with the product.
"""
import numpy as np

from tests import _np_dense as ND

NAN = float("nan")


def cost(row0, c):
    """min(row0[c], 0) as np.minimum has it: a NaN stays a NaN."""
    v = float(row0[c])
    if v != v:
        return v
    return v if v < 0.0 else 0.0


def dense_marginals(matrix, pos, n, m_ub, m_eq, sign):
    w = n + 1
    row0 = np.asarray(matrix, np.float64)[:w]
    s = np.float64(sign)

    def y(r):
        p = int(pos[w + r])
        return -cost(row0, p) if p < w else 0.0

    ineqlin = np.array([s * np.float64(y(1 + i)) + 0.0 for i in range(m_ub)], np.float64)
    eqlin = np.array([s * (np.float64(y(1 + m_ub + 2 * k)) - np.float64(y(2 + m_ub + 2 * k))) + 0.0 for k in range(m_eq)], np.float64)
    reduced = np.zeros(n, np.float64)
    for j in range(n):
        p = int(pos[j + 1])
        if p < w:
            reduced[j] = s * np.float64(cost(row0, p)) + 0.0
    return ineqlin, eqlin, reduced


def marginals_of(ref, n, m_ub, m_eq, sign):
    """dense_marginals of an oracle answer (tests/_lp_dense.py::Call.oracle_answer); NaN rows unless it ended optimal."""
    if ref["status"] != "optimal":
        return np.full(m_ub, NAN), np.full(m_eq, NAN), np.full(n, NAN)
    return dense_marginals(ref["matrix"], ref["pos"], n, m_ub, m_eq, sign)


def model_marginals(sol, n, m_ub, m_eq):
    """The three arrays from a sensitivity() dict of the equivalent model (status "optimal")."""
    cons, vars_ = dict(sol["sensitivity"]["constraints"]), dict(sol["sensitivity"]["variables"])
    return (np.array([cons["u%d" % i]["dual"] for i in range(m_ub)], np.float64),
            np.array([cons["e%d" % k]["dual"] for k in range(m_eq)], np.float64),
            np.array([vars_["x%d" % j]["reduced_cost"] for j in range(n)], np.float64))


def identity_residuals(lp, objective, ineqlin, eqlin, reduced):
    """(|objective - y.b|, max |reduced - (c - A^T y)|) of one optimal LP."""
    c, A_ub, b_ub, A_eq, b_eq = lp
    n, m_ub, m_eq = ND.shape_of(*lp)
    value, rc = 0.0, np.asarray(c, np.float64).copy()
    if m_ub:
        value += float(np.dot(ineqlin, b_ub))
        rc -= np.asarray(A_ub, np.float64).reshape(m_ub, n).T @ ineqlin
    if m_eq:
        value += float(np.dot(eqlin, b_eq))
        rc -= np.asarray(A_eq, np.float64).reshape(m_eq, n).T @ eqlin
    return abs(objective - value), float(np.abs(reduced - rc).max()) if n else 0.0


def objective_gradients(g, x, ineqlin, eqlin):
    """(dc, dA_ub, db_ub, dA_eq, db_eq) of g * objective for one optimal LP."""
    return g * x, -g * np.outer(ineqlin, x), g * ineqlin, -g * np.outer(eqlin, x), g * eqlin


# --------------------------------------------------------------------------------- both slacks of an equality out of the basis
# In exact arithmetic the two rows of an equality are each other's negation, and after a pivot in one the other reads
# slack + slack' = 0: its only entry is the column the first slack went to.  A pivot there needs that entry's row 0 cost or its
# right-hand side to ask for it, which rounding residue does at a precision of 0: found by search (find_both_slacks), pinned here.


def both_slacks_candidate(seed):
    rng = np.random.default_rng([20261024, seed])
    n, m_ub, m_eq = 4, 2, 2
    return (rng.random(n) * 4.0 - 1.0, rng.random((m_ub, n)) * 3.0, 1.0 + rng.random(m_ub) * 4.0,
            rng.random((m_eq, n)) * 3.0 - 0.5, 0.5 + rng.random(m_eq))


def slacks_out(pos, n, m_ub, m_eq):
    """The equalities k whose two slacks both sit in columns of the final tableau."""
    w = n + 1
    return [k for k in range(m_eq) if pos[w + 1 + m_ub + 2 * k] < w and pos[w + 2 + m_ub + 2 * k] < w]


def both_slacks_lp():
    """(lp, maximize, precision); tests/test_lp_dense_duals_model.py asserts the property on the oracle's answer."""
    return both_slacks_candidate(3), False, 0.0


def find_both_slacks(oracle, seeds=range(400), precision=0.0, maximize=False):
    """The search that chose both_slacks_lp's seed: the seeds whose LP ends optimal with both slacks of an equality in columns."""
    from tests import _lp_dense as LD
    out = []
    for seed in seeds:
        call = LD.Call("search", [both_slacks_candidate(seed)], maximize=maximize, precision=precision)
        ref = call.oracle_answer(oracle, 0)
        if ref["status"] == "optimal" and slacks_out(ref["pos"], call.n, call.m_ub, call.m_eq):
            out.append(seed)
    return out


def dense_from_case(name):
    """A golden case (tests/golden/cases) with constraints of one bound each, written densely: ((c, A_ub, b_ub, A_eq, b_eq),
    maximize).  {"max": b} is a row of A_ub, {"min": b} its negation, {"equal": b} a row of A_eq."""
    from tests import _cases
    model = _cases.load(name)["model"]
    keys = list(model["variables"])
    c = np.array([float(model["variables"][k].get(model["objective"], 0.0)) for k in keys])
    ub, eq = [], []
    for con, bound in model["constraints"].items():
        row = np.array([float(model["variables"][k].get(con, 0.0)) for k in keys])
        (kind, b), = bound.items()
        if kind == "equal":
            eq.append((row, float(b)))
        else:
            ub.append((row, float(b)) if kind == "max" else (-row, -float(b)))
    side = lambda rows: (np.stack([r for r, _ in rows]), np.array([b for _, b in rows])) if rows else (None, None)
    return (c, *side(ub), *side(eq)), model["direction"] == "maximize"


# ------------------------------------------------------------------------------------------- gradients by central differences
# b and c move the optimal value linearly inside a basis: a central difference is exact but for the rounding of the two results
# to `precision`, each off by at most precision / 2, so the quotient is off by at most precision / (2 h) < precision / h.
# An entry A[i, j] moves it rationally: with beta the entry of the basis inverse that joins variable j's row and constraint i's
# slack (it stands in the final tableau), f(d) = f(0) - d y_i x_j / (1 + d beta), so the central difference is the derivative
# times 1 / (1 - (h beta)^2): a relative error of (h beta)^2 / (1 - (h beta)^2) <= 2 (h beta)^2 while |h beta| <= 1/2.  A's
# step and precision are smaller for that reason.
GRAD_H, GRAD_PRECISION = 2.0 ** -6, 1e-8            # c, b_ub, b_eq: precision / h = 6.4e-7
GRAD_H_A, GRAD_PRECISION_A = 2.0 ** -12, 1e-12      # A_ub, A_eq:   precision / h = 4.1e-9, plus 2 (h beta)^2 |gradient|
GRAD_SHAPE = (3, 2, 1)                              # n, m_ub, m_eq
GRAD_SEEDS = ((9, False), (10, False), (2, True))   # (seed, maximize): a binding inequality, the equality, two variables basic


def gradient_lps():
    return [(gradient_candidate(seed), maximize) for seed, maximize in GRAD_SEEDS]


def gradient_candidate(seed):
    """Data in eighths, positive so that the LP is bounded and feasible: exactly representable."""
    rng = np.random.default_rng([20261025, seed])
    n, m_ub, m_eq = GRAD_SHAPE
    eighths = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64) / 8.0
    return (eighths(8, 40, n), eighths(8, 32, m_ub, n), eighths(40, 80, m_ub), eighths(8, 32, m_eq, n), eighths(16, 40, m_eq))


def elements(lp, operands):
    """[(k, index)] of every element of the operands k (0 = c, 1 = A_ub, 2 = b_ub, 3 = A_eq, 4 = b_eq) of one LP."""
    return [(k, idx) for k in operands for idx in np.ndindex(np.shape(lp[k]))]


def perturbed(lp, k, idx, delta):
    out = [None if a is None else np.array(a, np.float64) for a in lp]
    out[k][idx] += delta
    return tuple(out)


def gradient_batch(lp, h, operands):
    """[lp, then (+h, -h) for every element of the operands]: 1 + 2 * len(elements) LPs of one shape."""
    out = [lp]
    for k, idx in elements(lp, operands):
        out += [perturbed(lp, k, idx, h), perturbed(lp, k, idx, -h)]
    return out


def central_differences(objectives, lp, h, operands):
    """{k: array shaped like operand k} from the objectives of gradient_batch(lp, h, operands)."""
    out = {k: np.zeros(np.shape(lp[k])) for k in operands}
    for e, (k, idx) in enumerate(elements(lp, operands)):
        out[k][idx] = (objectives[1 + 2 * e] - objectives[2 + 2 * e]) / (2.0 * h)
    return out


def gradient_tolerances(ref, lp, formulas):
    """{k: array of bounds} for central_differences against the formulas, from the comment above; ref = the oracle's answer of
    the base LP at GRAD_PRECISION_A (its final matrix holds beta)."""
    n, m_ub, m_eq = GRAD_SHAPE
    w = n + 1
    M = np.asarray(ref["matrix"]).reshape(-1, w)
    out = {k: np.full(np.shape(lp[k]), GRAD_PRECISION / GRAD_H) for k in (0, 2, 4)}
    for k, rows, first in ((1, m_ub, lambda i: 1 + i), (3, m_eq, lambda i: 1 + m_ub + 2 * i)):
        tol = np.full((rows, n), GRAD_PRECISION_A / GRAD_H_A)
        for i in range(rows):
            for j in range(n):
                row = int(ref["pos"][j + 1]) - w
                if row < 0:
                    continue  # x_j = 0: the entry does not move the value at all
                cols = [int(ref["pos"][w + first(i) + t]) for t in range(2 if k == 3 else 1)]
                beta = max([abs(M[row, p]) for p in cols if p < w], default=0.0)
                assert GRAD_H_A * beta <= 0.5, (k, i, j, beta)
                tol[i, j] += 2.0 * (GRAD_H_A * beta) ** 2 * abs(formulas[k][i, j])
        out[k] = tol
    return out
