"""The marginals of linprog_batch(duals=True) / yalps_lpdense_solve_duals without a GPU: the numpy restatement of what
DenseJob::after writes (tests/_np_dense_duals.py) against sensitivity() of the equivalent model on the oracle's final tableau,
the two identities, an LP that ends with both slacks of an equality out of the basis, linprog_objective's gradient formulas
against central differences of the oracle's result, and what the new entry and the new Python arguments refuse without a
device."""
import os
import re

import numpy as np
import pytest

from tests import _lp_dense as LD
from tests import _np_dense as ND
from tests import _np_dense_duals as DD
from tests import _np_sensitivity as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((5, 4, 0), (5, 4, 1), (6, 3, 3), (4, 0, 2), (1, 2, 0), (1, 1, 1), (2, 0, 1))  # (n, m_ub, m_eq): m_eq in {0, 1, 3}, m_ub = 0, n = 1
SEEDS = 24
# The oracle's own residual on these LPs (small integers; measured over the 170-odd optimal records below): the objective
# identity is off by at most 4.6e-9 -- the rounding of the result to the precision of 1e-8, which allows precision / 2 = 5e-9 --
# and the reduced-cost identity by at most 2.1e-14, the rounding of duals such as 1/3 and 5/11 through the dot products.  The
# bounds are twice what the rounding allows and twice the measured figure.
OBJECTIVE_RESIDUAL = 2 * 5.0e-9
REDUCED_RESIDUAL = 2 * 2.1e-14


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpdense()
    return _native


def records(oracle, shape, maximize):
    """[(lp, the oracle's answer, sensitivity()'s dict by the oracle)] of SEEDS random LPs of one shape."""
    n, m_ub, m_eq = shape
    rng = np.random.default_rng([20261026, n, m_ub, m_eq])
    lps = [LD.random_lp(rng, n, m_ub, m_eq) for _ in range(SEEDS)]
    call = LD.Call("model", lps, maximize=maximize)
    sols = NS.oracle_sensitivity(oracle, [ND.equivalent_model(*lp, maximize=maximize) for lp in lps])
    return [(lp, call.oracle_answer(oracle, i), sols[i]) for i, lp in enumerate(lps)]


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
def test_dense_marginals_are_sensitivity_of_the_equivalent_model(oracle, shape, maximize):
    n, m_ub, m_eq = shape
    sign = 1.0 if maximize else -1.0
    optimal, worst = 0, [0.0, 0.0]
    for lp, ref, sol in records(oracle, shape, maximize):
        assert sol["status"] == ref["status"]
        got = DD.marginals_of(ref, n, m_ub, m_eq, sign)
        if ref["status"] != "optimal":
            assert sol["sensitivity"] is None and all(np.isnan(a).all() for a in got)
            continue
        optimal += 1
        for name, g, e in zip(("ineqlin", "eqlin", "reduced"), got, DD.model_marginals(sol, n, m_ub, m_eq)):
            assert np.array_equal(words(g), words(e)), (shape, maximize, name, g, e)
            assert not (words(g) == np.int64(-2 ** 63)).any(), (name, g)  # (the + 0.0: no -0.0)
        assert sol["result"] == ref["objective"]
        r_obj, r_red = DD.identity_residuals(lp, ref["objective"], *got)
        worst = [max(worst[0], r_obj), max(worst[1], r_red)]
        assert r_obj <= OBJECTIVE_RESIDUAL and r_red <= REDUCED_RESIDUAL, (shape, maximize, r_obj, r_red)
    print("shape %s maximize=%s: %d optimal, residuals %.3g %.3g" % (shape, maximize, optimal, *worst))
    assert optimal >= 3, (shape, maximize, optimal)


def test_both_slacks_of_an_equality_out_of_the_basis(oracle):
    """At a precision of 0 rounding residue in the second row of an equality is pivoted on: both slacks end in columns, and the
    dual is the difference of two costs.  The restatement is still sensitivity()'s value, bit for bit."""
    lp, maximize, precision = DD.both_slacks_lp()
    call = LD.Call("both slacks", [lp], maximize=maximize, precision=precision)
    ref = call.oracle_answer(oracle, 0)
    assert ref["status"] == "optimal"
    out = DD.slacks_out(ref["pos"], call.n, call.m_ub, call.m_eq)
    assert out, "no equality of the pinned LP ends with both slacks out of the basis: run find_both_slacks"
    assert 3 in DD.find_both_slacks(oracle, range(8))
    got = DD.marginals_of(ref, call.n, call.m_ub, call.m_eq, -1.0)
    sol = NS.oracle_sensitivity(oracle, [ND.equivalent_model(*lp, maximize=maximize)], {"precision": precision})[0]
    assert sol["status"] == "optimal"
    for g, e in zip(got, DD.model_marginals(sol, call.n, call.m_ub, call.m_eq)):
        assert np.array_equal(words(g), words(e)), (g, e)
    # both terms of the difference are read: dropping the second row's changes the value
    w, k = call.n + 1, out[0]
    row0 = ref["matrix"][:w]
    lower = -DD.cost(row0, int(ref["pos"][w + 2 + call.m_ub + 2 * k]))
    upper = -DD.cost(row0, int(ref["pos"][w + 1 + call.m_ub + 2 * k]))
    assert got[1][k] == -1.0 * (upper - lower) + 0.0


def test_nan_cost_stays_nan():
    """cost is np.minimum's, not fmin's: a NaN in row 0 is a NaN dual / reduced cost, and -0.0 never appears."""
    n, m_ub, m_eq = 2, 1, 1
    w = n + 1
    matrix = np.zeros(w * 4)
    matrix[1], matrix[2] = np.nan, -0.0
    pos = np.arange(w + 4, dtype=np.int32)
    pos[[1, w + 1]] = pos[[w + 1, 1]]  # x0 basic in row 1, the slack of u0 in column 1 (NaN); x1 in column 2 (-0.0)
    ineqlin, eqlin, reduced = DD.dense_marginals(matrix, pos, n, m_ub, m_eq, -1.0)
    assert np.isnan(ineqlin[0]) and words(eqlin)[0] == 0 and words(reduced).tolist() == [0, 0]
    want = np.minimum(matrix[:w], 0.0)
    assert np.isnan(want[1]) and DD.cost(matrix, 2) == 0.0 and np.isnan(DD.cost(matrix, 1))


@pytest.mark.parametrize("k", range(len(DD.GRAD_SEEDS)))
def test_gradient_formulas_against_central_differences(oracle, k):
    """dc = x, db = the marginals, dA = -marginal (x) x, against central differences of the oracle's objective; the steps stay
    inside the ranges sensitivity() reports, and every perturbed LP ends in the base's basis."""
    lp, maximize = DD.gradient_lps()[k]
    n, m_ub, m_eq = DD.GRAD_SHAPE
    sign = 1.0 if maximize else -1.0
    sol = NS.oracle_sensitivity(oracle, [ND.equivalent_model(*lp, maximize=maximize)], {"precision": DD.GRAD_PRECISION})[0]
    cons, variables = dict(sol["sensitivity"]["constraints"]), dict(sol["sensitivity"]["variables"])
    h = DD.GRAD_H
    for i in range(m_ub):
        lo, hi = cons["u%d" % i]["upper_range"]
        assert lo < lp[2][i] - h and lp[2][i] + h < hi, (i, lo, hi)
    for e in range(m_eq):  # (an equality moves both of its bounds: the far ends of the two one-sided ranges)
        lo, hi = cons["e%d" % e]["lower_range"][0], cons["e%d" % e]["upper_range"][1]
        assert lo < lp[4][e] - h and lp[4][e] + h < hi, (e, lo, hi)
    for j in range(n):
        lo, hi = variables["x%d" % j]["objective_range"]
        assert lo < lp[0][j] - h and lp[0][j] + h < hi, (j, lo, hi)
    numeric, base = {}, None
    for step, precision, operands in ((DD.GRAD_H, DD.GRAD_PRECISION, (0, 2, 4)), (DD.GRAD_H_A, DD.GRAD_PRECISION_A, (1, 3))):
        call = LD.Call("gradient", DD.gradient_batch(lp, step, operands), maximize=maximize, precision=precision)
        refs = [call.oracle_answer(oracle, i) for i in range(len(call.lps))]
        assert all(r["status"] == "optimal" and np.array_equal(r["pos"], refs[0]["pos"]) for r in refs)
        numeric.update(DD.central_differences([r["objective"] for r in refs], lp, step, operands))
        base = refs[0]
    ineqlin, eqlin, _ = DD.marginals_of(base, n, m_ub, m_eq, sign)
    formulas = dict(enumerate(DD.objective_gradients(1.0, base["x"], ineqlin, eqlin)))
    assert np.count_nonzero(ineqlin) and np.count_nonzero(eqlin) and np.count_nonzero(base["x"]) >= 2
    tol = DD.gradient_tolerances(base, lp, formulas)
    for op in range(5):
        assert (np.abs(numeric[op] - formulas[op]) <= tol[op]).all(), (op, numeric[op], formulas[op], tol[op])
        assert tol[op].max() < 1e-5 * max(1.0, np.abs(formulas[op]).max())


def test_dense_from_case_is_the_model(oracle):
    """The two degenerate golden cases written densely solve to their expected results, at a degenerate vertex."""
    from tests import _cases
    for name in ("Degenerate Max", "Degenerate Min"):
        lp, maximize = DD.dense_from_case(name)
        call = LD.Call(name, [lp], maximize=maximize)
        ref = call.oracle_answer(oracle, 0)
        exp = _cases.load(name)["expected"]
        assert ref["status"] == "optimal" and abs(ref["objective"] - exp["result"]) <= 1e-7
        basic_rows = [int(p) - call.w for p in ref["pos"] if p >= call.w]
        assert any(abs(ref["col0"][r]) <= 1e-8 for r in basic_rows if r > 0), "no basic variable at zero: the vertex is not degenerate"


FAKE = 4096  # a pointer value no check dereferences


def test_new_entry_refuses_on_the_host(nat):
    """yalps_lpdense_solve_duals without a handle, and LpDense.solve's routing: the three NULLs are yalps_lpdense_solve."""
    L = nat.lpdense_lib()
    assert "yalps_lpdense_solve_duals" in nat.SYMBOLS_LPDENSE and hasattr(L, "yalps_lpdense_solve_duals")
    null = [None] * 5
    rc = L.yalps_lpdense_solve_duals(None, 1, 1, 1, 0, *null, 0, 1e-8, 8192.0, 0, 0, None, None, None, None, FAKE, None, None, None)
    assert rc == -1 and L.yalps_lpdense_last_error() == b"yalps_lpdense_solve_duals: handle is NULL"
    rc = L.yalps_lpdense_solve(None, 1, 1, 1, 0, *null, 0, 1e-8, 8192.0, 0, 0, None, None, None, None, None)
    assert rc == -1 and L.yalps_lpdense_last_error() == b"yalps_lpdense_solve: handle is NULL"
    header = open(os.path.join(ROOT, "include", "yalps_lpdense.h")).read()
    for word in ("ineqlin_out[count][m_ub]", "eqlin_out[count][m_eq]", "reduced_out[count][n]", "lower.marginals"):
        assert word in header, word


def test_validate_is_unchanged_by_the_new_outputs(nat):
    """The shape checks the new entry makes first are yalps_lpdense_validate's: same refusals, same texts."""
    with pytest.raises(nat.NativeError, match=re.escape("b_eq is NULL")):
        nat.lpdense_validate(2, 3, 0, 2, [(FAKE, 3, 1, 0), None, None, (FAKE, 6, 3, 1), None])
    nat.lpdense_validate(5, 0, 2, 0, [None, None, (FAKE, 0, 1, 0), None, None])


def test_duals_flag_is_keyword_only_and_checked_before_the_library(nat, monkeypatch):
    import inspect
    import torch
    from yalps_amd import tensors
    monkeypatch.setattr(nat, "LpDense", lambda *a, **k: pytest.fail("the library was touched"))
    p = inspect.signature(tensors.linprog_batch).parameters["duals"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert tensors.LinprogDuals._fields == tensors.LinprogBatch._fields + ("ineqlin", "eqlin", "reduced_costs")
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(ValueError, match="CPU tensor"):
        tensors.linprog_batch(z(3), z(2, 3), z(2), duals=True)
    with pytest.raises(ValueError, match="CPU tensor"):
        tensors.linprog_objective(z(3).requires_grad_(), z(2, 3), z(2))
    with pytest.raises(ValueError, match="come together"):
        tensors.linprog_objective(z(3), z(2, 3))
    with pytest.raises(ValueError, match="disagree about B"):
        tensors.linprog_objective(z(5, 3), z(4, 2, 3), z(2))
    with pytest.raises(TypeError, match="float32"):
        tensors.linprog_objective(z(3).float(), z(2, 3), z(2))
    assert set(inspect.signature(tensors.linprog_objective).parameters) == {
        "c", "A_ub", "b_ub", "A_eq", "b_eq", "maximize", "precision", "max_pivots", "check_cycles"}


def test_objective_backward_formulas_on_the_host():
    """_Objective.backward is torch arithmetic on saved tensors: driven here with hand-made ones on the CPU.  Rows that did
    not end optimal -- NaN marginals, an infinite or NaN x -- contribute exact zeros; a shared operand gets the batch sum."""
    import torch
    from yalps_amd import tensors
    B, n, m_ub, m_eq = 3, 2, 2, 1
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[1.0, 2.0], [nan, nan], [0.0, inf]], dtype=torch.float64)
    status = torch.tensor([0, 1, 2], dtype=torch.int32)
    ineqlin = torch.tensor([[0.5, 0.0], [nan, nan], [nan, nan]], dtype=torch.float64)
    eqlin = torch.tensor([[-3.0], [nan], [nan]], dtype=torch.float64)

    class Ctx:
        saved_tensors = (x, status, ineqlin, eqlin)
        sides = (True, True)
        needs_input_grad = (False, True, True, True, True, True)
    g = torch.tensor([2.0, 5.0, 7.0], dtype=torch.float64)
    none, dc, dA_ub, db_ub, dA_eq, db_eq = tensors._Objective.backward(Ctx, g)
    assert none is None
    want = DD.objective_gradients(2.0, x[0].numpy(), ineqlin[0].numpy(), eqlin[0].numpy())
    for got, e in zip((dc, dA_ub, db_ub, dA_eq, db_eq), want):
        assert np.array_equal(got[0].numpy(), e), (got[0], e)
        assert not got[1:].isnan().any() and not got[1:].any(), got
    Ctx.needs_input_grad = (False, True, False, False, False, True)
    Ctx.sides = (True, False)
    assert [t is None for t in tensors._Objective.backward(Ctx, g)] == [True, False, True, True, True, True]
