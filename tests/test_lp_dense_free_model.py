"""The free variables of linprog_batch / yalps_lpdense_solve_free without a GPU: the numpy restatement of the split
(tests/_np_dense_free.py) against the explicitly built operands and against tableau_model of the equivalent model, with its two
documented exceptions pinned; the oracle's solves of the equivalent model; the mutants of FD.FLAWS and which hard call tells which;
the endings of the statuses call; the identities; the backward formula of lb; and what the new entries and the new Python
argument refuse without a device."""
import math
import os
import re

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _lp_dense_free as LF
from tests import _np_dense as ND
from tests import _np_dense_bounds as BD
from tests import _np_dense_free as FD
from tests.test_lp_dense_bounds_model import OBJECTIVE_RESIDUAL, REDUCED_RESIDUAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("none", "lb", "ub", "both")


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpdense()
    return _native


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------- restatement

def grid_call(n, m_ub, m_eq, mode, free, upper, maximize, seed):
    return LF.random_call("grid", 2, n, m_ub, m_eq, mode=mode, upper=upper, free=free, seed=seed, maximize=maximize)


def frees(n):
    return sorted({(0,), (n - 1,), tuple(range(n))}) + [True]


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m_eq", (0, 2))
@pytest.mark.parametrize("m_ub", (0, 3))
@pytest.mark.parametrize("n", (1, 2, 5))
def test_free_tableau_is_the_explicit_route_and_the_equivalent_model(n, m_ub, m_eq, mode, maximize):
    """Byte for byte bounded_tableau of the operands with the negated columns appended -- but for the -1.0 of a bound row of a free
    variable, the first documented exception -- and tableau_model of the equivalent model."""
    from yalps_amd.model import tableau_model
    for free in frees(n):
        for upper in ((True,) if mode in ("none", "lb") else (True, (0,), (n - 1,))):
            call = grid_call(n, m_ub, m_eq, mode, free, upper, maximize, 0)
            for lp, lb, ub in zip(call.lps, call.lbs, call.ubs):
                m = FD.free_tableau(*lp, lb=lb, ub=ub, upper=call.idx, free=call.fidx, maximize=maximize).reshape(call.h, call.w)
                *ops, elb, eub, eidx = FD.explicit_operands(*lp, lb=lb, ub=ub, upper=call.idx, free=call.fidx)
                explicit = BD.bounded_tableau(*ops, lb=elb, ub=eub, upper=eidx, maximize=maximize).reshape(call.h, call.w)
                h0 = call.h - call.k
                minus = [(h0 + t, 1 + n + call.fidx.index(j)) for t, j in enumerate(call.idx) if j in call.fidx]
                for cell in minus:
                    assert m[cell] == -1.0 and words([explicit[cell]])[0] == 0, cell
                    explicit[cell] = -1.0
                assert np.array_equal(words(m), words(explicit)), (n, m_ub, m_eq, mode, free, upper)
                t = tableau_model(FD.equivalent_model(*lp, lb=lb, ub=ub, upper=call.idx, free=call.fidx, maximize=maximize)).tableau
                assert (t.width, t.height) == (call.w, call.h)
                assert np.array_equal(words(m.ravel()), words(t.matrix)), (n, m_ub, m_eq, mode, free, upper, maximize)
                assert words(m[0, :1])[0] == 0 and not m[:, 1 + n + call.f:].size
                if lb is None and not call.f:
                    assert np.array_equal(words(m.ravel()), words(BD.bounded_tableau(*lp, lb=lb, ub=ub, upper=call.idx, maximize=maximize)))


def test_the_two_documented_exceptions_are_pinned():
    """1. The bound row of a free variable: x <= ub with no lower bound needs -1.0 under the twin; the explicit route, whose twin is
    a variable of its own, has +0.0 there.  2. shift_sum runs over the n originals only, and lb is not read at a free variable: a
    coefficient 1e16 at free column 0 with lb[0] = 1 would swallow the 1.0 of column 64 in lane 0; with l_eff[0] = +0.0 it does not."""
    n = 65
    a = np.zeros(n)
    a[0], a[64] = 1e16, 1.0
    lb = np.ones(n)
    lp = (np.ones(n), a.reshape(1, n), np.array([0.5]), None, None)
    m = FD.free_tableau(*lp, lb=lb, ub=lb + 1.0, upper=(0,), free=(0,)).reshape(3, n + 2)
    assert m[1, 0] == 0.5 - 1.0 and m[1, 1 + n] == -1e16 and m[2, 0] == 2.0 - 0.0 and m[2, 1] == 1.0 and m[2, 1 + n] == -1.0
    assert FD.free_tableau(*lp, lb=lb, ub=lb + 1.0, upper=(0,), free=(0,), flaw="lb read").reshape(3, n + 2)[1, 0] == 0.5 - 1e16
    wrong = FD.free_tableau(*lp, lb=lb, ub=lb + 1.0, upper=(0,), free=(0,), flaw="sum over twins").reshape(3, n + 2)
    assert wrong[1, 0] == 0.5 - (1.0 - 1e16)  # (lane 1 holds the twin's product -1e16 * 1)
    # the product with +0.0 is still formed: an infinite coefficient in a free column gives NaN in the right-hand side
    a[0] = math.inf
    assert math.isnan(FD.free_tableau(*lp[:1], a.reshape(1, n), *lp[2:], lb=lb, free=(0,)).reshape(2, n + 2)[1, 0])
    # without lb nothing is subtracted, and the bound row holds ub[j], the caller's bits
    m = FD.free_tableau(*lp[:1], a.reshape(1, n), *lp[2:], ub=-0.0 * lb, upper=(0,), free=(0,)).reshape(3, n + 2)
    assert m[1, 0] == 0.5 and words(m[2, :1])[0] == words([-0.0])[0]
    # a twin zero is the other zero, in row 0 too: -(sign * c[j])
    z = FD.free_tableau(np.array([0.0, -0.0]), np.array([[0.0, -0.0]]), np.array([1.0]), free=True, maximize=True).reshape(2, 5)
    assert words(z[:, 3:]).tolist() == [[words([-0.0])[0], 0], [words([-0.0])[0], 0]]
    z = FD.free_tableau(np.array([0.0, -0.0]), None, None, np.array([[0.0, -0.0]]), np.array([1.0]), free=True).reshape(3, 5)
    assert words(z[:, 3:]).tolist() == [[0, words([-0.0])[0]], [words([-0.0])[0], 0], [0, words([-0.0])[0]]]


def test_free_set_refuses():
    for bad in ((0, 0), (3,), (-1,)):
        with pytest.raises(ValueError):
            FD.free_set(3, bad)
    assert FD.free_set(3, (2, 0)) == (0, 2) and FD.free_set(3, True) == (0, 1, 2) and FD.free_set(3, ()) == FD.free_set(3, None) == FD.free_set(3, False) == ()


# ---------------------------------------------------------------------------------------------------------------- solves

SOLVE_SHAPES = ((5, 4, 0), (5, 4, 1), (4, 0, 2), (2, 3, 0))
SOLVE_SEEDS = 10


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("shape", SOLVE_SHAPES)
def test_solves_are_the_equivalent_model_and_keep_the_identities(oracle, shape, maximize):
    """solve() of the equivalent model -- tableau_model, the oracle's simplex, solution() --: the same status and pivots, and after the subtraction the
    same x and objective; on every optimal row the two identities, within the bounds model test's tolerances (the same generator of
    small integers)."""
    from yalps_amd.model import Tableau, TableauModel, tableau_model
    from yalps_amd.solve import solution
    n, m_ub, m_eq = shape
    optimal, negative, worst = 0, 0, [0.0, 0.0]
    for mode in MODES:
        for free in ((0,), tuple(sorted({1, n - 1})), True):
            call = LF.random_call("solves", SOLVE_SEEDS, n, m_ub, m_eq, mode=mode, upper=(0, n - 1) if mode in ("ub", "both") else True,
                                  free=free, maximize=maximize)
            for i, lp in enumerate(call.lps):
                ref = call.oracle_answer(oracle, i)
                lb, ub = call.lbs[i], call.ubs[i]
                model = FD.equivalent_model(*lp, lb=lb, ub=ub, upper=call.idx, free=call.fidx, maximize=maximize)
                t = tableau_model(model).tableau
                pos, var = np.arange(call.w + call.h, dtype=np.int32), np.arange(call.w + call.h, dtype=np.int32)
                tm = np.array(t.matrix, np.float64)
                status, result, npiv, _ = oracle.simplex(tm, call.w, call.h, pos, var, precision=call.precision, max_pivots=call.max_pivots)
                assert (status, npiv) == (ref["status"], ref["n_pivots"]) and np.array_equal(words(tm), words(ref["matrix"]))
                sign = 1.0 if maximize else -1.0
                done = TableauModel(Tableau(None, call.w, call.h, pos, var, tm.reshape(call.h, call.w)[:, 0].copy()), sign,
                                    [(name, {}) for name in model["variables"]], [])
                sol = solution(done, status, result, {"precision": call.precision, "includeZeroVariables": True})
                assert sol["status"] == ref["status"], (i, sol["status"], ref["status"])
                if ref["status"] != "optimal":
                    assert all(np.isnan(ref[k]).all() for k in LF.OUTPUTS)
                    continue
                values = dict(sol["variables"])
                low = call.low(i)
                x = np.array([np.float64(values["x%d" % j]) - (values["q%d" % j] if j in call.fidx else 0.0) for j in range(n)])
                if low is not None:
                    x = x + low
                assert np.array_equal(words(x), words(ref["x"])), (i, x, ref["x"])
                shift = BD.shift_sum(lp[0], low) if low is not None else None
                assert words([sol["result"] + shift if low is not None else sol["result"]])[0] == words([ref["objective"]])[0]
                optimal += 1
                negative += bool((ref["x"] < 0).any())
                r_obj, r_red = FD.identity_residuals(lp, lb, ub, call.idx, call.fidx, ref["objective"], *(ref[k] for k in LF.OUTPUTS))
                worst = [max(a, b) for a, b in zip(worst, (r_obj, r_red))]
                assert r_obj <= OBJECTIVE_RESIDUAL and r_red <= REDUCED_RESIDUAL, (call.name, i, r_obj, r_red)
                # objective = c . x: x and the result are each rounded to the precision, half a unit of it at the most
                assert abs(float(np.dot(lp[0], ref["x"])) - ref["objective"]) <= 0.5 * call.precision * (1.0 + float(np.abs(lp[0]).sum())) * (1 + 1e-6)
                assert not (words(np.concatenate([ref[k] for k in LF.OUTPUTS])) == np.int64(-2 ** 63)).any()  # (the + 0.0: no -0.0)
    print("shape %s maximize=%s: %d optimal, %d with a negative x, residuals %.3g %.3g" % (shape, maximize, optimal, negative, *worst))
    assert optimal >= 12 and negative >= 3, (shape, maximize, optimal, negative)


def test_statuses_call_holds_all_endings_and_an_unbounded_twin(oracle):
    call = LF.statuses_call()
    refs = LF.answers(oracle, call)
    assert {r["status"] for r in refs} == {"optimal", "infeasible", "unbounded", "cycled"}
    twins = [r for r in refs if r["status"] == "unbounded" and call.n < int(r["var"][int(r["result"])]) < call.w]
    assert twins and all((r["x"] == -math.inf).sum() == 1 and not (r["x"] == math.inf).any() for r in twins)
    assert any(r["status"] == "unbounded" and (r["x"] == math.inf).any() for r in refs)
    assert call.fidx == (1, 3) and call.idx == (0, 1) and call.maximize and call.max_pivots == 2.0 and len(call.lps) == 2100


def test_table_calls_end_optimal_in_their_forms(oracle):
    """Every generated call of the table ends optimal after more than a handful of pivots with a negative x, in the form its name
    says; together they run all six forms."""
    forms = set()
    for call in LF.table(oracle):
        forms.add(LF.kernel_of(call)[1])
        if call.name in ("statuses", "nonfinite"):
            continue
        refs = LF.answers(oracle, call)
        assert any(r["status"] == "optimal" and (r["x"] < 0).any() for r in refs), call.name
        if "bound" in call.name or call.name in ("HBM 301x280", "aux"):
            assert refs[0]["n_pivots"] >= 12 and call.fidx[-1] == call.n - 1 and call.idx[0] == call.fidx[0] == 0
    assert forms == {"lp_dense_free_kernel<%s>" % f for f in ("256,lds", "256,check,lds", "1024,lds", "1024,check,lds", "1024", "1024,check")}
    hist = LF.hist_call(oracle)
    assert all(r["status"] == "optimal" and r["n_pivots"] > 2 * LF.LD.HIST and (r["x"][list(hist.fidx)] != 0).any() for r in LF.answers(oracle, hist))
    a, b = LF.nan_lb_calls()
    for ra, rb in zip(LF.answers(oracle, a), LF.answers(oracle, b)):
        assert all(np.array_equal(words(ra[k]), words(rb[k])) for k in ("start", "matrix", "x", "objective") + LF.OUTPUTS)
        assert not np.isnan(ra["start"]).any() and (ra["status"] != "optimal" or not np.isnan(ra["x"]).any())
    refs = LF.answers(oracle, LF.nonfinite_call())
    assert np.isnan(refs[0]["start"].reshape(8, 8)[1, 0]) and np.isinf(refs[2]["start"]).any() and not np.isfinite(refs[3]["start"]).all()


# ---------------------------------------------------------------------------------------------------------------- mutants

# the flaws each hard call must tell (tests/_lp_dense_free.py's hard_table); found with the oracle alone
TELLS = {
    "start n=3 f=1 none min": {"both equality rows", "positive zero", "sum of halves"},
    "start n=3 f=1 lb min": {"lb read", "sum over twins"},
    "start n=3 f=1 ub min": {"bound row without -1"},
    "start n=3 f=1 both max": {"both equality rows", "lb read", "sum over twins", "bound row without -1", "sum of halves"},
    "free in upper": {"bound row without -1", "sum of halves", "twin +inf"},
    "signed zeros": {"positive zero"},
    "rounding": {"subtract first", "reduced without twin", "sum of halves", "twin +inf"},
}


@pytest.mark.parametrize("name", LF.hard_names())
def test_hard_calls_tell_the_mutants(oracle, name):
    call = {c.name: c for c in LF.hard_table()}[name]
    told = set(LF.told(oracle, call))
    print(name, sorted(told))
    assert told >= TELLS.get(name, set()), (name, sorted(told))
    assert not told & set(FD.UNTELLABLE), (name, sorted(told))
    assert all(r["status"] == "cycled" and r["n_pivots"] == 0 for r in LF.answers(oracle, LF.at_budget_0(call)))


def test_every_tellable_mutant_is_told_and_the_second_product_is_a_negation(oracle):
    assert set().union(*TELLS.values()) == set(FD.FLAWS) - set(FD.UNTELLABLE)
    # (-1) * sign * c IS -(sign * c) for every double that is not a NaN: zeros, subnormals, the largest, infinities
    with np.errstate(all="ignore"):
        for v in (0.0, -0.0, 5e-324, -5e-324, 1.7976931348623157e308, math.inf, -math.inf, 1.0 / 3.0):
            for sign in (1.0, -1.0):
                assert words([np.float64(-1.0) * np.float64(sign) * np.float64(v)])[0] == words([-(np.float64(sign) * np.float64(v))])[0]
    pin = LF.rounding_call()
    ref, bad = LF.answers(oracle, pin)[0], LF.answers(oracle, pin, "subtract first")[0]
    assert ref["status"] == "optimal" and ref["x"].tolist() == [-0.75, 0.0] and bad["x"].tolist() == [-0.5, 0.0]


# ------------------------------------------------------------------------------------------------------------- gradients

def test_gradient_call_has_a_negative_free_x_and_an_infeasible_row(oracle):
    call = LF.gradient_call()
    refs = LF.answers(oracle, call)
    assert [r["status"] for r in refs] == ["optimal", "optimal", "infeasible"] and refs[0]["x"][1] < 0
    assert np.count_nonzero(refs[0]["reduced"]) and abs(refs[0]["reduced"][1]) <= REDUCED_RESIDUAL


def test_backward_gives_exact_zeros_to_lb_at_free_variables():
    """_BoundedObjective.backward is torch arithmetic on saved tensors: hand-made ones on the CPU."""
    import torch
    from yalps_amd import tensors
    nan = float("nan")
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    x, status = t([[1.0, -2.0, -1.0], [nan, nan, nan]]), torch.tensor([0, 1], dtype=torch.int32)
    ineqlin, eqlin = t([[0.5], [nan]]), t([[], []])
    reduced, marg = t([[0.0, -3e-17, 0.25], [nan, nan, nan]]), t([[4.0, 0.0], [nan, nan]])

    class Ctx:
        saved_tensors = (x, status, ineqlin, eqlin, reduced, marg)
        sides, bounds, upper, free = (True, False), (True, True), [0, 2], [1]
        needs_input_grad = (False, False, True, True, True, False, False, True, True)
    got = tensors._BoundedObjective.backward(Ctx, t([2.0, 5.0]))
    assert got[2].tolist() == [[2.0, -4.0, -2.0], [0.0, 0.0, 0.0]]
    assert got[7].tolist() == [[0.0, 0.0, 0.5], [0.0, 0.0, 0.0]] and words(got[7].numpy())[0, 1] == 0
    assert got[8].tolist() == [[8.0, 0.0, 0.0], [0.0, 0.0, 0.0]]


# ------------------------------------------------------------------------------------------------------- argument checks

FAKE = 4096  # a pointer value no check dereferences


def test_new_entries_refuse_on_the_host(nat):
    L = nat.lpdense_lib()
    for s in ("yalps_lpdense_solve_free", "yalps_lpdense_validate_free"):
        assert s in nat.SYMBOLS_LPDENSE and hasattr(L, s)
    null = [None] * 5
    rc = L.yalps_lpdense_solve_free(None, 1, 1, 1, 0, *null, None, None, 0, None, 0, None, 0, 1e-8, 8192.0, 0, 0, *([None] * 8), None)
    assert rc == -1 and L.yalps_lpdense_last_error() == b"yalps_lpdense_solve_free: handle is NULL"
    ops = [(FAKE, 3, 1, 0), (FAKE, 6, 3, 1), (FAKE, 2, 1, 0), None, None]
    vec = (FAKE, 3, 1, 0)
    nat.lpdense_validate_free(2, 3, 2, 0, ops, lb=vec, ub=vec, upper=(0, 2), free=(0, 1))
    nat.lpdense_validate_free(2, 3, 2, 0, ops, free=(2,))  # free alone
    nat.lpdense_validate_free(2, 3, 2, 0, ops)  # nothing: yalps_lpdense_validate
    for kw, reason in ((dict(free=(0, 3)), "free_idx[1] = 3 is outside 0 .. n-1"), (dict(free=(-1,)), "outside 0 .. n-1"),
                       (dict(free=(1, 1)), "free_idx is not ascending"), (dict(free=(2, 0)), "free_idx is not ascending"),
                       (dict(free=(0,), upper=(0,)), "without ub"), (dict(free=(0,), lb=(None, 3, 1, 0)), "lb is NULL")):
        with pytest.raises(nat.NativeError, match=re.escape(reason)):
            nat.lpdense_validate_free(2, 3, 2, 0, ops, **kw)
    rc = L.yalps_lpdense_validate_free(2, 3, 2, 0, *[None] * 5, None, None, 0, None, -1, None)
    assert rc == -1 and b"n_free < 0" in L.yalps_lpdense_last_error()
    # the size limit counts the twins: (1 + 511 + 511) x 512 is 4 MiB less a row, one more row is above it, and the text names the shape
    big = [(FAKE, 0, 1, 0), (FAKE, 0, 511, 1), (FAKE, 0, 1, 0), None, None]
    nat.lpdense_validate_free(1, 511, 511, 0, big, free=range(511))
    with pytest.raises(nat.NativeError, match=re.escape("tableau of 513 x 1023 doubles is above the limit")):
        nat.lpdense_validate_free(1, 511, 512, 0, big, free=range(511))
    nat.lpdense_validate_bounds(1, 511, 512, 0, big)  # (without the twins it passes)
    header = open(os.path.join(ROOT, "include", "yalps_lpdense.h")).read()
    for word in ("x[j] = p[j] - q[j]", "column 1 + n + t", "NOT read at a free variable", "cost_nb(1 + j) - cost_nb(1 + n + t)", "n_free = 0"):
        assert word in header, word
    assert "Free variables are out of scope" not in header


def test_free_is_checked_before_the_library(nat, monkeypatch):
    import inspect
    import torch
    from yalps_amd import tensors
    monkeypatch.setattr(nat, "LpDense", lambda *a, **k: pytest.fail("the library was touched"))
    for fn in (tensors.linprog_batch, tensors.linprog_objective_bounds):
        p = inspect.signature(fn).parameters["free"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == ()
    assert "free" not in inspect.signature(tensors.linprog_objective).parameters and "free" not in inspect.signature(tensors.milp_batch).parameters
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    for call in (tensors.linprog_batch, tensors.linprog_objective_bounds):
        with pytest.raises(ValueError, match="free names variable 1 twice"):
            call(z(3), z(2, 3), z(2), free=(1, 1))
        for bad in ((3,), (-1,)):
            with pytest.raises(ValueError, match="outside 0 .. 2"):
                call(z(3), z(2, 3), z(2), free=bad)
        for bad in ((1.5,), (True,), "01", 7, ("1",)):
            with pytest.raises((TypeError, ValueError), match="free"):
                call(z(3), z(2, 3), z(2), free=bad)
        for bad in ((1.5,), (True,), "01", 7):
            with pytest.raises(TypeError, match="free"):
                call(z(3), z(2, 3), z(2), free=bad)
        for none in ((), False, None, [], (2.0,), range(3), True, np.array([0, 2])):
            with pytest.raises(ValueError, match="CPU tensor"):  # (the set is accepted; the operands are refused next)
                call(z(3), z(2, 3), z(2), free=none)
    assert tensors._free_set(3, (2, 0)) == [0, 2] and tensors._free_set(3, True) == [0, 1, 2] and tensors._free_set(3, None) == []
    # the size limit counts the twins, and the text names the widened shape
    with pytest.raises(ValueError, match=r"513 x 1023 doubles.*solve\(\)"):
        tensors.linprog_batch(z(511), z(512, 511), z(512), free=True)
    with pytest.raises(ValueError, match="CPU tensor"):
        tensors.linprog_batch(z(511), z(511, 511), z(511), free=True)
    with pytest.raises(ValueError, match="CPU tensor"):
        tensors.linprog_batch(z(511), z(512, 511), z(512))
    for doc in (tensors.linprog_batch.__doc__, tensors.linprog_objective_bounds.__doc__):
        assert "free" in doc and "Out of scope: free" not in doc and "er-LP `upper` and `free` sets" in doc
    assert "Out of scope: free" in tensors.milp_batch.__doc__


def test_free_kernels_pass_the_register_budget(nat):
    """The six free forms are a code object of their own, under the same build gate: no scratch, no accumulator registers,
    within 128 VGPRs, static LDS a multiple of 16; the other two code objects hold the six forms each they held."""
    from yalps_amd import build
    ks = build.check_register_budgets(build.LIB_LPDENSE_FREE, min_resident=0)
    assert len(ks) == 6 and all("lp_dense_free_kernel" in k for k in ks), sorted(ks)
    for k, md in ks.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0 and int(md["vgpr_count"]) <= 128, (k, md)
        assert int(md["group_segment_fixed_size"]) % 16 == 0
    for lib, kernel in ((build.LIB_LPDENSE, "lp_dense_kernel"), (build.LIB_LPDENSE_BOUNDS, "lp_dense_bounds_kernel")):
        ks = build.kernel_metadata(lib)
        assert len(ks) == 6 and all(kernel in k for k in ks), (lib, sorted(ks))
