"""The bounds of linprog_batch / yalps_lpdense_solve_bounds without a GPU: the canonical shift_sum, its second statement and its
named flawed forms, the floors by which the hard calls of tests/_lp_dense_bounds.py tell every flaw, the numpy restatement of the
bounded tableau (tests/_np_dense_bounds.py) against the explicitly built operands and against tableau_model of the equivalent
model, the oracle's solves of it (feasibility, the two identities, the three endings bounds add), the lb / ub gradient formulas
against central differences of the oracle's objective, and what the new entries and the new Python arguments refuse without a
device."""
import math
import os
import re

import numpy as np
import pytest

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _lp_dense_bounds as LBD
from tests import _np_dense as ND
from tests import _np_dense_bounds as BD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("lb", "ub", "both")
# The oracle's own residuals on the grid of test_solves_respect_the_bounds_and_the_identities (small integers; measured over its
# 896 optimal records); each bound is twice the measured figure.  x leaves [lb, ub] by 0.0: the values are integers, rounded to
# the precision of 1e-8 before lb is added.  The objective identity is off by at most 4.865e-9, the rounding of the result to 1e-8.
# The reduced-cost identity is off by at most 1.85e-13, the rounding of duals such as 1/3 through the dot products and the
# products with bounds of up to 8.
FEASIBILITY = 2 * 0.0
OBJECTIVE_RESIDUAL = 2 * 4.865e-9
REDUCED_RESIDUAL = 2 * 1.85e-13


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpdense()
    return _native


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------ shift_sum

def test_shift_sum_order_is_pinned():
    """1e16 at column 0, 1.0 at column 64, -1e16 at column 1: lane 0 adds 1e16 + 1.0 = 1e16 (the 1.0 is lost), lane 1 holds -1e16, the
    tree adds them to 0.0.  Left to right gives 1e16 - 1e16 + 1.0 = 1.0, and so does numpy's dot."""
    a = np.zeros(65)
    a[0], a[64], a[1] = 1e16, 1.0, -1e16
    one = np.ones(65)
    got = BD.shift_sum(a, one)
    assert words([got])[0] == words([0.0])[0]
    loop = 0.0
    for v in a:
        loop += v * 1.0
    assert loop == 1.0 and float(np.dot(a, one)) != got and loop != got
    # the tree's order too: lanes 0 and 32 meet first (1e16 + -1e16 = 0), lane 16 joins afterwards and survives
    b = np.zeros(64)
    b[0], b[32], b[16] = 1e16, -1e16, 1.0
    assert BD.shift_sum(b, np.ones(64)) == 1.0
    b[0], b[32], b[16] = 1e16, 1.0, -1e16
    assert BD.shift_sum(b, np.ones(64)) == 0.0
    # every product is rounded on its own: (1 + 2^-30)^2 rounds to 1 + 2^-29, and the sum with -1 - 2^-29 is exactly 0
    e = 1.0 + 2.0 ** -30
    assert BD.shift_sum([e, 1.0], [e, -(1.0 + 2.0 ** -29)]) == 0.0
    assert BD.fma(e, e, -(1.0 + 2.0 ** -29)) == 2.0 ** -60  # (in rationals: this Python may have no math.fma)
    if hasattr(math, "fma"):
        assert math.fma(e, e, -(1.0 + 2.0 ** -29)) == 2.0 ** -60
    # with n = 2 every lane holds one product, and 0.0 + a * l fused is still the rounded product: a fused kernel shows only
    # where one lane holds two columns, j and j + 64
    assert BD.flawed_shift_sum([e, 1.0], [e, -(1.0 + 2.0 ** -29)], "fused") == 0.0
    a, l = np.zeros(65), np.ones(65)
    a[0], l[0], a[64], l[64] = 1.0, -(1.0 + 2.0 ** -29), e, e
    assert words([BD.shift_sum(a, l)])[0] == 0 and BD.flawed_shift_sum(a, l, "fused") == 2.0 ** -60
    assert words([BD.shift_sum([], [])])[0] == 0 and words([BD.shift_sum([-0.0], [1.0])])[0] == 0  # starts from +0.0


def test_fma_in_rationals_rounds_once():
    """BD.fma against cases whose single rounding is known, and against the two-step value where both agree."""
    e = 1.0 + 2.0 ** -30
    assert BD.fma(e, e, 0.0) == 1.0 + 2.0 ** -29 == e * e  # one rounding of 1 + 2^-29 + 2^-60
    assert BD.fma(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, -1.0) == 2.0 ** -53 - 2.0 ** -105  # the product alone would round to 1 + 2^-53 -> 1.0
    assert BD.fma(3.0, 5.0, 7.0) == 22.0 and BD.fma(1e308, 10.0, 0.0) == math.inf and BD.fma(-1e308, 10.0, 0.0) == -math.inf
    assert words([BD.fma(0.0, -1.0, 0.0)])[0] == 0 and words([BD.fma(0.0, -1.0, -0.0)])[0] == words([-0.0])[0]  # -0 + +0, -0 + -0
    assert words([BD.fma(2.0, 3.0, -6.0)])[0] == 0 and math.isnan(BD.fma(math.inf, 0.0, 1.0)) and BD.fma(math.inf, 1.0, 1.0) == math.inf
    rng = np.random.default_rng(20261202)
    for a, b, c in rng.standard_normal((200, 3)):
        exact = BD.Fraction(float(a)) * BD.Fraction(float(b)) + BD.Fraction(float(c))
        got = BD.fma(a, b, c)
        assert abs(BD.Fraction(got) - exact) <= min(abs(BD.Fraction(float(np.nextafter(got, s))) - exact) for s in (-math.inf, math.inf))


def test_flawed_sums_are_what_their_names_say():
    """Each of BD.SUM_FLAWS on a row where its value is known, beside THE order's."""
    one = np.ones(65)
    a = np.zeros(65)
    a[0], a[64], a[1] = 1e16, 1.0, -1e16
    assert BD.flawed_shift_sum(a, one, "left to right") == 1.0 and BD.shift_sum(a, one) == 0.0
    b = np.zeros(64)
    b[0], b[32], b[16] = 1e16, -1e16, 1.0  # THE order: lanes 0 and 32 meet first; upward, lanes 0 .. 15 swallow lane 16 first
    assert BD.shift_sum(b, np.ones(64)) == 1.0 and BD.flawed_shift_sum(b, np.ones(64), "fold upward") == 0.0
    b[0], b[32], b[16] = 1e16, 1.0, -1e16
    assert BD.shift_sum(b, np.ones(64)) == 0.0 and BD.flawed_shift_sum(b, np.ones(64), "fold upward") == 1.0
    # 32 lanes: up to n = 64 they ARE the order (lane k of 32 is p[k] + p[k + 32], the first fold of 64), so random rows of 64 columns
    # agree bit for bit; with column 64 the orders part: (a[0] + a[64]) + a[32] against (a[0] + a[32]) + a[64]
    rng = np.random.default_rng(20261203)
    for n in (1, 33, 63, 64):
        r, l = rng.standard_normal(n) * 1e3, rng.standard_normal(n)
        assert words([BD.shift_sum(r, l)])[0] == words([BD.flawed_shift_sum(r, l, "lanes of 32")])[0]
    d = np.zeros(65)
    d[0], d[32], d[64] = 1e16, -1e16, 1.0
    assert BD.shift_sum(d, one) == 0.0 and BD.flawed_shift_sum(d, one, "lanes of 32") == 1.0


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129))
def test_shift_sum_lengths(n):
    """Against an independent statement of the order: the columns of lane k are k, k + 64, ..; the tree is fixed."""
    rng = np.random.default_rng([20261106, n])
    a, l = rng.standard_normal(n) * 1e3, rng.standard_normal(n)
    lanes = [0.0] * 64
    for k in range(min(64, n)):
        for j in range(k, n, 64):
            lanes[k] = lanes[k] + float(a[j]) * float(l[j])
    v = lanes
    while len(v) > 1:
        half = len(v) // 2
        v = [v[k] + v[k + half] for k in range(half)]
    assert words([BD.shift_sum(a, l)])[0] == words([v[0]])[0]
    assert abs(BD.shift_sum(a, l) - float(np.dot(a, l))) <= 1e-9 * float(np.abs(a * l).sum())


# ------------------------------------------------------------------------------------------------------- the hard calls

@pytest.fixture(scope="module")
def hard(oracle):
    return {c.name: c for c in LBD.hard_table(oracle)}


@pytest.mark.parametrize("name", list(LBD.HARD))
def test_hard_calls_tell_every_flaw(oracle, hard, name):
    """The floors the hard fixtures were picked for, with the oracle alone: at least half of the LPs end "optimal"; one takes 8
    pivots or more; every sum flaw changes the bits of a right-hand-side cell of a start tableau, and for n >= 129 some LP's
    shift_sum(c, lb); every read-out flaw changes a word of x or of the objective.  Two exemptions, both for n <= 64, where the
    flawed sum IS the canonical one for every input: "fused" (every lane holds one product, and fma(a, l, +0.0) is the rounded
    product) and "lanes of 32" (lane k of 32 holds p[k] + p[k + 32], which is the first fold of the 64)."""
    call = hard[name]
    assert (LB.size_class(call.w, call.h), int(BS.aux_hbm(call.w, call.h))) == LBD.HARD_FORMS[name]
    refs = LBD.hard_answers(oracle, call)
    statuses, pivots = [r["status"] for r in refs], [r["n_pivots"] for r in refs]
    counts = LBD.discrimination(oracle, call)
    rhs = len(call.lps) * (call.m_ub + 2 * call.m_eq)
    print("%s: %s, pivots %s" % (name, statuses, pivots))
    for flaw, (cells, shifts, answer) in counts.items():
        print("    %-24s %3d of %d right-hand-side cells, shift_sum(c, lb) of %d of %d LPs, %d words of x / objective"
              % (flaw, cells, rhs, shifts, len(call.lps), answer))
    assert 2 * statuses.count("optimal") >= len(statuses) and max(pivots) >= 8, (name, statuses, pivots)
    for flaw in BD.SUM_FLAWS:
        same_function = call.n <= 64 and flaw in ("fused", "lanes of 32")
        assert counts[flaw][0] >= (0 if same_function else 1), (name, flaw, counts[flaw])
        assert not same_function or counts[flaw] == (0, 0, 0), (name, flaw, counts[flaw])
        assert call.n < 129 or counts[flaw][1] >= 1, (name, flaw, counts[flaw])
    for flaw in BD.READ_FLAWS:
        assert counts[flaw][2] >= 1 and counts[flaw][:2] == (0, 0), (name, flaw, counts[flaw])


def test_both_statements_of_the_order_agree_on_every_hard_row(oracle, hard):
    rows = 0
    for call in hard.values():
        if not call.has_lb:
            continue
        for lp, lb in zip(call.lps, call.lbs):
            c, A_ub, _, A_eq, _ = lp
            for a in [c] + list(np.asarray(A_ub).reshape(call.m_ub, call.n)) + ([] if A_eq is None else list(np.asarray(A_eq).reshape(call.m_eq, call.n))):
                assert words([BD.shift_sum(a, lb)])[0] == words([BD.shift_sum_lanes(a, lb)])[0], call.name
                rows += 1
    assert rows > 400, rows


def test_pins_hold_their_known_values(oracle, hard):
    """Cell (1, 0) of every pin's start tableau: the canonical word, and the wrong one under the flaw the pin is for."""
    for name, pins in ((LBD.PIN_NAMES[0], LBD.PINS_65), (LBD.PIN_NAMES[1], LBD.PINS_64)):
        call = hard[name]
        assert len(pins) == len(call.lps) and call.has_lb and not call.has_ub and call.k == 0
        for i, (want, flaw, wrong) in enumerate(pins):
            start = LBD.hard_answers(oracle, call)[i]["start"]
            assert words(start[call.w:call.w + 1])[0] == words([want])[0], (name, i, start[call.w], want)
            if flaw is not None:
                bad = LBD.hard_answers(oracle, call, flaw)[i]["start"]
                assert words(bad[call.w:call.w + 1])[0] == words([wrong])[0], (name, i, flaw, bad[call.w], wrong)
        at0 = LBD.at_budget_0(call)
        assert all(r["status"] == "cycled" and r["n_pivots"] == 0 for r in LBD.hard_answers(oracle, at0))
    # the one addition to the objective: -0.0 without lb, -0.0 + shift_sum(c, 0) = -0.0 + +0.0 = +0.0 with lb = 0
    with_lb, without = hard[LBD.PIN_NAMES[2]], hard[LBD.PIN_NAMES[3]]
    a, b = LBD.hard_answers(oracle, with_lb)[0], LBD.hard_answers(oracle, without)[0]
    assert a["status"] == b["status"] == "optimal" and a["n_pivots"] == b["n_pivots"] == 1
    assert np.array_equal(words(a["matrix"]), words(b["matrix"])) and with_lb.k == without.k == 0 and not without.has_lb
    assert words([b["objective"]])[0] == words([-0.0])[0] and words([a["objective"]])[0] == 0, (a["objective"], b["objective"])
    assert words([BD.shift_sum(with_lb.lps[0][0], with_lb.lbs[0])])[0] == 0


# ---------------------------------------------------------------------------------------------------------- restatement

def grid_lp(n, m_ub, m_eq, mode, seed):
    from tests.test_lp_dense_model import random_lp
    rng = np.random.default_rng([20261107, n, m_ub, m_eq, MODES.index(mode), seed])
    lp = random_lp(rng, n, m_ub, m_eq)
    lb = rng.integers(-6, 5, n).astype(np.float64) * 0.25 if mode != "ub" else None
    ub = rng.integers(-4, 9, n).astype(np.float64) * 0.5 if mode != "lb" else None
    return lp, lb, ub


def uppers(n, mode):
    return (True,) if mode == "lb" else (True, (), (0,), (n - 1,))


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m_eq", (0, 1, 2))
@pytest.mark.parametrize("m_ub", (0, 3))
@pytest.mark.parametrize("n", (1, 2, 5))
def test_bounded_tableau_is_the_explicit_route_and_the_equivalent_model(n, m_ub, m_eq, mode, maximize):
    from yalps_amd.model import tableau_model
    for seed in range(2):
        lp, lb, ub = grid_lp(n, m_ub, m_eq, mode, seed)
        for upper in uppers(n, mode):
            k = len(BD.upper_set(n, upper, ub is not None))
            w, h = n + 1, 1 + m_ub + 2 * m_eq + k
            m = BD.bounded_tableau(*lp, lb=lb, ub=ub, upper=upper, maximize=maximize)
            assert m.size == w * h
            explicit = ND.dense_tableau(*BD.explicit_operands(*lp, lb=lb, ub=ub, upper=upper), maximize=maximize).reshape(h, w)
            assert np.array_equal(words(m), words(explicit[BD.explicit_rows(m_ub, m_eq, k)].ravel())), (n, m_ub, m_eq, mode, upper)
            t = tableau_model(BD.equivalent_model(*lp, lb=lb, ub=ub, upper=upper, maximize=maximize)).tableau
            assert (t.width, t.height) == (w, h)
            assert np.array_equal(words(m), words(t.matrix)), (n, m_ub, m_eq, mode, upper, maximize, seed)
            assert words(m[:1])[0] == 0  # cell (0, 0) stays +0.0
            if lb is None:  # no subtraction at all: the right-hand sides are the caller's bits (a -0.0 stays one)
                plain = ND.dense_tableau(*lp, maximize=maximize)
                assert np.array_equal(words(m[:plain.size]), words(plain))


def test_upper_set_refuses():
    for bad in ((0, 0), (3,), (-1,)):
        with pytest.raises(ValueError):
            BD.upper_set(3, bad)
    assert BD.upper_set(3, (2, 0)) == (0, 2) and BD.upper_set(3, True) == (0, 1, 2) and BD.upper_set(3, True, has_ub=False) == ()


# ---------------------------------------------------------------------------------------------------------------- solves

SOLVE_SHAPES = ((5, 4, 0), (5, 4, 1), (6, 3, 3), (4, 0, 2), (1, 2, 0), (2, 0, 1), (5, 0, 0))
SOLVE_SEEDS = 12


def solve_calls(shape, maximize):
    n, m_ub, m_eq = shape
    out = []
    for mode in MODES:
        for upper in ((True,) if mode == "lb" else (True, (0,), (n - 1,))):
            out.append(LBD.random_call("solves %s %s" % (mode, upper), SOLVE_SEEDS, n, m_ub, m_eq, mode=mode, upper=upper, maximize=maximize))
    return out


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("shape", SOLVE_SHAPES)
def test_solves_respect_the_bounds_and_the_identities(oracle, shape, maximize):
    optimal, worst = 0, [0.0, 0.0, 0.0]
    for call in solve_calls(shape, maximize):
        for i, lp in enumerate(call.lps):
            ref = call.oracle_answer(oracle, i)
            lb, ub = call.lbs[i], call.ubs[i]
            if ref["status"] != "optimal":
                assert all(np.isnan(ref[k]).all() for k in LBD.OUTPUTS)
                continue
            optimal += 1
            low = np.zeros(call.n) if lb is None else lb
            leave = max(float((low - ref["x"]).max()), max([float(ref["x"][j] - ub[j]) for j in call.idx], default=0.0), 0.0)
            r_obj, r_red = BD.identity_residuals(lp, lb, ub, call.idx, ref["objective"], *(ref[k] for k in LBD.OUTPUTS))
            worst = [max(a, b) for a, b in zip(worst, (leave, r_obj, r_red))]
            assert leave <= FEASIBILITY and r_obj <= OBJECTIVE_RESIDUAL and r_red <= REDUCED_RESIDUAL, (call.name, i, leave, r_obj, r_red)
            assert not (words(np.concatenate([ref[k] for k in LBD.OUTPUTS])) == np.int64(-2 ** 63)).any()  # (the + 0.0: no -0.0)
    print("shape %s maximize=%s: %d optimal, leaves the box by %.3g, residuals %.3g %.3g" % (shape, maximize, optimal, *worst))
    assert optimal >= 12, (shape, maximize, optimal)


def lp_of(c, A, b, lb, ub):
    a = lambda v: None if v is None else np.array(v, np.float64)
    return (a(c), a(A), a(b), None, None, a(lb), a(ub))


def test_three_endings_bounds_add(oracle):
    # a negative lower bound, and the optimum at a negative x: minimise x0 + x1 with x >= (-3, -2)
    call = LBD.BCall("negative", [lp_of([1.0, 1.0], [[1.0, 1.0]], [4.0], [-3.0, -2.0], None)])
    ref = call.oracle_answer(oracle, 0)
    assert ref["status"] == "optimal" and ref["x"].tolist() == [-3.0, -2.0] and ref["objective"] == -5.0
    assert ref["reduced"].tolist() == [1.0, 1.0] and ref["ineqlin"].tolist() == [0.0]
    # lb > ub on one variable: infeasible
    call = LBD.BCall("crossed", [lp_of([1.0, 1.0], [[1.0, 1.0]], [9.0], [0.0, 2.0], [5.0, 1.0])])
    ref = call.oracle_answer(oracle, 0)
    assert ref["status"] == "infeasible" and np.isnan(ref["x"]).all() and math.isnan(ref["objective"]) and np.isnan(ref["upper"]).all()
    # unbounded through the variable `upper` does not list; its +inf stays +inf after the shift, the others are lb
    call = LBD.BCall("unlisted", [lp_of([0.0, 1.0], [[1.0, -1.0]], [9.0], [-1.0, -4.0], [3.0, 3.0])], upper=(0,), maximize=True)
    ref = call.oracle_answer(oracle, 0)
    assert ref["status"] == "unbounded" and ref["x"].tolist() == [-1.0, math.inf] and ref["objective"] == math.inf
    listed = LBD.BCall("listed", [lp_of([1.0, 1.0], [[1.0, -1.0]], [2.0], [-1.0, -4.0], [3.0, 3.0])], maximize=True)
    ref = listed.oracle_answer(oracle, 0)
    assert ref["status"] == "optimal" and ref["x"].tolist() == [3.0, 3.0] and ref["upper"].tolist() == [1.0, 1.0]


# ------------------------------------------------------------------------------------------------------------- gradients

def test_bound_gradient_formulas_against_central_differences(oracle):
    """d lb = reduced_costs, d ub = upper, against central differences of the oracle's objective: data in eighths, step 2^-6,
    precision 1e-8, so a quotient is off by at most precision / h (tests/_np_dense_duals.py says why); every perturbed LP ends in
    the base's basis."""
    call = LBD.difference_call()
    refs = [call.oracle_answer(oracle, i) for i in range(len(call.lps))]
    assert all(r["status"] == "optimal" and np.array_equal(r["pos"], refs[0]["pos"]) for r in refs)
    obj = [r["objective"] for r in refs]
    numeric = np.array([(obj[1 + 2 * e] - obj[2 + 2 * e]) / (2.0 * LBD.GRAD_H) for e in range(6)])
    formulas = np.concatenate([refs[0]["reduced"], refs[0]["upper"]])
    assert np.count_nonzero(refs[0]["reduced"]) and np.count_nonzero(refs[0]["upper"]) and np.count_nonzero(refs[0]["ineqlin"])
    assert (np.abs(numeric - formulas) <= LBD.GRAD_PRECISION / LBD.GRAD_H).all(), (numeric, formulas)


def test_bounded_objective_backward_formulas_on_the_host():
    """_BoundedObjective.backward is torch arithmetic on saved tensors: hand-made ones on the CPU.  A row that did not end
    optimal contributes exact zeros; d ub is scattered into zeros at the listed variables."""
    import torch
    from yalps_amd import tensors
    nan = float("nan")
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    x, status = t([[1.0, 2.0, -1.0], [nan, nan, nan]]), torch.tensor([0, 1], dtype=torch.int32)
    ineqlin, eqlin = t([[0.5], [nan]]), t([[], []])
    reduced, marg = t([[0.0, -3.0, 0.25], [nan, nan, nan]]), t([[4.0, 0.0], [nan, nan]])

    class Ctx:
        saved_tensors = (x, status, ineqlin, eqlin, reduced, marg)
        sides, bounds, upper = (True, False), (True, True), [0, 2]
        needs_input_grad = (False, False, True, True, True, False, False, True, True)
    g = t([2.0, 5.0])
    got = tensors._BoundedObjective.backward(Ctx, g)
    assert len(got) == 9 and got[0] is None and got[1] is None and got[5] is None and got[6] is None
    assert got[2].tolist() == [[2.0, 4.0, -2.0], [0.0, 0.0, 0.0]] and got[4].tolist() == [[1.0], [0.0]]
    assert got[3].tolist() == [[[-1.0, -2.0, 1.0]], [[0.0, 0.0, 0.0]]] or got[3][0].tolist() == [[-1.0, -2.0, 1.0]]
    assert got[7].tolist() == [[0.0, -6.0, 0.5], [0.0, 0.0, 0.0]]
    assert got[8].tolist() == [[8.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert not any(torch.isnan(v).any() for v in got if v is not None)


# ------------------------------------------------------------------------------------------------------- argument checks

FAKE = 4096  # a pointer value no check dereferences


def test_new_entries_refuse_on_the_host(nat):
    L = nat.lpdense_lib()
    for s in ("yalps_lpdense_solve_bounds", "yalps_lpdense_validate_bounds"):
        assert s in nat.SYMBOLS_LPDENSE and hasattr(L, s)
    null = [None] * 5
    rc = L.yalps_lpdense_solve_bounds(None, 1, 1, 1, 0, *null, None, None, 0, None, 0, 1e-8, 8192.0, 0, 0, *([None] * 8), None)
    assert rc == -1 and L.yalps_lpdense_last_error() == b"yalps_lpdense_solve_bounds: handle is NULL"
    ops = [(FAKE, 3, 1, 0), (FAKE, 6, 3, 1), (FAKE, 2, 1, 0), None, None]
    vec = (FAKE, 3, 1, 0)
    nat.lpdense_validate_bounds(2, 3, 2, 0, ops, lb=vec, ub=vec, upper=(0, 2))
    nat.lpdense_validate_bounds(2, 3, 2, 0, ops)  # no bounds: yalps_lpdense_validate
    nat.lpdense_validate_bounds(2, 3, 2, 0, ops, ub=(None, 0, 0, 0))  # ub without a listed variable is never read
    for kw, reason in ((dict(lb=(FAKE, 3, -1, 0)), "lb: negative stride"), (dict(ub=(FAKE, -3, 1, 0), upper=(0,)), "ub: negative stride"),
                       (dict(lb=(None, 3, 1, 0)), "lb is NULL"), (dict(ub=(None, 3, 1, 0), upper=(1,)), "ub is NULL"),
                       (dict(ub=vec, upper=(0, 3)), "outside 0 .. n-1"), (dict(ub=vec, upper=(-1,)), "outside 0 .. n-1"),
                       (dict(ub=vec, upper=(1, 1)), "not ascending"), (dict(ub=vec, upper=(2, 0)), "not ascending"),
                       (dict(upper=(0,)), "without ub")):
        with pytest.raises(nat.NativeError, match=re.escape(reason)):
            nat.lpdense_validate_bounds(2, 3, 2, 0, ops, **kw)
    # the size limit counts the bound rows: 512 x (1 + 511 + 511) is 4 MiB exactly, one more row is above it
    big = [(FAKE, 0, 1, 0), (FAKE, 0, 511, 1), (FAKE, 0, 1, 0), None, None]
    wide = (FAKE, 0, 1, 0)
    nat.lpdense_validate_bounds(1, 511, 512, 0, big, ub=wide, upper=range(511))
    with pytest.raises(nat.NativeError, match="above the limit"):
        nat.lpdense_validate_bounds(1, 511, 513, 0, big, ub=wide, upper=range(511))
    header = open(os.path.join(ROOT, "include", "yalps_lpdense.h")).read()
    for word in ("upper_out[count][n_upper]", "shift_sum", "upper.marginals", "REPLACES x >= 0", "-inf is taken as it lies"):
        assert word in header, word


def test_bounds_are_checked_before_the_library(nat, monkeypatch):
    import inspect
    import torch
    from yalps_amd import tensors
    monkeypatch.setattr(nat, "LpDense", lambda *a, **k: pytest.fail("the library was touched"))
    sig = inspect.signature(tensors.linprog_batch).parameters
    for name, default in (("lb", None), ("ub", None), ("upper", True)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is default
    assert tensors.LinprogBoundDuals._fields == tensors.LinprogDuals._fields + ("upper",) and len(tensors.LinprogDuals._fields) == 7
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    for call, who in ((tensors.linprog_batch, "linprog_batch"), (tensors.linprog_objective_bounds, "linprog_objective_bounds")):
        with pytest.raises(ValueError, match="twice"):
            call(z(3), z(2, 3), z(2), ub=z(3), upper=(1, 1))
        with pytest.raises(ValueError, match="outside 0 .. 2"):
            call(z(3), z(2, 3), z(2), ub=z(3), upper=(3,))
        with pytest.raises(ValueError, match="outside 0 .. 2"):
            call(z(3), z(2, 3), z(2), ub=z(3), upper=(-1,))
        with pytest.raises(ValueError, match="no ub was given"):
            call(z(3), z(2, 3), z(2), lb=z(3), upper=())
        with pytest.raises(TypeError, match="float32"):
            call(z(3), z(2, 3), z(2), lb=z(3).float())
        with pytest.raises(TypeError, match="torch.Tensor"):
            call(z(3), z(2, 3), z(2), ub=np.zeros(3))
        with pytest.raises(ValueError, match="lb has 4 entries"):
            call(z(3), z(2, 3), z(2), lb=z(4))
        with pytest.raises(ValueError, match="disagree about B"):
            call(z(5, 3), z(2, 3), z(2), ub=z(4, 3))
        with pytest.raises(ValueError, match="dimensions"):
            call(z(3), z(2, 3), z(2), lb=z(2, 2, 3))
        with pytest.raises(ValueError, match="CPU tensor"):
            call(z(3), z(2, 3), z(2), lb=z(3), ub=z(3), upper=[2, 0])
    with pytest.raises(ValueError, match=r"solve\(\)"):
        tensors.linprog_batch(z(511), z(513, 511), z(513), ub=z(511))  # 1025 rows with the 511 bound rows
    with pytest.raises(ValueError, match="CPU tensor"):
        tensors.linprog_batch(z(511), z(513, 511), z(513), ub=z(511), upper=range(510))  # 4 MiB exactly passes the size check
    with pytest.raises(ValueError, match="CPU tensor"):
        tensors.linprog_batch(z(511), z(1023, 511), z(1023), lb=z(511))  # lb adds no row


def test_bounds_kernels_pass_the_register_budget(nat):
    """The six bounded forms are a code object of their own, under the same build gate: no scratch, no accumulator registers,
    within 128 VGPRs, static LDS a multiple of 16."""
    from yalps_amd import build
    ks = build.check_register_budgets(build.LIB_LPDENSE_BOUNDS, min_resident=0)
    assert len(ks) == 6 and all("lp_dense_bounds_kernel" in k for k in ks), sorted(ks)
    for k, md in ks.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0 and int(md["vgpr_count"]) <= 128, (k, md)
        assert int(md["group_segment_fixed_size"]) % 16 == 0
