"""Sensitivity analysis of LP batches (include/yalps_lpsens.h, yalps_amd.sensitivity): libyalps_lpsens.so's boundary and its
kernels by name, and the mapping from the five native arrays to duals, reduced costs and ranges, driven on the CPU by the C
oracle plus the numpy restatement (tests/_np_sensitivity.py) and checked by finite differences; on the GPU every
instantiation, the shape table, the golden and edge records, the work queue, the history rerun, handle reuse, the large-LP
route and sensitivity_many on every golden LP case.

Comparisons: the solve as tests/_lp_batch.check_lp compares it (bit for bit); row0 bit for bit; the four ratio arrays equal as
numbers, infinities included."""
import copy
import math
import os
import re

import numpy as np
import pytest

from tests import _batch_shapes as BS
from tests import _cases as K
from tests import _golden as G
from tests import _lp_batch as B
from tests import _np_sensitivity as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf

# kernel spelling -> (size class, checkCycles)
KERNELS = {
    "lp_sens_kernel<256,lds>": (0, False),
    "lp_sens_kernel<256,check,lds>": (0, True),
    "lp_sens_kernel<1024,lds>": (3, False),
    "lp_sens_kernel<1024,check,lds>": (3, True),
    "lp_sens_kernel<1024>": (4, False),
    "lp_sens_kernel<1024,check>": (4, True),
}
NO_OBJECTIVE = 8  # golden models without an `objective` key (three of them infeasible): only their constraint sides are checked


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpsens()
    return _native


# ---------------------------------------------------------------------------------------------------------- CPU

def test_header_symbols_are_exported(nat):
    text = open(os.path.join(ROOT, "include", "yalps_lpsens.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text))
    assert declared and all(s.startswith("yalps_lpsens_") for s in declared), declared
    L = nat.lpsens_lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(nat.SYMBOLS_LPSENS)
    for other in (nat.SYMBOLS, nat.SYMBOLS_LPBATCH, nat.SYMBOLS_MILPBATCH, nat.SYMBOLS_LPVAR):
        assert not set(nat.SYMBOLS_LPSENS) & set(other)


def test_kernels_are_the_table_and_stay_out_of_the_other_libraries(nat):
    from yalps_amd import build
    ks = build.kernel_metadata(lib=build.LIB_LPSENS)
    spelt = {NS.spelling(s): md for s, md in ks.items()}
    assert len(spelt) == len(ks)
    assert set(spelt) == set(KERNELS), sorted(set(spelt) ^ set(KERNELS))
    for name, md in spelt.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0, (name, md)
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (name, md["group_segment_fixed_size"])
    assert "lp_sens" in build.NO_SCRATCH
    build.check_register_budgets(lib=build.LIB_LPSENS, min_resident=0)
    build.build_hip()
    build.build_lpbatch()
    build.build_milpbatch()
    build.build_lpvar()
    for lib in (build.LIB, build.LIB_LPBATCH, build.LIB_MILPBATCH, build.LIB_LPVAR):
        assert not [s for s in build.kernel_metadata(lib) if "lp_sens" in s], lib


def test_no_cpu_fallback(nat):
    from yalps_amd import build
    build.build_hip()
    if nat.lib().yalps_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(nat.NativeError, match="no HIP device"):
        nat.LpSens(0)


def test_argument_errors_name_the_lp_before_any_device_call(nat, oracle):
    """yalps_lpsens_validate is what yalps_lpsens_solve runs first; it needs no device."""
    good = B.dense_lp(oracle, 5, 4, 1)
    too_big = (1024, 513, *good[2:])
    unsorted_ = (good[0], good[1], good[2][::-1].copy(), good[3][::-1].copy(), good[4][::-1].copy(), *good[5:])
    outside = (good[0], good[1], good[2], good[3] + good[0], good[4], *good[5:])
    for bad, what in ((too_big, "above the batch limit"), (unsorted_, "not sorted"), (outside, "outside"),
                      ((0, 3, *good[2:]), "at least 1"), ((3, 0, *good[2:]), "at least 1")):
        with pytest.raises(nat.NativeError, match="yalps_lpsens: LP 2: .*" + what):
            nat.lpsens_validate(nat.PackedLps([good, good, bad, good]))
    nat.lpsens_validate(nat.PackedLps([good, good]))
    nat.lpsens_validate(nat.PackedLps([]))


def test_the_restatement_and_the_product_ranging_on_a_hand_tableau():
    """A final matrix small enough to range by hand: an odd n, empty sets, an entry within the precision, NaN quotients
    (inf / inf) that are ignored and a -0.0 quotient that is not."""
    from yalps_amd.sensitivity import ranges_from_tableau
    M = np.array([[-36.0, -1.5, 0.0, -1.0],
                  [2.0, 0.5, 0.0, -0.25],
                  [6.0, -2.0, 0.0, 4.0],
                  [INF, INF, 1e-9, -INF]])
    want = (M[0], [0.0, 4.0, INF, 1.5], [0.0, 3.0, INF, 8.0], [0.0, -3.0, -0.25, -0.0], [0.0, 4.0, 0.75, 0.0])
    for got in (NS.restate(M.ravel(), 4, 4, 1e-8), ranges_from_tableau(M.ravel(), 4, 4, 1e-8)):
        NS.check_ranges(got, tuple(np.array(a, np.float64) for a in want))
    for w, h in ((1, 1), (1, 3), (3, 1)):
        m = np.arange(w * h, dtype=np.float64)
        NS.check_ranges(ranges_from_tableau(m, w, h, 1e-8), NS.restate(m, w, h, 1e-8))


TEXTBOOK = {
    "direction": "maximize", "objective": "profit",
    "constraints": {"plant1": {"max": 4}, "plant2": {"max": 12}, "plant3": {"max": 18}},
    "variables": {"x": {"profit": 3, "plant1": 1, "plant3": 3}, "y": {"profit": 5, "plant2": 2, "plant3": 2}},
}


def test_textbook_example(oracle):
    r = NS.oracle_sensitivity(oracle, [TEXTBOOK])[0]
    assert (r["status"], r["result"], r["variables"]) == ("optimal", 36.0, [("x", 2.0), ("y", 6.0)])
    cons, vars_ = r["sensitivity"]["constraints"], r["sensitivity"]["variables"]
    assert [k for k, _ in cons] == ["plant1", "plant2", "plant3"] and [k for k, _ in vars_] == ["x", "y"]
    assert [c["dual"] for _, c in cons] == [0.0, 1.5, 1.0]
    assert [c["upper_range"] for _, c in cons] == [(2.0, INF), (6.0, 18.0), (12.0, 24.0)]
    assert all("lower_range" not in c for _, c in cons)
    assert [v["objective_range"] for _, v in vars_] == [(0.0, 7.5), (2.0, INF)]
    assert [v["reduced_cost"] for _, v in vars_] == [0.0, 0.0]


def merged_constraint(bound, lower=None, upper=None):
    lo, hi = bound["lower"] if lower is None else lower, bound["upper"] if upper is None else upper
    out = {}
    if math.isfinite(lo):
        out["min"] = lo
    if math.isfinite(hi):
        out["max"] = hi
    return out


def halfway(value, lo, hi):
    """The two steps: halfway to each end of [lo, hi]; an infinite end is capped at max(1, |value|) away."""
    cap = max(1.0, abs(value))
    return [(end if math.isfinite(end) else value + sign * cap) / 2.0 - value / 2.0 for end, sign in ((lo, -1.0), (hi, 1.0))]


def finite_differences(oracle, model, options, own_side=False):
    """[(what, status, objective, predicted, old)] of every step of the property: every side of every constraint that is not
    `equal` and, where the model has an objective, every variable's coefficient, moved halfway to each end of its range and
    re-solved through the oracle; the objective is predicted to move by dual * delta, respectively delta * value.
    [] where the model is not optimal.
    own_side: a stricter reading for two-sided constraints.  "dual" is one number per constraint, and at most one side of a
    constraint that is not `equal` binds; moving the side that does not bind leaves the objective alone.  The side that binds
    is known from the sign: raising an upper bound can only help the objective (sign * dual > 0), raising a lower bound only
    hurt it.  With own_side the prediction for a side is dual * delta where the dual is that side's, and 0 where it is the
    other's; an `equal` constraint is then moved as a whole, both sides by +-1e-3, and predicted to move by dual * delta."""
    from yalps_amd.model import apply_variant, entries, tableau_model_with_bounds
    base = NS.oracle_sensitivity(oracle, [model], options)[0]
    if base["status"] != "optimal":
        assert base["sensitivity"] is None
        return []
    old, sens = base["result"], base["sensitivity"]
    bounds = tableau_model_with_bounds(model, sparse=True)[1]["bounds"]
    assert [k for k, _ in sens["constraints"]] == list(bounds)
    out = []

    def resolve(what, variant, predicted):
        r = NS.oracle_sensitivity(oracle, [apply_variant(model, variant)], options)[0]
        out.append((what, r["status"], r["result"], predicted, old))

    sign = -1.0 if model.get("direction") == "minimize" else 1.0
    for key, c in sens["constraints"]:
        b = bounds[key]
        if b["lower"] == b["upper"]:
            for delta in ((-1e-3, 1e-3) if own_side else ()):
                resolve((key, "equal", delta), {"constraints": {key: {"equal": b["upper"] + delta}}}, old + c["dual"] * delta)
            continue
        for side, name in (("upper", "upper_range"), ("lower", "lower_range")):
            assert (name in c) == math.isfinite(b[side]), (key, name)
            if name not in c:
                continue
            lo, hi = c[name]
            slack = 1e-7 * max(1.0, abs(b[side]))  # (a basic slack may stand at -1e-12)
            assert lo - slack <= b[side] <= hi + slack, (key, name, c[name], b[side])
            for delta in halfway(b[side], lo, hi):
                mine = not own_side or sign * c["dual"] * (1.0 if side == "upper" else -1.0) > 0
                resolve((key, side, delta), {"constraints": {key: merged_constraint(b, **{side: b[side] + delta})}},
                        old + (c["dual"] if mine else 0.0) * delta)
    objective = model.get("objective")
    if objective is None:
        return out
    variables = entries(model["variables"])
    assert len({k for k, _ in variables}) == len(variables) == len(sens["variables"])
    values = dict(base["variables"])
    for (key, coefs), (skey, v) in zip(variables, sens["variables"]):
        assert key == skey
        coef = float(dict(entries(coefs)).get(objective, 0.0))
        lo, hi = v["objective_range"]
        assert lo <= coef <= hi, (key, v, coef)
        for delta in halfway(coef, lo, hi):
            resolve((key, "objective", delta), {"variables": {key: {objective: coef + delta}}}, old + delta * values.get(key, 0.0))
    return out


def assert_property(steps, name):
    for what, status, got, predicted, old in steps:
        print(name, what, status, got, predicted)
        assert status == "optimal", (name, what, status)
        assert abs(got - predicted) <= 1e-7 * max(1.0, abs(old), abs(predicted)), (name, what, got, predicted)


MINIMISE = {
    "direction": "minimize", "objective": "cost",
    "constraints": {"protein": {"min": 10}, "fat": {"min": 5, "max": 8}, "fibre": {"equal": 4}, "salt": {"max": 3},
                    "sugar": {"min": 1, "max": 20}},
    "variables": {"a": {"cost": 2.0, "protein": 3, "fat": 1, "fibre": 1, "salt": 0.5, "sugar": 1},
                  "b": {"cost": 3.0, "protein": 1, "fat": 2, "fibre": 0.5, "salt": 0.2, "sugar": 2},
                  "c": {"cost": 1.5, "protein": 0.5, "fat": 0.2, "fibre": 2, "salt": 0.1, "sugar": 0.5},
                  "d": {"cost": 9.0, "protein": 1, "fat": 0.1, "fibre": 0.1, "salt": 1, "sugar": 0.1}},
}


def test_minimise_model_with_min_equal_and_two_sided_constraints(oracle):
    r = NS.oracle_sensitivity(oracle, [MINIMISE])[0]
    assert r["status"] == "optimal"
    cons, vars_ = dict(r["sensitivity"]["constraints"]), dict(r["sensitivity"]["variables"])
    assert set(cons["protein"]) == {"dual", "lower_range"} and set(cons["salt"]) == {"dual", "upper_range"}
    for key in ("fat", "fibre", "sugar"):
        assert set(cons[key]) == {"dual", "upper_range", "lower_range"}
    # a binding `min` of a minimisation costs money: its dual is positive; d is too dear to be used
    # (fat binds at its lower side alone: moving its upper side, within that side's range, leaves the objective alone)
    assert cons["fat"]["dual"] > 0 and cons["fat"]["upper_range"] == (5.0, INF)
    assert cons["protein"]["dual"] > 0 and vars_["d"]["reduced_cost"] > 0 and "d" not in dict(r["variables"])
    assert vars_["d"]["objective_range"][1] == INF and vars_["d"]["objective_range"][0] == 9.0 - vars_["d"]["reduced_cost"]
    steps = finite_differences(oracle, MINIMISE, None, own_side=True)
    assert len(steps) == 2 * (6 + 1 + 4)  # six sides, the `equal` constraint as a whole, four coefficients
    assert -1e-3 <= cons["fibre"]["upper_range"][0] - 4.0 <= 0 <= cons["fibre"]["lower_range"][1] - 4.0 <= 1e-3
    assert_property(steps, "minimise")
    # every sign: some step of a bound and some step of a coefficient moved the objective up, another down
    moved = [(what[1], predicted - old) for what, _, _, predicted, old in steps]
    assert cons["fibre"]["dual"] != 0
    for kind in ("lower", "equal", "objective"):
        assert any(k == kind and d > 1e-6 for k, d in moved) and any(k == kind and d < -1e-6 for k, d in moved), kind


def lp_cases():
    """Every golden model but the three large ones, integrality dropped."""
    out = []
    for name in K.names():
        if name in K.LARGE:
            continue
        case = K.load(name)
        model = {k: v for k, v in case["model"].items() if k not in ("integers", "binaries")}
        out.append((name, model, case["options"]))
    return out


def test_finite_difference_property_on_the_golden_models(oracle):
    cases = lp_cases()
    assert len(cases) == 43 and sum(1 for _, m, _ in cases if m.get("objective") is None) == NO_OBJECTIVE
    checked = 0
    for name, model, options in cases:
        steps = finite_differences(oracle, model, options)
        assert_property(steps, name)
        checked += len(steps)
    print('checked', checked)
    assert checked > 800, checked


def test_routing_statuses_and_option_lists(oracle):
    from yalps_amd.sensitivity import _sensitivity_many_with
    from tests.test_lp_batch import large_lp_model, oracle_backend, same_solution
    from yalps_amd import solve as S
    infeasible = {"direction": "maximize", "objective": "p", "constraints": {"a": {"max": 1}, "b": {"min": 2}},
                  "variables": {"x": {"p": 1, "a": 1, "b": 1}}}
    unbounded = {"direction": "maximize", "objective": "p", "constraints": {"a": {"min": 1}}, "variables": {"x": {"p": 1, "a": 1}}}
    models = [TEXTBOOK, infeasible, large_lp_model(), unbounded, MINIMISE, TEXTBOOK]
    options = [None, {}, None, {"precision": 1e-9}, {"checkCycles": True}, {"maxPivots": 1}]
    seen, stats = {}, {}
    got = _sensitivity_many_with(*NS.oracle_backends(oracle, seen), models, options, stats)
    assert stats == {"batched": 5, "large": 1} and seen == {"batch_calls": 1, "batched": 5, "large": 1}
    assert [r["status"] for r in got] == ["optimal", "infeasible", "optimal", "unbounded", "optimal", "cycled"]
    for r, m, o in zip(got, models, options):
        assert set(r) == {"status", "result", "variables", "sensitivity"}
        assert same_solution(r, S._solve_with(oracle_backend(oracle), m, o))
        assert (r["sensitivity"] is None) == (r["status"] != "optimal")
    big = got[2]["sensitivity"]
    assert len(big["constraints"]) == 700 and len(big["variables"]) == 800
    # one option set for all, an empty batch, wrong lengths, integers
    one = _sensitivity_many_with(*NS.oracle_backends(oracle), [TEXTBOOK, MINIMISE], {"precision": 1e-9})
    assert [r["status"] for r in one] == ["optimal", "optimal"]
    assert _sensitivity_many_with(*NS.oracle_backends(oracle), []) == []
    with pytest.raises(ValueError, match="3 models but 2 option sets"):
        _sensitivity_many_with(*NS.oracle_backends(oracle), models[:3], [{}, {}])
    for extra in ({"integers": ["x"]}, {"binaries": ["y"]}, {"integers": True}):
        seen = {}
        with pytest.raises(ValueError, match="model 1 has integer or binary variables"):
            _sensitivity_many_with(*NS.oracle_backends(oracle, seen), [TEXTBOOK, dict(TEXTBOOK, **extra)])
        assert seen == {}  # (refused before anything is solved)
    assert S.sensitivity_many.__doc__ and "branch-and-cut" in S.sensitivity_many.__doc__ and "branch-and-cut" in S.sensitivity.__doc__


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu(nat):
    from yalps_amd import build
    build.build_hip()
    assert nat.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return nat


@pytest.fixture(scope="module")
def sens(gpu):
    s = gpu.LpSens(0)
    yield s
    s.close()


def launches_of(info, passes=(0,)):
    return sorted((k["kernel"], k["class"], k["lps"]) for k in info["kernels"] if k["pass"] in passes)


def solve_and_check(s, lps, oracle, labels=None, refs=None):
    out = s.solve(lps, keep_tableaux=True)
    refs = refs or [B.oracle_answer(oracle, lp) for lp in lps]
    for i, (lp, ref) in enumerate(zip(lps, refs)):
        NS.check_lp(s, i, out, ref, lp, tag=labels[i] if labels else "")
    return refs


@pytest.mark.gpu
def test_every_instantiation_by_name(sens, oracle):
    shapes = ((30, 30), (130, 120), (300, 280), (30, 29), (300, 279))
    lps = [B.dense_lp(oracle, M, N, 3 + k, check_cycles=check) for check in (False, True) for k, (M, N) in enumerate(shapes)]
    refs = solve_and_check(sens, lps, oracle, ["%dx%d" % (lp[1], lp[0]) for lp in lps])
    assert all(r["status"] == "optimal" for r in refs)
    want = []
    for name, (cls, check) in KERNELS.items():
        want.append((name, cls, sum(1 for lp in lps if B.size_class(lp[0], lp[1]) == cls and lp[7] == check)))
    assert launches_of(sens.info()) == sorted(want) and all(n > 0 for _, _, n in want)


@pytest.mark.gpu
def test_shape_table_as_one_batch(sens, oracle):
    shapes = BS.shape_table(oracle)
    lps = [lp for _, lp in shapes]
    refs = solve_and_check(sens, lps, oracle, [name for name, _ in shapes])
    endings = {r["status"] for r in refs}
    assert endings == {"optimal", "infeasible", "unbounded", "cycled"}
    # budgets 0 and n / 2 of the aux rows end "cycled": no ranges (checked above through yalps_lpsens_ranges' E_ARG)
    assert sum(1 for (name, _), r in zip(shapes, refs) if name.startswith("aux") and r["status"] == "cycled") >= 10
    info = sens.info()
    assert info["reruns"] == 0 and {k["kernel"] for k in info["kernels"]} <= set(KERNELS)


@pytest.mark.gpu
def test_golden_and_edge_records_in_one_batch(sens, oracle):
    from tests import _edges as E
    recs = [(r, B.record_lp, G.label) for kind in ("cases", "mixed", "dense") for r in G.records(kind)]
    recs += [(r, B.edge_lp, E.label) for r in G.records("edges")]
    kept = [(r, make, label) for r, make, label in recs if B.size_class(r["width"], r["height"]) >= 0]
    assert len(kept) == 104 + 64
    lps = [make(r, oracle) for r, make, _ in kept]
    refs = solve_and_check(sens, lps, oracle, [label(r) for r, _, label in kept])
    for (r, _, _), ref in zip(kept, refs):  # (the oracle's answers are the records')
        assert (ref["status"], ref["n_pivots"], G.sha256(ref["matrix"])) == (r["status"], r["n_pivots"], r["final_sha256"])
    optimal = [NS.restate(ref["matrix"], lp[0], lp[1], lp[5]) for lp, ref in zip(lps, refs) if ref["status"] == "optimal"]
    assert len(optimal) == 97
    # what the records bring: infinite ranges on both kinds of array, and signed zeros among the quotients
    assert any(np.isinf(a).any() for rng in optimal for a in rng[1:3]) and any(np.isinf(a).any() for rng in optimal for a in rng[3:])
    assert any((a[1:] == 0).any() for rng in optimal for a in rng[1:])


def small_lps(oracle, count, check=False):
    """Alternating shapes of one class and alternating endings: optimal, stopped by its budget, infeasible."""
    out = []
    for i in range(count):
        M, N = ((12, 9), (7, 14))[i % 2]
        lp = B.dense_lp(oracle, M, N, 1 + i, check_cycles=check)
        if i % 3 == 1:
            lp = BS.with_options(lp, 1.0, check)
        elif i % 3 == 2:
            w, h, row, col, val = lp[:5]
            val = val.copy()
            val[(row == 1) & (col > 0)] = np.abs(val[(row == 1) & (col > 0)])  # a row of positive coefficients ...
            val[(row == 1) & (col == 0)] = -1.0                                # ... below a negative right-hand side
            lp = (w, h, row, col, val, *lp[5:])
        out.append(lp)
    return out


@pytest.mark.gpu
def test_queue_hands_out_more_lps_than_workgroups(sens, oracle):
    lps = small_lps(oracle, 4500)
    refs = solve_and_check(sens, lps, oracle)
    info = sens.info()
    assert info["launches"] == 1 and info["kernels"][0]["lps"] == 4500 > info["kernels"][0]["grid"]
    assert {r["status"] for r in refs} >= {"optimal", "infeasible", "cycled"}
    # no range of one LP shows a neighbour's: the same LPs in another order give every LP its own ranges again
    order = list(np.random.default_rng(11).permutation(len(lps)))
    solve_and_check(sens, [lps[j] for j in order], oracle, refs=[refs[j] for j in order])
    statuses, results, pivots, _ = sens.solve([])
    assert statuses == [] and results.size == 0 and pivots.size == 0 and sens.info()["launches"] == 0


@pytest.mark.gpu
def test_history_rerun_recomputes_the_ranges(gpu, oracle, monkeypatch):
    lps = [B.dense_lp(oracle, 96, 80, 9, check_cycles=True), B.dense_lp(oracle, 300, 279, 5, check_cycles=True),
           B.dense_lp(oracle, 30, 30, 2, check_cycles=False), B.dense_lp(oracle, 30, 29, 2, check_cycles=True)]
    uncapped = gpu.LpSens(0)
    monkeypatch.setenv("YALPS_LPSENS_HIST", "8")
    monkeypatch.setenv("YALPS_LPBATCH_HIST", "1")  # (the LP batch's switch is not this library's)
    capped = gpu.LpSens(0)
    try:
        refs = solve_and_check(uncapped, lps, oracle)
        assert uncapped.info()["reruns"] == 0
        solve_and_check(capped, lps, oracle, refs=refs)
        info = capped.info()
        assert {0, 1} <= set(info["rerun_lps"]) and 2 not in info["rerun_lps"]
        later = [k for k in info["kernels"] if k["pass"] > 0]
        assert later and all("check" in k["kernel"] and k["hist_cap"] == 8 * 4 ** k["pass"] for k in later)
        for i in range(len(lps)):
            NS.check_ranges(capped.ranges(i), uncapped.ranges(i), i)
    finally:
        uncapped.close()
        capped.close()


@pytest.mark.gpu
def test_handle_reuse_grows_and_shrinks(gpu, oracle):
    s = gpu.LpSens(0)
    try:
        first = small_lps(oracle, 40)
        second = small_lps(oracle, 300)[::-1] + [B.dense_lp(oracle, 300, 280, 5), B.dense_lp(oracle, 130, 120, 6)]
        third = [B.dense_lp(oracle, 60, 50, 8), B.dense_lp(oracle, 300, 280, 7, max_pivots=40)]
        for lps in (first, second, third, first[:3]):
            solve_and_check(s, lps, oracle)
            with pytest.raises(gpu.NativeError, match="no such LP"):
                s.ranges(len(lps))
        s.solve(third)
        s.ranges(0)  # (the ranges need no kept tableaux)
        with pytest.raises(gpu.NativeError, match="keep_tableaux"):
            s.tableau(0)
        with pytest.raises(gpu.NativeError, match="LP 1: .*above the batch limit"):
            s.solve([third[0], (1024, 513, *third[0][2:])])
        with pytest.raises(gpu.NativeError, match="no such LP"):
            s.ranges(0)
    finally:
        s.close()


def same_sensitivity(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a == b  # (tuples and dicts of floats: no NaN in a range)


@pytest.mark.gpu
def test_large_lp_route(gpu, oracle):
    """dense-LP(1023, 512): 1024 x 513 doubles, 4 MiB + 8 KiB (two rows above the limit), as a model: through DeviceTableau and the host ranging."""
    from yalps_amd import sensitivity as SE
    from yalps_amd import solve as S
    M, N = 1023, 512
    m = oracle.dense_lp(M, N, 3).reshape(M + 1, N + 1)
    assert 8 * m.size > B.MAX_BYTES >= 8 * (m.size - 2 * (N + 1))
    model = {"direction": "maximize", "objective": "obj",
             "constraints": {"r%d" % r: {"max": float(m[r, 0])} for r in range(1, M + 1)},
             "variables": {"x%d" % c: dict({"obj": float(m[0, c])}, **{"r%d" % r: float(m[r, c]) for r in range(1, M + 1)})
                           for c in range(1, N + 1)}}
    routed = []
    real = SE.device_tableau_sensitivity
    try:  # (sensitivity() has no stats: count what reaches the large backend)
        SE.device_tableau_sensitivity = lambda t, o: routed.append((t.width, t.height)) or real(t, o)
        got = SE._sensitivity_many_with(SE.lpsens_simplex, SE.device_tableau_sensitivity, [model])[0]
    finally:
        SE.device_tableau_sensitivity = real
    want = NS.oracle_sensitivity(oracle, [model])[0]
    assert routed == [(N + 1, M + 1)]
    assert got["status"] == want["status"] == "optimal" and got["result"] == want["result"] and got["variables"] == want["variables"]
    assert same_sensitivity(got["sensitivity"], want["sensitivity"])


@pytest.mark.gpu
def test_sensitivity_many_on_every_golden_lp_case(gpu, oracle):
    from yalps_amd import solve as S
    from tests.test_lp_batch import same_solution
    cases = [K.load(n) for n in K.names()]
    cases = [c for c in cases if not c["model"].get("integers") and not c["model"].get("binaries")]
    assert len(cases) >= 20
    models, options = [c["model"] for c in cases], [c["options"] for c in cases]
    stats = {}
    got = S.sensitivity_many(models, options, stats)
    want = NS.oracle_sensitivity(oracle, models, options)
    assert stats["batched"] + stats["large"] == len(cases) and stats["launches"] >= 1
    assert all(k["kernel"] in KERNELS for k in stats["kernels"])
    for c, g, e in zip(cases, got, want):
        assert same_solution(g, S.solve(c["model"], c["options"])), c["name"]
        assert same_solution(g, e) and same_sensitivity(g["sensitivity"], e["sensitivity"]), c["name"]
    assert sum(1 for g in got if g["sensitivity"] is not None) >= 15
    k = next(i for i, g in enumerate(got) if g["sensitivity"] is not None)
    assert copy.deepcopy(got[k]) == S.sensitivity(models[k], options[k])
