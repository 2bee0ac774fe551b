"""Variants of one LP reoptimised from the base's optimal tableau (include/yalps_lpwarm.h, yalps_amd.solve.reoptimize_variants).

On the CPU: the warm tableau's formulas (tests/_np_warm.py) against exact pivoting, the routing and the marshalling with the C
oracle as backend on the golden models -- 24 seeded variants of each of the 23 LPs whose base ends optimal, every answer under
the reference's validator against the cold answer; the single-bound moves inside the sensitivity ranges, which must take no
pivot; the eight bases that do not end optimal -- libyalps_lpwarm.so's boundary and its kernels by name.

On the GPU every comparison is bit for bit (tests/_lp_batch.py::check_lp) against the oracle started from _np_warm's tableau
with the base's permutations: status, result, pivots, column 0, both permutations and the kept matrix.  The fill alone runs
with maxPivots = 0, where the kept matrix is the warm tableau itself."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _batch_shapes as BS
from tests import _cases as K
from tests import _lp_batch as LB
from tests import _lp_variants as V
from tests import _np_warm as NW
from tests import _variant_shapes as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpwarm()
    return _native


@pytest.fixture(scope="module")
def golden(oracle):
    good, bad = NW.golden_lp_cases(oracle)
    assert (len(good), len(bad)) == (NW.GOLDEN_LPS, NW.NON_OPTIMAL)
    return good, bad


# ---------------------------------------------------------------------------------------------------------- CPU

EXACT_MODELS = ("Berlin Air Lift Problem", "Chocolate Problem", "Coffee Problem", "Computer Problem", "Wiki 1")


def test_warm_tableau_is_the_pivoted_variant_in_exact_arithmetic(oracle):
    """W(F, patch) == the variant's initial tableau pivoted along the base's pivot sequence, in Fractions: the formulas, their
    signs and their order, not a restatement of them."""
    from fractions import Fraction
    from yalps_amd.model import tableau_model_with_bounds, variant_patch_cells
    checked, kinds = 0, set()
    for name in EXACT_MODELS:
        case = K.load(name)
        tabmod, info = tableau_model_with_bounds(case["model"], sparse=True)
        t = tabmod.tableau
        w, h = t.width, t.height
        o = case["options"]
        base = NW.solve_base(oracle, t.cells, w, h, o["precision"], o["maxPivots"], o["checkCycles"], trace_cap=4096)
        assert base["status"] == "optimal" and 0 < base["n_pivots"] == len(base["trace"]), name
        initial = NW.dense_of(t.cells, w, h)
        F, pos, var = NW.exact_along(initial, w, h, base["trace"])
        assert np.array_equal(pos, base["pos"]) and np.array_equal(var, base["var"]), name
        b0 = NW.edge_cells(t.cells, w)
        for variant in NW.golden_variants(case["model"]):
            patch = variant_patch_cells(tabmod, info, variant)
            assert patch is not None and all(k < w or k % w == 0 for k, _ in patch), (name, variant)
            moved = initial.copy()
            for k, v in patch:
                moved[k] = v
            want, _, _ = NW.exact_along(moved, w, h, base["trace"])
            got = NW.warm_tableau(F, pos, b0, patch, number=lambda x: Fraction(float(x)))
            assert np.array_equal(got, want), (name, variant)
            for k, v in patch:
                if v != b0.get(k, 0.0):
                    p = int(pos[w + k // w] if k % w == 0 else pos[k])
                    kinds.add(("column 0" if k % w == 0 else "row 0", "non-basic" if p < w else "basic"))
            checked += 1
    assert checked == len(EXACT_MODELS) * NW.N_VARIANTS
    assert kinds == {(line, where) for line in ("column 0", "row 0") for where in ("basic", "non-basic")}


def test_the_552_golden_variants_are_valid_answers_and_cheaper(oracle, golden):
    from tests.test_lp_batch import oracle_backend
    from yalps_amd import solve as S
    from yalps_amd.model import apply_variant, tableau_model
    warm, cold = NW.oracle_warm_backend(oracle), NW.oracle_cold(oracle)
    one = oracle_backend(oracle)
    total = identical = warm_pivots = cold_pivots = 0
    for case in golden[0]:
        model, options = case["model"], case["options"]
        variants = NW.golden_variants(model)
        stats = {}
        got = S._reoptimize_variants_with(warm, cold, model, variants, options, options, stats)
        assert (stats["warm"], stats["cold"], stats["base_status"]) == (NW.N_VARIANTS, 0, "optimal"), case["name"]
        assert len(stats["pivots"]) == NW.N_VARIANTS and "solve_variants" not in stats
        expected = cold(model, variants, options, None)
        for v, g, e in zip(variants, got, expected):
            full = apply_variant(model, v)
            assert K.valid_solution_and_status(g, e, full, options), (case["name"], v, g["status"], g["result"], e["status"], e["result"])
            assert repr(S._solve_with(one, full, options)) == repr(e)  # (the cold answer is solve()'s for the variant's full model)
            identical += repr(g) == repr(e)
            cold_pivots += LB.oracle_answer(oracle, LB.model_lp(tableau_model(full, sparse=True), options))["n_pivots"]
        total += len(variants)
        warm_pivots += sum(stats["pivots"])
    assert total == 552 and identical >= 500
    assert warm_pivots < cold_pivots, (warm_pivots, cold_pivots)


def test_moves_inside_the_sensitivity_ranges_take_no_pivot(oracle, golden):
    from tests import _np_sensitivity as NS
    from yalps_amd import solve as S
    warm, cold = NW.oracle_warm_backend(oracle), NW.oracle_cold(oracle)
    moves = 0
    for case in golden[0]:
        model, options = case["model"], case["options"]
        answer = NS.oracle_sensitivity(oracle, [model], [options])[0]
        todo = NW.midpoint_moves(model, answer["sensitivity"])
        stats = {}
        got = S._reoptimize_variants_with(warm, cold, model, [m for m, _ in todo], options, options, stats)
        assert stats["warm"] == len(todo) and stats["cold"] == 0, case["name"]
        for (_, label), g, pivots in zip(todo, got, stats["pivots"]):
            assert (pivots, g["status"]) == (0, "optimal"), (case["name"], label, pivots, g["status"])
        moves += len(todo)
    assert moves == 1371


def test_a_base_that_is_not_optimal_is_solve_variants(oracle, golden):
    from yalps_amd import solve as S
    warm, cold = NW.oracle_warm_backend(oracle), NW.oracle_cold(oracle)
    statuses = set()
    for case in golden[1]:
        model, options = case["model"], case["options"]
        variants = [{}] + NW.golden_variants(model)[:5]
        stats = {}
        got = S._reoptimize_variants_with(warm, cold, model, variants, options, options, stats)
        expected = cold(model, variants, options, None)
        assert repr(got) == repr(expected), case["name"]
        assert (stats["warm"], stats["cold"]) == (0, len(variants)) and stats["base_status"] != "optimal", (case["name"], stats)
        assert stats["pivots"] == [] and "solve_variants" in stats
        statuses.add(stats["base_status"])
    assert statuses == {"infeasible", "unbounded", "cycled"}


def recording(calls, answer="cold"):
    def cold(model, variants, options, stats):
        calls.append((len(variants), options))
        return [answer] * len(variants)
    return cold


def refusing(*_):
    raise AssertionError("the warm backend was called")


def test_routing(oracle):
    from yalps_amd import solve as S
    model = V.dense_model(oracle, 12, 10, 4)
    warm_log = []
    warm = NW.oracle_warm_backend(oracle, warm_log)
    plain = {"constraints": {"c2": {"max": 3.5}}, "variables": {"x3": {"obj": 0.25}}}
    body = {"constraints": {"c2": {"max": 3.5}}, "variables": {"x3": {"c4": 0.25}}}
    structure = {"constraints": {"c3": {"equal": 2.0}}}
    infinite = {"variables": {"x1": {"obj": INF}}}
    # a body cell, another structure and a delta that is not finite go cold, in one call, the rest warm; the order is kept
    calls, stats = [], {}
    variants = [plain, body, {}, structure, infinite, plain]
    options = [{"maxPivots": 100 + i} for i in range(len(variants))]
    got = S._reoptimize_variants_with(warm, recording(calls), model, variants, options, None, stats)
    assert [g == "cold" for g in got] == [False, True, False, True, True, False]
    assert calls == [(3, [options[1], options[3], options[4]])]
    assert (stats["warm"], stats["cold"], stats["base_status"]) == (3, 3, "optimal") and len(stats["pivots"]) == 3
    assert [o["maxPivots"] for o in warm_log[0][1]] == [100, 102, 105]
    assert got[0] == got[5] and got[0]["status"] == "optimal"
    # cells whose value is the base's are dropped before the backend sees them
    same = {"constraints": {"c2": {"max": model["constraints"]["c2"]["max"]}}, "variables": {"x3": {"obj": model["variables"]["x3"]["obj"]}}}
    del warm_log[:]
    got = S._reoptimize_variants_with(warm, refusing, model, [same, plain], None, None, stats)
    assert [len(p) for p in warm_log[0][0]] == [0, 2] and stats["pivots"][0] == 0
    # a base with integers and a base above 4 MiB: the whole call, with the same arguments
    integer = dict(model, integers=["x1"])
    n = 730
    large = {"direction": "maximize", "objective": "obj", "constraints": {"c%d" % r: {"max": 1.0} for r in range(n)},
             "variables": {"x%d" % r: {"obj": 1.0, "c%d" % r: 1.0} for r in range(n)}}
    assert 8 * (n + 1) * (n + 1) > 4 << 20
    for m in (integer, large):
        calls, stats = [], {}
        opts = [{"precision": 1e-6}, None]
        got = S._reoptimize_variants_with(refusing, recording(calls), m, [plain, {}], opts, None, stats)
        assert got == ["cold", "cold"] and calls == [(2, opts)] and (stats["warm"], stats["cold"]) == (0, 2)
    # only cold variants: the base is not solved at all
    calls = []
    assert S._reoptimize_variants_with(refusing, recording(calls), model, [body, structure], None) == ["cold", "cold"]
    # option counts
    with pytest.raises(ValueError):
        S._reoptimize_variants_with(warm, recording([]), model, [plain, plain, plain], [{}, {}])
    assert S._reoptimize_variants_with(refusing, recording([]), model, []) == []
    # base_options are the base's alone: a base cut short is not optimal, and the call goes cold
    calls, stats = [], {}
    got = S._reoptimize_variants_with(warm, recording(calls), model, [plain], None, {"maxPivots": 1}, stats)
    assert got == ["cold"] and stats["base_status"] == "cycled" and stats["base_pivots"] == 1


def test_header_symbols_are_exported(nat):
    text = open(os.path.join(ROOT, "include", "yalps_lpwarm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text))
    assert declared and all(s.startswith("yalps_lpwarm_") for s in declared), declared
    L = nat.lpwarm_lib()
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert declared == set(nat.SYMBOLS_LPWARM)


def test_kernels_are_the_table(nat):
    from yalps_amd import build
    ks = build.kernel_metadata(lib=build.LIB_LPWARM)
    spelt = {NW.spelling(s): md for s, md in ks.items()}
    warm = {NW.kernel_of(cls, check) for cls in range(5) for check in (False, True)}
    assert len(warm) == 6 and len(spelt) == len(ks)
    assert set(spelt) == warm | {NW.IMAGE_KERNEL} | {k.replace("lp_warm_kernel", "lp_batch_kernel") for k in warm}, sorted(spelt)
    for name, md in spelt.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0, (name, md)
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (name, md["group_segment_fixed_size"])


def _i32(*a):
    return np.array(a, np.int32)


REFUSALS = {  # name: (width, height, base (row, col), patch offsets, patch (row, col), count, text)
    "width below 1": (0, 3, ((), ()), (0, 0), ((), ()), 1, "width and height"),
    "above the limit": (1024, 1024, ((), ()), (0, 0), ((), ()), 1, "above the limit"),
    "base cell outside": (4, 3, ((0, 3), (1, 0)), (0, 0), ((), ()), 1, "base cell 1 lies outside"),
    "base cells unsorted": (4, 3, ((1, 0), (0, 1)), (0, 0), ((), ()), 1, "base cells are not sorted"),
    "negative count": (4, 3, ((), ()), (0,), ((), ()), -1, "count < 0"),
    "negative offset": (4, 3, ((), ()), (-1, 0), ((), ()), 1, "variant 0: negative patch offset"),
    "offsets decrease": (4, 3, ((), ()), (0, 1, 0), ((0,), (1,)), 2, "variant 1: patch offsets decrease"),
    "patch cell outside": (4, 3, ((), ()), (0, 1, 2), ((0, 3), (1, 0)), 2, "variant 1: patch cell 0 lies outside"),
    "patch cells unsorted": (4, 3, ((), ()), (0, 0, 2), ((1, 0), (0, 1)), 2, "variant 1: patch cells are not sorted"),
    "body cell": (4, 3, ((), ()), (0, 1, 1, 3), ((0, 0, 1), (1, 2, 2)), 3, "variant 2: patch cell 1 lies in the body"),
    "cell (0, 0)": (4, 3, ((), ()), (0, 1, 3), ((1, 0, 0), (0, 0, 1)), 2, "variant 1: patch cell 0 is the cell (0, 0)"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_validate_refuses(nat, name):
    w, h, base, off, patch, count, text = REFUSALS[name]
    brow, bcol, prow, pcol = _i32(*base[0]), _i32(*base[1]), _i32(*patch[0]), _i32(*patch[1])
    off = np.array(off, np.int64)
    L = nat.lpwarm_lib()
    rc = L.yalps_lpwarm_validate(w, h, brow.size, brow.ctypes.data, bcol.ctypes.data, count, off.ctypes.data, prow.ctypes.data,
                                 pcol.ctypes.data)
    assert rc == -1 and text in L.yalps_lpwarm_last_error().decode(), (rc, L.yalps_lpwarm_last_error())


def test_validate_accepts_what_a_warm_patch_is(nat):
    brow, bcol = _i32(0, 1, 2), _i32(1, 0, 3)
    prow, pcol, off = _i32(0, 0, 1, 2, 2), _i32(1, 3, 0, 0, 0), np.array([0, 4, 4, 5], np.int64)
    L = nat.lpwarm_lib()
    assert L.yalps_lpwarm_validate(4, 3, 3, brow.ctypes.data, bcol.ctypes.data, 3, off.ctypes.data, prow.ctypes.data, pcol.ctypes.data) == 0
    assert L.yalps_lpwarm_validate(4, 3, 0, None, None, 0, None, None, None) == 0


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def lw(nat):
    handle = nat.LpWarm(0)
    yield handle
    handle.close()


_BASES = {}


def base_of(oracle, w, h, seed=5):
    """(LP tuple, the oracle's solve, b0) of dense-LP(h - 1, w - 1, seed); shared among the tests and left unchanged."""
    key = (w, h, seed)
    if key not in _BASES:
        lp = LB.dense_lp(oracle, h - 1, w - 1, seed)
        base = NW.solve_base(oracle, lp[2:5], w, h, max_pivots=INF)
        assert base["status"] == "optimal", key
        _BASES[key] = (lp, base, NW.edge_cells(lp[2:5], w))
    return _BASES[key]


def fill_patches(base, b0, w, h):
    """{kind: patch} of the records the fill has to get right on this base; a kind the base's basis does not offer is absent."""
    F, pos = base["matrix"].reshape(h, w), base["pos"]
    cell = lambda k, d: (k, b0.get(k, 0.0) + d)
    slack_nb = [r for r in range(1, h) if pos[w + r] < w]
    slack_b = [r for r in range(1, h) if pos[w + r] >= w]
    var_nb = [c for c in range(1, w) if pos[c] < w]
    var_b = [c for c in range(1, w) if pos[c] >= w]
    out = {"none": []}
    if slack_nb:
        out["column 0, non-basic slack"] = [cell(slack_nb[-1] * w, 0.375)]
    if slack_b:
        out["column 0, basic slack"] = [cell(slack_b[0] * w, 0.625)]
        r = slack_b[-1]
        out["right-hand side below zero"] = [cell(r * w, -(F[pos[w + r] - w, 0] + 1.5))]
    if var_nb:
        out["row 0, non-basic variable"] = [cell(var_nb[0], -0.25)]
    if var_b:
        out["row 0, basic variable"] = [cell(var_b[-1], 0.5)]
    for c in var_b:  # a row 0 record reads, in its basic row, what a column 0 record wrote there
        R = pos[c] - w
        hit = [r for r in slack_nb if F[R, pos[w + r]] * 0.75 + F[R, 0] != F[R, 0]]
        if hit:
            out["column 0 and row 0 meet"] = [cell(c, 0.5), cell(hit[0] * w, 0.75)]
            break
    out["every bound and every coefficient"] = ([cell(c, 0.01 * (c % 7 - 3) + 0.005) for c in range(1, w)] +
                                                [cell(r * w, 0.02 * (r % 5 - 1) + 0.01) for r in range(1, h)])
    return out


def run_fill(nat, lw, oracle, shapes, need=()):
    kinds = set()
    for w, h in shapes:
        lp, base, b0 = base_of(oracle, w, h)
        patches = fill_patches(base, b0, w, h)
        names = list(patches)
        out = lw.solve(NW.packed_cells(nat, lp, [patches[k] for k in names], [(1e-8, 0.0, False)] * len(names),
                                       base_options=(1e-8, INF, False)), keep_tableaux=True)
        assert out is not None and lw.base[0] == "optimal" and lw.base[2] == base["n_pivots"], (w, h, lw.base)
        info = lw.info()
        cls = LB.size_class(w, h)
        assert [k["kernel"] for k in info["kernels"]] == [NW.kernel_of(cls, False)] and info["kernels"][0]["class"] == cls, info["text"]
        assert info["kernels"][0]["aux"] == int(cls == 4 and BS.aux_hbm(w, h))
        for i, name in enumerate(names):
            ref = NW.warm_answer(oracle, base, w, h, b0, patches[name], max_pivots=0.0)
            assert ref["n_pivots"] == 0 and LB.same_words(ref["matrix"], ref["start"].reshape(-1)), (w, h, name)
            if name == "right-hand side below zero":
                assert ref["start"][1:, 0].min() < -1.0
            if name != "none":
                assert not LB.same_words(ref["matrix"], base["matrix"]), (w, h, name)
            LB.check_lp(lw, i, out, ref, lp, label="%s, fill" % name)
        kinds |= set(names)
    assert kinds >= set(need), set(need) - kinds
    return kinds


ALL_KINDS = ("none", "column 0, non-basic slack", "column 0, basic slack", "right-hand side below zero", "row 0, non-basic variable",
             "row 0, basic variable", "column 0 and row 0 meet", "every bound and every coefficient")
CLASS_SHAPES = ((31, 31), (8, 300), (80, 97), (121, 131), (281, 301))  # (w, h) of the classes 0 .. 4


@pytest.mark.gpu
def test_fill_at_every_parity(nat, lw, oracle):
    run_fill(nat, lw, oracle, ((4, 6), (4, 7), (5, 6), (7, 5)), need=ALL_KINDS)


@pytest.mark.gpu
def test_fill_in_every_size_class(nat, lw, oracle):
    assert [LB.size_class(w, h) for w, h in CLASS_SHAPES] == [0, 1, 2, 3, 4]
    w, h = CLASS_SHAPES[1]
    assert (w - 1) + (h - 1) > NW.KERNEL_LANES[1] and h - 1 > NW.KERNEL_LANES[1]  # (more records than the workgroup has lanes)
    run_fill(nat, lw, oracle, CLASS_SHAPES, need=ALL_KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(BS.BOUND_WIDTHS))
def test_fill_on_both_sides_of_a_class_bound(nat, lw, oracle, k):
    w = BS.BOUND_WIDTHS[k]
    h = BS.rows_under(LB.BOUNDS[k], w)
    assert (LB.size_class(w, h), LB.size_class(w, h + 1)) == (k, k + 1)
    run_fill(nat, lw, oracle, ((w, h), (w, h + 1)), need=ALL_KINDS)


@pytest.mark.gpu
def test_fill_in_the_aux_form(nat, lw, oracle):
    w, h = 8152, 41
    assert BS.pcols(w) + h == 8193 and BS.aux_hbm(w, h) and (w - 1) + (h - 1) > 1024
    run_fill(nat, lw, oracle, ((w, h),), need=ALL_KINDS)


def ending_base(oracle):
    """A 31 x 30 base for whole reoptimisations: dense-LP(30, 29, 3) with row 5 negated (a floor under a sum, which a lower
    right-hand side raises: phase 1 runs and can end feasible) and with one column that no row bounds and the objective does
    not want (a variant that wants it is unbounded)."""
    key = "endings"
    if key not in _BASES:
        w, h = 30, 31
        A = LB.scatter(LB.dense_lp(oracle, h - 1, w - 1, 3)).reshape(h, w).copy()
        A[5, 1:] = -A[5, 1:]
        A[1:, 7] = 0.0
        A[0, 7] = -1.0
        lp = LB.from_dense(A.ravel(), w, h)
        base = NW.solve_base(oracle, lp[2:5], w, h, max_pivots=INF)
        assert base["status"] == "optimal"
        _BASES[key] = (lp, base, NW.edge_cells(lp[2:5], w))
    return _BASES[key]


def ending_variants(oracle):
    """[(label, patch, (precision, maxPivots, checkCycles))] and their answers: every ending of a reoptimisation."""
    lp, base, b0 = ending_base(oracle)
    w, h = lp[:2]
    F, pos = base["matrix"].reshape(h, w), base["pos"]
    cell = lambda k, d: (k, b0.get(k, 0.0) + d)
    slack_b = [r for r in range(1, h) if pos[w + r] >= w]
    slack_nb = [r for r in range(1, h) if pos[w + r] < w]
    assert len(slack_b) >= 2 and len(slack_nb) >= 3 and 5 in slack_b
    floor = [cell(5 * w, -(F[pos[w + 5] - w, 0] + 0.05))]  # the floor of row 5 just above what the base's optimum gives
    phase1 = [(r * w, -0.5 - 0.01 * r) for r in slack_nb[:3]]
    phase2 = [cell(c, (-1.0) ** c * 0.5 * b0.get(c, 0.0)) for c in range(1, w) if c != 7]
    rows = [
        ("no pivot", [cell(slack_b[0] * w, 0.25)], (1e-8, 8192.0, False)),
        ("through phase 1", floor, (1e-8, INF, False)),
        ("infeasible", [(slack_nb[0] * w, -1.0)] + [cell(r * w, 0.125) for r in slack_b[:1]], (1e-8, 8192.0, True)),
        ("unbounded", [(7, 1.0)], (1e-6, 8192.0, False)),
        ("budget inside phase 1", phase1, (1e-8, 1.0, False)),
        ("phase 2", phase2, (1e-6, INF, True)),
        ("budget inside phase 2", phase2, (1e-8, 2.0, False)),
    ]
    rows = [(label, sorted(patch), opt) for label, patch, opt in rows]  # (the order the ABI asks for)
    refs = [NW.warm_answer(oracle, base, w, h, b0, patch, *opt) for _, patch, opt in rows]
    return lp, base, rows, refs


@pytest.mark.gpu
def test_every_ending_with_mixed_options_in_one_call(nat, lw, oracle):
    lp, base, rows, refs = ending_variants(oracle)
    w, h = lp[:2]
    by = {label: ref for (label, _, _), ref in zip(rows, refs)}
    # (what the rows are there for, on the reference's side)
    assert (by["no pivot"]["status"], by["no pivot"]["n_pivots"]) == ("optimal", 0)
    assert by["through phase 1"]["status"] == "optimal" and by["through phase 1"]["n_pivots"] >= 1
    assert by["through phase 1"]["start"][1:, 0].min() < -0.04
    assert by["infeasible"]["status"] == "infeasible" and by["unbounded"]["status"] == "unbounded"
    cut1, cut2 = by["budget inside phase 1"], by["budget inside phase 2"]
    assert (cut1["status"], cut1["n_pivots"]) == ("cycled", 1) and cut1["matrix"][w::w].min() < -1e-8      # a row is still infeasible
    assert (cut2["status"], cut2["n_pivots"]) == ("cycled", 2) and cut2["matrix"][w::w].min() >= -1e-8     # none was, row 0 is not done
    assert by["phase 2"]["status"] == "optimal" and by["phase 2"]["n_pivots"] > 2
    out = lw.solve(NW.packed_cells(nat, lp, [p for _, p, _ in rows], [o for _, _, o in rows], base_options=(1e-8, INF, False)),
                   keep_tableaux=True)
    assert {k["kernel"] for k in lw.info()["kernels"]} == {NW.kernel_of(0, False), NW.kernel_of(0, True)}
    for i, ((label, _, _), ref) in enumerate(zip(rows, refs)):
        LB.check_lp(lw, i, out, ref, lp, label=label)


@pytest.mark.gpu
def test_history_rerun(nat, oracle, monkeypatch):
    lp, base, rows, refs = ending_variants(oracle)
    i = [label for label, _, _ in rows].index("phase 2")
    assert refs[i]["n_pivots"] > 2 * 2
    monkeypatch.setenv("YALPS_LPWARM_HIST", "2")
    handle = nat.LpWarm(0)
    try:
        out = handle.solve(NW.packed_cells(nat, lp, [p for _, p, _ in rows], [o for _, _, o in rows], base_options=(1e-8, INF, False)),
                           keep_tableaux=True)
        info = handle.info()
        assert info["reruns"] >= 1 and i in info["rerun_lps"] and info["launches"] >= 3, info["text"]
        assert all(k["kernel"] == NW.kernel_of(0, True) and k["hist_cap"] == 2 * 4 ** k["pass"] for k in info["kernels"] if k["pass"] > 0)
        for j, ((label, _, _), ref) in enumerate(zip(rows, refs)):
            LB.check_lp(handle, j, out, ref, lp, label=label)
    finally:
        handle.close()


@pytest.mark.gpu
def test_more_variants_than_workgroups_in_the_hbm_form(nat, oracle, monkeypatch):
    w, h = CLASS_SHAPES[4]
    lp, base, b0 = base_of(oracle, w, h)
    rng = np.random.default_rng(11)
    patches = []
    for i in range(7):  # bounds and coefficients moved by up to +-50 %, a few per variant; every second one with checkCycles
        cols, rows = rng.choice(np.arange(1, w), 3, replace=False), rng.choice(np.arange(1, h), 3, replace=False)
        patches.append(sorted([(int(c), b0.get(int(c), 0.0) * (1.0 + rng.uniform(-0.5, 0.5))) for c in cols] +
                              [(int(r) * w, b0.get(int(r) * w, 0.0) * (1.0 + rng.uniform(-0.5, 0.5))) for r in rows]))
    options = [(1e-8, 8192.0, bool(i % 2)) for i in range(7)]
    monkeypatch.setenv("YALPS_LPWARM_CUS", "2")
    monkeypatch.setenv("YALPS_LPWARM_PER_CU", "1")
    handle = nat.LpWarm(0)
    try:
        out = handle.solve(NW.packed_cells(nat, lp, patches, options, base_options=(1e-8, INF, False)), keep_tableaux=True)
        info = handle.info()
        first = sorted((k["kernel"], k["grid"], k["lps"]) for k in info["kernels"] if k["pass"] == 0)  # (a long variant may run again)
        assert first == sorted([(NW.kernel_of(4, False), 2, 4), (NW.kernel_of(4, True), 2, 3)]), info["text"]
        pivots = 0
        for i, (patch, o) in enumerate(zip(patches, options)):
            ref = NW.warm_answer(oracle, base, w, h, b0, patch, *o)
            pivots += ref["n_pivots"]
            LB.check_lp(handle, i, out, ref, lp, label="variant")
        assert pivots > 0
    finally:
        handle.close()


@pytest.mark.gpu
def test_a_handle_takes_another_shape(nat, oracle):
    handle = nat.LpWarm(0)
    try:
        for w, h in ((31, 31), (121, 131), (5, 6), (31, 31)):
            lp, base, b0 = base_of(oracle, w, h)
            patches = fill_patches(base, b0, w, h)
            names = [k for k in patches if k != "none"][:4]
            out = handle.solve(NW.packed_cells(nat, lp, [patches[k] for k in names], base_options=(1e-8, INF, False)), keep_tableaux=True)
            for i, name in enumerate(names):
                LB.check_lp(handle, i, out, NW.warm_answer(oracle, base, w, h, b0, patches[name]), lp, label=name)
        # a base that does not end optimal: its status, nothing for the variants, and the handle goes on
        lp, base, b0 = base_of(oracle, 31, 31)
        assert handle.solve(NW.packed_cells(nat, lp, [[]], base_options=(1e-8, 1.0, False))) is None
        assert handle.base[0] == "cycled" and handle.base[2] == 1 and handle.info()["launches"] == 0
        with pytest.raises(nat.NativeError):
            handle.solution(0)
        assert handle.solve(NW.packed_cells(nat, lp, [[]], base_options=(1e-8, INF, False))) is not None
    finally:
        handle.close()


@pytest.mark.gpu
def test_caller_stream(nat, lw, oracle, tmp_path):
    lp, base, rows, refs = ending_variants(oracle)
    path = str(tmp_path / "stream.npz")
    child = subprocess.run([sys.executable, "-m", "tests._np_warm", path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    got = np.load(path)
    out = lw.solve(NW.packed_cells(nat, lp, [p for _, p, _ in rows], [o for _, _, o in rows], base_options=(1e-8, INF, False)),
                   keep_tableaux=True)
    mine = VS.outputs(lw, out, len(rows))
    for key, value in mine.items():
        a, b = np.asarray(value), got[key]
        same = np.array_equal(a, b) if a.dtype.kind != "f" else LB.same_words(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0))
        assert same, key
    for j, ((label, _, _), ref) in enumerate(zip(rows, refs)):
        LB.check_lp(lw, j, out, ref, lp, label=label)


GOLDEN_GROUPS = {"Monster Problem": lambda n: n == "Monster Problem", "the others": lambda n: n != "Monster Problem"}


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GOLDEN_GROUPS))
def test_reoptimize_variants_on_the_golden_models(nat, golden, group):
    from yalps_amd import solve as S
    from yalps_amd.model import apply_variant
    cases = [c for c in golden[0] if GOLDEN_GROUPS[group](c["name"])]
    assert len(cases) == (1 if group == "Monster Problem" else NW.GOLDEN_LPS - 1)
    for case in cases:
        model, options = case["model"], case["options"]
        variants = NW.golden_variants(model)
        stats = {}
        got = S.reoptimize_variants(model, variants, options, options, stats)
        expected = S.solve_variants(model, variants, options)
        assert (stats["warm"], stats["cold"], stats["base_status"], stats["launches"]) == (NW.N_VARIANTS, 0, "optimal", 1), (case["name"], stats)
        assert all(k["kernel"].startswith("lp_warm_kernel<") for k in stats["kernels"])
        for v, g, e in zip(variants, got, expected):
            assert K.valid_solution_and_status(g, e, apply_variant(model, v), options), (case["name"], v, g["status"], g["result"], e["result"])


@pytest.mark.gpu
def test_reoptimize_variants_with_a_base_that_is_not_optimal(nat, golden):
    from yalps_amd import solve as S
    for case in golden[1]:
        model, options = case["model"], case["options"]
        variants = [{}] + NW.golden_variants(model)[:5]
        stats = {}
        got = S.reoptimize_variants(model, variants, options, options, stats)
        assert repr(got) == repr(S.solve_variants(model, variants, options)), case["name"]
        assert (stats["warm"], stats["cold"]) == (0, len(variants)) and stats["base_status"] != "optimal", (case["name"], stats)
