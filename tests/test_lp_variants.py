"""Many variants of one LP (include/yalps_lpvar.h, yalps_amd.solve.solve_variants): apply_variant and variant_patch against
tableau_model on the CPU, the routing with the oracle as backend, libyalps_lpvar.so's boundary and its kernels by name; on the
GPU every kernel instantiation, degenerate shapes, the work queue, mixed endings, the checkCycles history rerun, handle reuse
and solve_variants against solve.  Comparisons are bit for bit (tests/_lp_batch.py::check_lp): status, pivot count, result,
both permutations, column 0 and (with keep_tableaux) every word of the final matrix.  The expected answer of a variant is
always the C oracle's on the dense tableau of tableau_model(apply_variant(model, variant)).

KERNELS holds one row per compiled instantiation of the solving kernel: the size class whose launch uses it, checkCycles,
and the (M, N) of a tests/_lp_variants.py::dense_model of that class; lp_variants_base_kernel builds the image.

tests/test_variant_shapes.py takes the kernel through what these tests do not reach: patches longer than a workgroup, a base
without cells, patch_offsets[0] > 0, both sides of every class bound, tests/_batch_shapes.py::shape_table and the edge families
of tests/_edges.py as variants, queue reuse in the HBM and the aux form with history reruns, a caller's stream."""
import math
import os
import re

import numpy as np
import pytest

from tests import _batch_shapes as BS
from tests import _cases as K
from tests import _lp_batch as B
from tests import _lp_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = {
    "lp_variants_kernel<256,lds>": (0, False, (30, 30)),
    "lp_variants_kernel<256,check,lds>": (0, True, (30, 30)),
    "lp_variants_kernel<1024,lds>": (3, False, (130, 120)),
    "lp_variants_kernel<1024,check,lds>": (3, True, (130, 120)),
    "lp_variants_kernel<1024>": (4, False, (300, 280)),
    "lp_variants_kernel<1024,check>": (4, True, (300, 280)),
}
BASE_KERNEL = "lp_variants_base_kernel"


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpvar()
    return _native


# ---------------------------------------------------------------------------------------------------------- CPU

def test_patch_equals_rebuild_on_every_golden_model():
    from yalps_amd.model import apply_variant, tableau_model, tableau_model_with_bounds, variant_patch
    rng = np.random.default_rng(20261017)
    names = K.names()
    assert len(names) == 46
    patched_cells = 0
    for name in names:
        model = K.load(name)["model"]
        tabmod, info = tableau_model_with_bounds(model, sparse=True)
        assert B.same_words(tabmod.tableau.dense(), tableau_model(model).tableau.matrix), name
        tabmod.tableau.matrix = None
        for k in range(1 if name in K.LARGE else 3):
            variant = V.seeded_variant(model, rng)
            patch = variant_patch(tabmod, info, variant)
            assert patch is not None, (name, variant)
            row, col, val = patch
            key = row.astype(np.int64) * tabmod.tableau.width + col
            assert np.all(np.diff(key) > 0) and row.dtype == col.dtype == np.int32, name
            want = tableau_model(apply_variant(model, variant)).tableau
            assert (want.width, want.height) == (tabmod.tableau.width, tabmod.tableau.height), name
            assert B.same_words(V.patched_matrix(tabmod, patch), want.matrix), (name, k, variant)
            patched_cells += row.size
        empty = variant_patch(tabmod, info, {})
        assert empty is not None and all(a.size == 0 for a in empty)
    assert patched_cells > 46 * 3


def test_patch_writes_minus_zero_where_tableau_model_does():
    from yalps_amd.model import apply_variant, tableau_model, tableau_model_with_bounds, variant_patch
    model = {"direction": "minimize", "objective": "cost", "constraints": {"a": {"min": 2}, "b": {"min": 1, "max": 4}, "e": {"equal": 3}},
             "variables": {"x": {"a": 1, "b": 2, "cost": 3}, "y": {"a": 2, "e": 1, "cost": 0}}}
    variant = {"constraints": {"a": {"min": 0}, "b": {"min": 0, "max": 0}, "e": {"min": -1, "max": -1}}, "variables": {"y": {"cost": 0, "b": 0}}}
    tabmod, info = tableau_model_with_bounds(model, sparse=True)
    row, col, val = variant_patch(tabmod, info, variant)
    want = tableau_model(apply_variant(model, variant)).tableau.matrix
    assert B.same_words(V.patched_matrix(tabmod, (row, col, val)), want)
    minus_zero = np.flatnonzero(val.view(np.int64) == np.float64(-0.0).view(np.int64))
    assert minus_zero.size >= 3  # -lower of a and b, sign * 0 of y's cost, -coef of b's lower row


def test_structure_changes_and_unknown_keys():
    from yalps_amd.model import apply_variant, tableau_model, tableau_model_with_bounds, variant_patch
    model = {"direction": "maximize", "objective": "p", "constraints": {"up": {"max": 10}, "lo": {"min": 1}, "both": {"min": 0, "max": 5},
                                                                             "eq": {"equal": 2}},
             "variables": {"x": {"up": 1, "lo": 1, "both": 1, "p": 2}, "y": {"up": 2, "eq": 1, "p": 1}}}
    tabmod, info = tableau_model_with_bounds(model, sparse=True)
    changes = ({"up": {"equal": 3}}, {"lo": {"max": 3}}, {"both": {"max": 5}}, {"eq": {"min": 2}}, {"up": {}}, {"up": {"max": math.inf}})
    for cons in changes:
        assert variant_patch(tabmod, info, {"constraints": cons}) is None, cons
        t = tableau_model(apply_variant(model, {"constraints": cons})).tableau  # (apply_variant still gives the model)
        assert (t.height, t.width) != (tabmod.tableau.height, tabmod.tableau.width) or cons == {"lo": {"max": 3}}
    # same finite sides under another spelling: a patch
    for cons in ({"eq": {"min": 2, "max": 2}}, {"both": {"equal": 1}}, {"up": {"max": -1}}):
        patch = variant_patch(tabmod, info, {"constraints": cons})
        assert patch is not None
        assert B.same_words(V.patched_matrix(tabmod, patch), tableau_model(apply_variant(model, {"constraints": cons})).tableau.matrix)
    for bad in ({"constraints": {"nope": {"max": 1}}}, {"variables": {"z": {"up": 1}}}):
        with pytest.raises(ValueError):
            variant_patch(tabmod, info, bad)
        with pytest.raises(ValueError):
            apply_variant(model, bad)
    # a coefficient for a constraint key the model lacks is what it is in tableau_model: no cell
    patch = variant_patch(tabmod, info, {"variables": {"x": {"unheard": 4.0}}})
    assert all(a.size == 0 for a in patch)
    # apply_variant copies nothing it does not change
    applied = apply_variant(model, {"constraints": {"up": {"max": 4}}, "variables": {"y": {"p": 7}}})
    assert applied["variables"]["x"] is model["variables"]["x"] and applied["constraints"]["lo"] is model["constraints"]["lo"]
    assert model["variables"]["y"]["p"] == 1 and model["constraints"]["up"] == {"max": 10}
    assert list(applied["constraints"]) == list(model["constraints"]) and list(applied["variables"]) == list(model["variables"])


def test_iterable_models_with_duplicate_keys():
    from yalps_amd.model import apply_variant, tableau_model, tableau_model_with_bounds, variant_patch
    model = {"direction": "minimize", "objective": "c",
             "constraints": [("r", {"min": 1}), ("s", {"max": 9}), ("r", {"max": 6}), ("t", {"equal": 2}), ("s", {"max": 7})],
             "variables": [("x", [("r", 1), ("c", 2), ("r", 3)]), ("y", {"s": 1, "t": 1, "c": 1}), ("x", [("t", 2), ("c", 5)])]}
    tabmod, info = tableau_model_with_bounds(model, sparse=True)
    assert tabmod.tableau.width == 4 and info["columns"]["x"] == [1, 3]
    variants = [
        {"constraints": {"r": {"min": 0, "max": 2}}},                       # both entries of r replaced by one
        {"constraints": {"s": {"max": -4}}, "variables": {"x": {"r": 8, "s": 0.5}}},  # both x columns
        {"variables": {"y": {"c": -1, "r": 2}, "x": {"c": 0}}},
    ]
    for v in variants:
        applied = apply_variant(model, v)
        assert [k for k, _ in applied["constraints"]].count("r") == (1 if "r" in v.get("constraints", {}) else 2)
        patch = variant_patch(tabmod, info, v)
        assert patch is not None
        assert B.same_words(V.patched_matrix(tabmod, patch), tableau_model(applied).tableau.matrix), v
    assert variant_patch(tabmod, info, {"constraints": {"r": {"min": 1}}}) is None  # merged r was two-sided
    with pytest.raises(ValueError):
        apply_variant(model, {"constraints": {"u": {"max": 1}}})


def oracle_variants_backend(oracle):
    """variants_backend of _solve_variants_with by the C oracle: the base's cells with the patch over them, dense."""
    def backend(tableau, patches, options, stats=None):
        out = []
        row, col, val = tableau.cells
        w, h = tableau.width, tableau.height
        for patch, o in zip(patches, options):
            m = np.zeros(w * h, np.float64)
            m[row.astype(np.int64) * w + col] = val
            for k, v in patch:
                m[k] = v
            pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
            status, result, _, _ = oracle.simplex(m, w, h, pos, var, precision=o["precision"], max_pivots=o["maxPivots"],
                                                  check_cycles=o["checkCycles"])
            out.append((status, result, m[::w].copy(), pos, var))
        if stats is not None:
            stats.update(launches=1, reruns=0, kernels=["oracle"])
        return out
    return backend


def oracle_solve_many(oracle):
    from tests.test_lp_batch import oracle_backend, oracle_batch_backend
    from yalps_amd import solve as S
    one = oracle_backend(oracle)
    return one, lambda models, options, stats: S._solve_many_with(oracle_batch_backend(oracle), lambda m, o: S._solve_with(one, m, o),
                                                                   models, options, stats)


def test_solve_variants_routing_and_marshalling_with_the_oracle(oracle):
    from tests.test_lp_batch import same_solution
    from yalps_amd import solve as S
    from yalps_amd.model import apply_variant, tableau_model
    one, many = oracle_solve_many(oracle)
    rng = np.random.default_rng(5)
    lp_names = [n for n in K.names() if n not in K.LARGE and not tableau_model(K.load(n)["model"], sparse=True).integers][:6]
    milp_name = next(n for n in K.names() if n not in K.LARGE and tableau_model(K.load(n)["model"], sparse=True).integers)
    assert len(lp_names) == 6
    for name in lp_names:  # a patched base
        case = K.load(name)
        variants = [{}] + [V.seeded_variant(case["model"], rng) for _ in range(5)]
        stats = {}
        got = S._solve_variants_with(oracle_variants_backend(oracle), many, case["model"], variants, case["options"], stats)
        expected = [S._solve_with(one, apply_variant(case["model"], v), case["options"]) for v in variants]
        assert all(same_solution(g, e) for g, e in zip(got, expected)), name
        assert (stats["patched"], stats["materialised"], stats["launches"]) == (6, 0, 1) and "solve_many" not in stats
        assert stats["base_cells"] == tableau_model(case["model"], sparse=True).tableau.cells[0].size
        assert stats["patch_cells"] > 0
    # a base with integers: every variant materialised, in one solve_many call
    case = K.load(milp_name)
    variants = [{}] + [V.seeded_variant(case["model"], rng, n_variables=1) for _ in range(2)]
    stats = {}
    got = S._solve_variants_with(oracle_variants_backend(oracle), many, case["model"], variants, case["options"], stats)
    expected = [S._solve_with(one, apply_variant(case["model"], v), case["options"]) for v in variants]
    assert all(same_solution(g, e) for g, e in zip(got, expected))
    assert (stats["patched"], stats["materialised"], stats["launches"]) == (0, 3, 0) and stats["solve_many"]["milp"] == 3
    # structure-changing variants among patched ones, per-variant options: order preserved
    model = V.dense_model(oracle, 12, 10, 4)
    variants = V.shape_variants(12, 10)
    variants[2:2] = [{"constraints": {"c3": {"equal": 2.0}}}]
    variants.append({"constraints": {"c1": {"min": 0.5}}, "variables": {"x2": {"obj": 3.0}}})
    options = [{"maxPivots": p, "checkCycles": c, "precision": q, "includeZeroVariables": z}
               for p, c, q, z in zip((8192, 0, 8192, 2.5, math.inf, 3, 8192, 8192, 1, 8192), (False, True) * 5, (1e-8, 1e-8, 1e-6) * 4,
                                     (False, False, True) * 4)]
    calls = []
    stats = {}
    got = S._solve_variants_with(oracle_variants_backend(oracle), lambda *a: calls.append(len(a[0])) or many(*a), model, variants,
                                 options, stats)
    expected = [S._solve_with(one, apply_variant(model, v), o) for v, o in zip(variants, options)]
    assert len(got) == len(variants) == 10 and all(same_solution(g, e) for g, e in zip(got, expected))
    assert (stats["patched"], stats["materialised"], calls) == (8, 2, [2]) and stats["solve_many"]["batched"] == 2
    assert len({g["status"] for g in got}) >= 2
    with pytest.raises(ValueError):
        S._solve_variants_with(oracle_variants_backend(oracle), many, model, variants[:3], [{}, {}])
    assert S._solve_variants_with(oracle_variants_backend(oracle), many, model, []) == []


def test_header_symbols_are_exported(nat):
    text = open(os.path.join(ROOT, "include", "yalps_lpvar.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text))
    assert declared and all(s.startswith("yalps_lpvar_") for s in declared), declared
    L = nat.lpvar_lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(nat.SYMBOLS_LPVAR)
    assert not set(nat.SYMBOLS_LPVAR) & (set(nat.SYMBOLS) | set(nat.SYMBOLS_LPBATCH) | set(nat.SYMBOLS_MILPBATCH))


def test_kernels_are_the_table(nat):
    from yalps_amd import build
    ks = build.kernel_metadata(lib=build.LIB_LPVAR)
    spelt = {V.spelling(s): md for s, md in ks.items()}
    assert len(spelt) == len(ks)
    assert set(spelt) == set(KERNELS) | {BASE_KERNEL}, sorted(set(spelt) ^ (set(KERNELS) | {BASE_KERNEL}))
    for name, md in spelt.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0, (name, md)
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (name, md["group_segment_fixed_size"])
    for name, (cls, check, (M, N)) in KERNELS.items():
        assert B.size_class(N + 1, M + 1) == cls == B.size_class(N, M + 1), name  # (the odd-n shape of the GPU test too)
        assert V.kernel_of(cls, check) == name
    build.check_register_budgets(lib=build.LIB_LPVAR, min_resident=0)
    # the other three libraries stay what their own tests pin: nothing of this one in them
    build.build_hip(), build.build_lpbatch(), build.build_milpbatch()
    for lib in (build.LIB, build.LIB_LPBATCH, build.LIB_MILPBATCH):
        assert not [k for k in build.kernel_metadata(lib=lib) if "lp_variants" in k], lib


def test_validate_names_the_variant_before_any_device_call(nat, oracle):
    model = V.dense_model(oracle, 5, 4, 1)
    good = V.packed(nat, model, V.shape_variants(5, 4))
    good.validate()
    assert good.count == 8 and good.offsets[1] == 0 and good.patch_row.size == good.offsets[-1] > 0

    def broken(**change):
        p = V.packed(nat, model, V.shape_variants(5, 4))
        for k, v in change.items():
            setattr(p, k, v)
        return p

    lo, hi = int(good.offsets[3]), int(good.offsets[4])
    assert hi - lo >= 2
    off = good.offsets.copy()
    off[4] = off[3] - 1  # (variant 3 ends before it starts)
    col, row, rev_r, rev_c = good.patch_col.copy(), good.patch_row.copy(), good.patch_row.copy(), good.patch_col.copy()
    col[lo] = good.width
    row[hi - 1] = good.height
    rev_r[lo:hi], rev_c[lo:hi] = good.patch_row[lo:hi][::-1], good.patch_col[lo:hi][::-1]
    twice_r, twice_c = good.patch_row.copy(), good.patch_col.copy()
    twice_r[lo + 1], twice_c[lo + 1] = twice_r[lo], twice_c[lo]
    for p, what in ((broken(offsets=off), "variant 3: patch offsets decrease"),
                    (broken(patch_col=col), "variant 3: patch cell 0 lies outside"),
                    (broken(patch_row=row), "variant 3: patch cell %d lies outside" % (hi - lo - 1)),
                    (broken(patch_row=rev_r, patch_col=rev_c), "variant 3: .*not sorted"),
                    (broken(patch_row=twice_r, patch_col=twice_c), "variant 3: .*not sorted"),
                    (broken(width=1024, height=513), "above the limit"),
                    (broken(width=0), "at least 1"), (broken(height=0), "at least 1"),
                    (broken(row=good.row[::-1].copy(), col=good.col[::-1].copy()), "base cells are not sorted"),
                    (broken(col=good.col + good.width), "base cell 0 lies outside")):
        with pytest.raises(nat.NativeError, match=what):
            p.validate()
    empty = nat.PackedVariants(good.width, good.height, good.row, good.col, good.val, [])
    empty.validate()
    no_cells = nat.PackedVariants(3, 2, *(np.zeros(0, t) for t in (np.int32, np.int32, np.float64)), [(np.zeros(0, np.int32),) * 2 + (np.zeros(0),)])
    no_cells.validate()


def test_no_cpu_fallback(nat):
    from yalps_amd import build
    build.build_hip()
    if nat.lib().yalps_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(nat.NativeError, match="no HIP device"):
        nat.LpVariants(0)


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu(nat):
    assert nat.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return nat


@pytest.fixture(scope="module")
def lv(gpu):
    v = gpu.LpVariants(0)
    yield v
    v.close()


def run_and_check(nat, lv, oracle, model, variants, options=None, label=""):
    """One call of LpVariants on (model, variants); every variant against the oracle on its rebuilt tableau.  Returns (info, refs)."""
    per = options if isinstance(options, (list, tuple)) else [options] * len(variants)
    lps = [V.variant_lp(model, v, o) for v, o in zip(variants, per)]
    refs = [B.oracle_answer(oracle, lp) for lp in lps]
    out = lv.solve(V.packed(nat, model, variants, per), keep_tableaux=True)
    assert len(out[0]) == len(variants)
    for i, (lp, ref) in enumerate(zip(lps, refs)):
        B.check_lp(lv, i, out, ref, lp, label="%s variant %d" % (label, i))
    return lv.info(), refs


def launches_of(info, passes=(0,)):
    return sorted((k["kernel"], k["class"], k["lps"]) for k in info["kernels"] if k["pass"] in passes)


@pytest.fixture(scope="module")
def shape_models(oracle):
    """dense_model per (M, N) of KERNELS and its odd-n neighbour, built once."""
    return {(M, N): V.dense_model(oracle, M, N, 3) for _, _, (M0, N0) in KERNELS.values() for M, N in ((M0, N0), (M0, N0 - 1))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_every_instantiation_by_name(gpu, lv, oracle, shape_models, name):
    cls, check, (M, N0) = KERNELS[name]
    for N in (N0, N0 - 1):  # even n | odd n: the last column shares its 16-byte unit with the pitch padding
        variants = V.shape_variants(M, N)
        assert len(variants) == 8
        info, refs = run_and_check(gpu, lv, oracle, shape_models[(M, N)], variants, {"checkCycles": check}, label=name)
        assert launches_of(info) == [(name, cls, 8)] and info["launches"] == 1 and info["reruns"] == 0
        assert info["kernels"][0]["aux"] == 0 and info["patch_cells"] > 0
        assert len({r["n_pivots"] for r in refs}) > 4  # (the patches matter: the variants take different paths)


def tiny_models():
    no_vars = {"direction": "maximize", "objective": "p", "constraints": {"a": {"max": 1}, "b": {"max": 2}, "c": {"min": -3, "max": 5}},
               "variables": {}}
    no_rows_odd = {"direction": "maximize", "objective": "p", "constraints": {}, "variables": {"x%d" % j: {"p": -1.0 - j} for j in range(7)}}
    no_rows_even = {"direction": "minimize", "objective": "p", "constraints": {}, "variables": {"x%d" % j: {"p": 1.0 + j} for j in range(8)}}
    one_row = {"direction": "maximize", "objective": "p", "constraints": {"a": {"max": 4}}, "variables": {"x": {"a": 2, "p": 1}}}
    return [
        ("w = 1", no_vars, [{}, {"constraints": {"a": {"max": -1}}}, {"constraints": {"c": {"min": 0, "max": 0}}},
                            {"constraints": {"b": {"max": 0}, "c": {"min": 6, "max": 5}}}], (1, 5)),
        ("h = 1, n odd", no_rows_odd, [{}, {"variables": {"x6": {"p": 2.0}}}, {"variables": {"x0": {"p": 0}, "x3": {"p": 1.5}}}], (8, 1)),
        ("h = 1, n even", no_rows_even, [{}, {"variables": {"x7": {"p": -2.0}}}, {"variables": {"x0": {"p": -1}, "x7": {"p": 0}}}], (9, 1)),
        ("w = 2, h = 2", one_row, [{}, {"constraints": {"a": {"max": 0}}}, {"variables": {"x": {"a": -1}}}, {"variables": {"x": {"p": -1}}}], (2, 2)),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("check", (False, True))
def test_degenerate_shapes(gpu, lv, oracle, check):
    for label, model, variants, (w, h) in tiny_models():
        info, refs = run_and_check(gpu, lv, oracle, model, variants, {"checkCycles": check}, label=label)
        assert launches_of(info) == [(V.kernel_of(0, check), 0, len(variants))], label
        assert (refs[0]["matrix"].size, h) == (w * h, h), label
        assert len({r["status"] for r in refs}) >= 2 or label == "w = 2, h = 2", label
    # the aux form of the HBM class, at its bound: even(w - 1) + h = 8193 with one variable (8192 stays in LDS)
    w, h = 2, 8191
    assert BS.aux_hbm(w, h) and not BS.aux_hbm(w, h - 1) and B.size_class(w, h) == 4
    model = V.dense_model(oracle, h - 1, 1, 3, holes=False)
    variants = [{}, {"constraints": {"c%d" % (h - 1): {"max": 0.001}}}, {"variables": {"x1": {"c1": 900.0, "obj": 2.0}}},
                {"constraints": {"c7": {"max": -1.0}}}, {"variables": {"x1": {"obj": -1.0}}}]
    info, refs = run_and_check(gpu, lv, oracle, model, variants, {"checkCycles": check}, label="aux")
    assert launches_of(info) == [(V.kernel_of(4, check), 4, 5)] and info["kernels"][0]["aux"] == 1
    assert {r["status"] for r in refs} == {"optimal", "infeasible"} and max(r["n_pivots"] for r in refs) >= 1


@pytest.mark.gpu
def test_no_state_leaks_through_the_queue(gpu, oracle, monkeypatch):
    """4 x the grid's variants, a heavy patch and the empty patch in turn: a workgroup that kept anything of the variant
    before (a patched cell, a permutation, a right-hand side) would get the empty-patch variant after it wrong."""
    monkeypatch.setenv("YALPS_LPVAR_PER_CU", "1")
    v = gpu.LpVariants(0)
    try:
        M, N = 12, 11
        model = V.dense_model(oracle, M, N, 8)
        rng = np.random.default_rng(12)
        first = v.solve(V.packed(gpu, model, [{}] * 2))
        grid = 256  # one workgroup per CU with the hook (asserted below)
        variants = []
        for k in range(2 * grid):
            heavy = {"constraints": {"c%d" % r: {"max": float(rng.integers(1, 9))} for r in range(1, M + 1)},
                     "variables": {"x%d" % j: {"obj": float(rng.integers(-3, 9)), "c%d" % (1 + (j + k) % M): float(rng.random())}
                                   for j in range(1, N + 1)}}
            variants += [heavy, {}]
        lps = [V.variant_lp(model, x) for x in variants]
        base_ref = B.oracle_answer(oracle, lps[1])
        out = v.solve(V.packed(gpu, model, variants), keep_tableaux=True)
        info = v.info()
        assert info["launches"] == 1 and info["kernels"][0]["lps"] == len(variants) == 4 * info["kernels"][0]["grid"], info["text"]
        for i, lp in enumerate(lps):
            B.check_lp(v, i, out, base_ref if i % 2 else B.oracle_answer(oracle, lp), lp, label="queue")
        assert first[0] == [base_ref["status"]] * 2
    finally:
        v.close()


@pytest.mark.gpu
def test_mixed_endings_in_one_call(gpu, lv, oracle):
    M, N = 12, 10
    model = V.dense_model(oracle, M, N, 6)
    unbounded = {"variables": {"x3": dict({"c%d" % r: -0.5 for r in range(1, M + 1)}, obj=4.0)}}
    infeasible = {"constraints": {"c2": {"max": -1.0}}}
    variants = [{}, infeasible, unbounded, V.shape_variants(M, N)[3], {}, {}, {}, {}, infeasible, unbounded]
    budgets = [8192, 8192, 8192, 8192, 0, 2.5, math.inf, 1, math.inf, 0.5]
    options = [{"maxPivots": b, "checkCycles": bool(i % 2)} for i, b in enumerate(budgets)]
    info, refs = run_and_check(gpu, lv, oracle, model, variants, options, label="endings")
    assert [r["status"] for r in refs[:3]] == ["optimal", "infeasible", "unbounded"]
    assert [(r["status"], r["n_pivots"]) for r in refs[4:6]] == [("cycled", 0), ("cycled", 3)] and refs[6]["status"] == "optimal"
    assert info["launches"] == 2 and sorted(k["lps"] for k in info["kernels"]) == [5, 5]
    # hasCycle ends a variant: the cycling golden base with checkCycles on, next to variants it does not end
    case = K.load("Chvatal Cycling")
    cyc = case["model"]
    key = next(iter(dict(cyc["constraints"]) if isinstance(cyc["constraints"], dict) else cyc["constraints"]))
    key = key if isinstance(cyc["constraints"], dict) else key[0]
    variants = [{}, {}, {"constraints": {key: {"max": 5.0}}}, {"constraints": {key: {"max": 5.0}}}]
    options = [dict(case["options"], checkCycles=c, maxPivots=m) for c, m in ((True, 8192), (False, 64), (True, 8192), (True, 0))]
    info, refs = run_and_check(gpu, lv, oracle, cyc, variants, options, label="Chvatal")
    assert refs[0]["status"] == "cycled" and refs[0]["n_pivots"] < 64 == refs[1]["n_pivots"] and refs[3]["n_pivots"] == 0


@pytest.mark.gpu
def test_history_rerun_only_for_the_variants_that_overflowed(gpu, oracle, monkeypatch):
    cap = 8
    monkeypatch.setenv("YALPS_LPVAR_HIST", str(cap))
    v = gpu.LpVariants(0)
    try:
        for (M, N, seed), cls in (((96, 80, 9), 2), ((300, 280, 3), 4)):  # (long enough: the oracle's pivot counts are asserted below)
            model = V.dense_model(oracle, M, N, seed)
            variants = V.shape_variants(M, N)[:6]
            options = [{"checkCycles": c, "maxPivots": p} for c, p in ((True, 8192), (True, 8192), (False, 8192), (True, 3), (True, 8192), (False, 8192))]
            info, refs = run_and_check(gpu, v, oracle, model, variants, options, label="hist")
            rerun = set(info["rerun_lps"])
            # a phase holds at most `cap` pivots before the history is full: more than 2 * cap pivots must have overflowed,
            # at most `cap` pivots (or no checkCycles) cannot have
            must = {i for i, (o, r) in enumerate(zip(options, refs)) if o["checkCycles"] and r["n_pivots"] > 2 * cap}
            never = {i for i, (o, r) in enumerate(zip(options, refs)) if not o["checkCycles"] or r["n_pivots"] <= cap}
            assert {0, 1, 4} <= must and {2, 3, 5} <= never, (must, never)
            assert must <= rerun and not rerun & never, (sorted(rerun), sorted(must), sorted(never))
            assert info["reruns"] == len(info["rerun_lps"]) >= len(must)
            later = [k for k in info["kernels"] if k["pass"] > 0]
            assert later and all(k["kernel"] == V.kernel_of(cls, True) and k["hist_cap"] == cap * 4 ** k["pass"] for k in later)
            assert sum(k["lps"] for k in later) == info["reruns"]
    finally:
        v.close()


@pytest.mark.gpu
def test_handle_reuse_across_shapes_and_counts(gpu, oracle):
    v = gpu.LpVariants(0)
    try:
        for (M, N), count in (((12, 10), 8), ((96, 80), 3), ((5, 4), 6)):
            model = V.dense_model(oracle, M, N, 2)
            variants = V.shape_variants(M, N)[:count]
            run_and_check(gpu, v, oracle, model, variants)
            with pytest.raises(gpu.NativeError, match="no such variant"):
                v.solution(count)
        p = V.packed(gpu, model, variants)
        v.solve(p)
        with pytest.raises(gpu.NativeError, match="keep_tableaux"):
            v.tableau(0)
        statuses, results, pivots, _ = v.solve(gpu.PackedVariants(p.width, p.height, p.row, p.col, p.val, []))
        assert statuses == [] and results.size == 0 and pivots.size == 0 and v.info()["launches"] == 0
        with pytest.raises(gpu.NativeError, match="no such variant"):
            v.solution(0)
        # a refused call launches nothing and leaves no last solve behind
        p.patch_col = p.patch_col + p.width
        with pytest.raises(gpu.NativeError, match="variant 1: .*outside"):
            v.solve(p)
    finally:
        v.close()


@pytest.mark.gpu
def test_solve_variants_equals_solve_on_golden_models(gpu):
    from tests.test_lp_batch import same_solution
    from yalps_amd import solve as S
    from yalps_amd.model import apply_variant, tableau_model
    rng = np.random.default_rng(9)
    small = [n for n in K.names() if n not in K.LARGE]
    lp_names = [n for n in small if not tableau_model(K.load(n)["model"], sparse=True).integers][:3]
    milp_name = next(n for n in small if tableau_model(K.load(n)["model"], sparse=True).integers)
    assert len(lp_names) == 3
    for name in lp_names:
        case = K.load(name)
        variants = [{}] + [V.seeded_variant(case["model"], rng) for _ in range(6)]
        options = [dict(case["options"], checkCycles=bool(i % 2)) for i in range(len(variants))]
        stats = {}
        got = S.solve_variants(case["model"], variants, options, stats)
        assert (stats["patched"], stats["materialised"]) == (7, 0) and 1 <= stats["launches"] == len(stats["kernels"]), (name, stats)
        assert all(k["kernel"].startswith("lp_variants_kernel<") for k in stats["kernels"])
        for v, o, g in zip(variants, options, got):
            e = S.solve(apply_variant(case["model"], v), o)
            assert same_solution(g, e), (name, v, g, e)
        assert same_solution(got[0], S.solve(case["model"], options[0]))
    case = K.load(milp_name)
    variants = [{}, V.seeded_variant(case["model"], rng, n_variables=1)]
    stats = {}
    got = S.solve_variants(case["model"], variants, case["options"], stats)
    assert (stats["patched"], stats["materialised"], stats["launches"]) == (0, 2, 0) and stats["solve_many"]["milp"] == 2
    for v, g in zip(variants, got):
        assert same_solution(g, S.solve(apply_variant(case["model"], v), case["options"])), (milp_name, v)
