"""Batches of independent LPs (include/yalps_lpbatch.h, yalps_amd.solve.solve_many): libyalps_lpbatch.so's boundary, its
kernels by name, the packing and the class binning on the CPU; on the GPU every golden and edge record within the batch
limit in one call, every kernel instantiation, the work queue, budgets, the checkCycles history rerun, handle reuse and
solve_many against solve.  Comparisons are bit for bit: status, pivot count, result, both permutations, column 0 and (with
keep_tableaux) every word of the final matrix.

KERNELS holds one row per compiled instantiation: the size class whose launch uses it, checkCycles, and a dense-LP(M, N)
that lands in that class."""
import math
import os
import re

import numpy as np
import pytest

from tests import _cases as K
from tests import _golden as G
from tests import _lp_batch as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel spelling -> (size class, checkCycles, (M, N) of a dense LP of that class)
KERNELS = {
    "lp_batch_kernel<256,lds>": (0, False, (30, 30)),
    "lp_batch_kernel<256,check,lds>": (0, True, (30, 30)),
    "lp_batch_kernel<1024,lds>": (3, False, (130, 120)),
    "lp_batch_kernel<1024,check,lds>": (3, True, (130, 120)),
    "lp_batch_kernel<1024>": (4, False, (300, 280)),
    "lp_batch_kernel<1024,check>": (4, True, (300, 280)),
}
# a dense-LP(M, N) of every class (classes 0..2 share the 256-lane kernels)
CLASS_SHAPES = {0: (30, 30), 1: (60, 50), 2: (96, 80), 3: (130, 120), 4: (300, 280)}
CLASS_LANES = {0: 256, 1: 256, 2: 256, 3: 1024, 4: 1024}


def kernel_of(cls, check):
    return "lp_batch_kernel<%d%s%s>" % (CLASS_LANES[cls], ",check" if check else "", ",lds" if cls < 4 else "")


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpbatch()
    return _native


# ---------------------------------------------------------------------------------------------------------- CPU

def test_header_symbols_are_exported(nat):
    text = open(os.path.join(ROOT, "include", "yalps_lpbatch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text))
    assert declared and all(s.startswith("yalps_lpbatch_") for s in declared), declared
    L = nat.lpbatch_lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(nat.SYMBOLS_LPBATCH)
    assert not set(nat.SYMBOLS_LPBATCH) & set(nat.SYMBOLS)


def test_no_cpu_fallback(nat):
    from yalps_amd import build
    build.build_hip()
    if nat.lib().yalps_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(nat.NativeError, match="no HIP device"):
        nat.LpBatch(0)


def test_kernels_are_the_table_and_stay_out_of_the_main_library(nat):
    from yalps_amd import build
    ks = build.kernel_metadata(lib=build.LIB_LPBATCH)
    spelt = {B.spelling(s): md for s, md in ks.items()}
    assert len(spelt) == len(ks)
    assert set(spelt) == set(KERNELS), sorted(set(spelt) ^ set(KERNELS))
    for name, md in spelt.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0, (name, md)
        # the dynamic LDS block (tableau, pivot row: 128-bit accesses) starts where the static LDS ends
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (name, md["group_segment_fixed_size"])
    for name, (cls, check, (M, N)) in KERNELS.items():
        assert nat.lpbatch_class(N + 1, M + 1) == cls == B.size_class(N + 1, M + 1), name
        assert kernel_of(cls, check) == name
    build.check_register_budgets(lib=build.LIB_LPBATCH, min_resident=0)
    build.build_hip()
    assert not [s for s in build.kernel_metadata() if "lp_batch" in s]


def seeded_dense(oracle, count=12):
    rng = np.random.default_rng(20261016)
    return [B.dense_lp(oracle, int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(1, 1000))) for _ in range(count)]


def test_packing_reproduces_the_reference_tableau(nat, oracle):
    from yalps_amd.model import tableau_model
    from yalps_amd.solve import default_options
    lps, dense = [], []
    for name in K.names():
        model = K.load(name)["model"]
        lps.append(B.model_lp(tableau_model(model, sparse=True), default_options))
        dense.append(tableau_model(model).tableau.matrix)
    assert len(lps) == 46
    for lp in seeded_dense(oracle):
        lps.append(lp)
        dense.append(B.scatter(lp))
    p = nat.PackedLps(lps)
    assert p.count == len(lps) and p.offsets[0] == 0 and np.all(np.diff(p.offsets) >= 0) and p.offsets[-1] == p.row.size
    for i, (lp, ref) in enumerate(zip(lps, dense)):
        lo, hi = int(p.offsets[i]), int(p.offsets[i + 1])  # (consecutive, so no two LPs share a cell)
        w, h = int(p.width[i]), int(p.height[i])
        got = B.scatter((w, h, p.row[lo:hi], p.col[lo:hi], p.val[lo:hi]))
        assert B.same_words(got, ref), i
        key = p.row[lo:hi].astype(np.int64) * w + p.col[lo:hi]
        assert np.all(np.diff(key) > 0), i
    # what the library accepts: everything within the batch limit
    small = [lp for lp in lps if 8 * lp[0] * lp[1] <= B.MAX_BYTES]
    assert 0 < len(small) < len(lps)
    nat.PackedLps(small).validate()
    # dense_cells keeps a written -0.0
    m = np.array([0.0, -0.0, 1.0, 0.0, 2.0, -0.0])
    row, col, val = nat.dense_cells(m, 3, 2)
    assert list(row) == [0, 0, 1, 1] and list(col) == [1, 2, 1, 2] and B.same_words(val, m[[1, 2, 4, 5]])


def test_class_binning_on_both_sides_of_every_boundary(nat):
    for w in (2, 31, 64, 121):
        for k, bound in enumerate(B.BOUNDS):
            h = 1
            while B.lds_bytes(w, h + 1) <= bound:
                h += 1
            if 8 * w * (h + 1) > B.MAX_BYTES:
                continue
            assert nat.lpbatch_lds_bytes(w, h) == B.lds_bytes(w, h) <= bound < B.lds_bytes(w, h + 1)
            assert nat.lpbatch_class(w, h) == k and nat.lpbatch_class(w, h + 1) == k + 1, (w, h, k)
    assert nat.lpbatch_class(1024, 512) == 4 and nat.lpbatch_class(1024, 513) == -1  # 4 MiB exactly | above
    # the aux form of the HBM class: colbuf + prow (even(w - 1) + h doubles) above 64 KiB, on both sides of the bound
    for w, h in ((8152, 40), (8153, 40), (31, 8162), (30, 8162), (2, 8190), (1, 8192), (64, 8128)):
        assert (w & ~1) + h == 8192 and nat.lpbatch_class(w, h) == nat.lpbatch_class(w, h + 1) == 4
        assert (nat.lpbatch_aux_hbm(w, h), nat.lpbatch_aux_hbm(w, h + 1)) == (0, 1), (w, h)
    assert nat.lpbatch_aux_hbm(262144, 2) == 1 and nat.lpbatch_aux_hbm(64, 8191) == 1 and nat.lpbatch_aux_hbm(512, 1024) == 0
    assert nat.lpbatch_aux_hbm(30, 30) == 0 and nat.lpbatch_aux_hbm(1024, 513) == -1 and nat.lpbatch_aux_hbm(0, 5) == -1
    assert nat.lpbatch_class(0, 5) == -1 and nat.lpbatch_class(5, 0) == -1
    for cls, (M, N) in CLASS_SHAPES.items():
        assert nat.lpbatch_class(N + 1, M + 1) == cls


def test_argument_errors_name_the_lp_before_any_device_call(nat, oracle):
    """yalps_lpbatch_validate is what yalps_lpbatch_solve runs first; it needs no device."""
    good = B.dense_lp(oracle, 5, 4, 1)
    too_big = (1024, 513, *good[2:])
    unsorted_ = (good[0], good[1], good[2][::-1].copy(), good[3][::-1].copy(), good[4][::-1].copy(), *good[5:])
    twice = (good[0], good[1], np.repeat(good[2][:1], 2), np.repeat(good[3][:1], 2), np.repeat(good[4][:1], 2), *good[5:])
    outside = (good[0], good[1], good[2], good[3] + good[0], good[4], *good[5:])
    for bad, what in ((too_big, "above the batch limit"), (unsorted_, "not sorted"), (twice, "not sorted"), (outside, "outside"),
                      ((0, 3, *good[2:]), "at least 1"), ((3, 0, *good[2:]), "at least 1")):
        with pytest.raises(nat.NativeError, match="LP 2: .*" + what):
            nat.PackedLps([good, good, bad, good]).validate()
    nat.PackedLps([good, good]).validate()
    nat.PackedLps([]).validate()


def large_lp_model(nvars=800, ncons=700):
    """A model without integers whose tableau (801 x 701 doubles) is above the batch limit: none of the 46 cases is."""
    rng = np.random.default_rng(3)
    constraints = {"c%d" % j: {"max": float(rng.integers(50, 150))} for j in range(ncons)}
    variables = {}
    for i in range(nvars):
        coefs = {"c%d" % j: float(rng.integers(1, 9)) for j in rng.choice(ncons, 4, replace=False)}
        coefs["profit"] = float(rng.integers(1, 20))
        variables["x%d" % i] = coefs
    return {"direction": "maximize", "objective": "profit", "constraints": constraints, "variables": variables}


def same_solution(a, b):
    return (a["status"] == b["status"] and G.same_number(a["result"], b["result"]) and len(a["variables"]) == len(b["variables"])
            and all(ka == kb and G.same_number(va, vb) for (ka, va), (kb, vb) in zip(a["variables"], b["variables"])))


def oracle_backend(oracle):
    """simplex(tableau, options) by the C oracle, in place on the dense matrix (the backend _solve_with takes)."""
    def simplex(tableau, options):
        status, result, _, _ = oracle.simplex(tableau.matrix, tableau.width, tableau.height, tableau.position_of_variable,
                                              tableau.variable_at_position, precision=options["precision"],
                                              max_pivots=options["maxPivots"], check_cycles=options["checkCycles"])
        return status, result
    return simplex


def oracle_batch_backend(oracle):
    one = oracle_backend(oracle)

    def batch_simplex(tableaux, options, stats=None):
        out = []
        for t, o in zip(tableaux, options):
            assert t.matrix is None and t.cells is not None  # (built sparse, as the device takes them)
            t.dense()
            out.append(one(t, o))
        return out
    return batch_simplex


def test_solve_many_routing_and_marshalling_with_the_oracle(oracle):
    from yalps_amd import solve as S
    from yalps_amd.model import tableau_model
    cases = [K.load(n) for n in K.names()]
    assert len(cases) == 46
    cases.insert(20, {"name": "large LP", "model": large_lp_model(), "options": dict(S.default_options)})
    models = [c["model"] for c in cases]
    tms = [tableau_model(m, sparse=True) for m in models]
    milp = sum(1 for tm in tms if tm.integers)
    large = sum(1 for tm in tms if not tm.integers and 8 * tm.tableau.width * tm.tableau.height > S.NODE_BATCH_MAX_BYTES)
    assert milp > 0 and large == 1
    one = oracle_backend(oracle)
    routed = []

    def solve_one(model, options):
        routed.append(model)
        return S._solve_with(one, model, options)

    shared = {"precision": 1e-8, "checkCycles": True, "maxPivots": 4096}
    for options in ([c["options"] for c in cases], shared):
        per_model = options if isinstance(options, list) else [options] * len(models)
        expected = [S._solve_with(one, m, o) for m, o in zip(models, per_model)]
        del routed[:]
        stats = {}
        got = S._solve_many_with(oracle_batch_backend(oracle), solve_one, models, options, stats)
        assert len(got) == len(expected)
        for c, g, e in zip(cases, got, expected):
            assert same_solution(g, e), (c["name"], g["status"], e["status"])
        assert stats == {"batched": len(cases) - milp - large, "milp": milp, "large": large}
        assert [id(m) for m in routed] == [id(m) for m, tm in zip(models, tms)
                                           if tm.integers or 8 * tm.tableau.width * tm.tableau.height > S.NODE_BATCH_MAX_BYTES]
    with pytest.raises(ValueError):
        S._solve_many_with(oracle_batch_backend(oracle), solve_one, models[:3], [{}, {}])
    assert S._solve_many_with(oracle_batch_backend(oracle), solve_one, []) == []


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu(nat):
    assert nat.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return nat


@pytest.fixture(scope="module")
def batch(gpu):
    b = gpu.LpBatch(0)
    yield b
    b.close()


def launches_of(info, passes=(0,)):
    return sorted((k["kernel"], k["class"], k["lps"]) for k in info["kernels"] if k["pass"] in passes)


@pytest.mark.gpu
def test_golden_records_in_one_batch(batch, oracle):
    recs = [r for kind in ("cases", "mixed", "dense") for r in G.records(kind)]
    assert len(recs) == 108
    classes = [B.size_class(r["width"], r["height"]) for r in recs]
    assert sum(0 <= c < 4 for c in classes) == 94 and classes.count(4) == 10 and classes.count(-1) == 4
    kept = [r for r, c in zip(recs, classes) if c >= 0]
    assert sum(bool(r["options"]["checkCycles"]) for r in kept) == 15
    assert {r["status"] for r in kept} == {"optimal", "infeasible", "unbounded", "cycled"}
    lps = [B.record_lp(r, oracle) for r in kept]
    out = batch.solve(lps, keep_tableaux=True)
    for i, (r, lp) in enumerate(zip(kept, lps)):
        B.check_lp(batch, i, out, G.expected(r), lp, label=G.label(r))
    info = batch.info()
    first = [k for k in info["kernels"] if k["pass"] == 0]
    assert info["launches"] == len(info["kernels"]) and len(first) == len({(k["class"], "check" in k["kernel"]) for k in first})
    assert sum(k["lps"] for k in first) == 104


@pytest.mark.gpu
def test_edge_records_in_one_batch(batch, oracle):
    from tests import _edges as E
    recs = G.records("edges")
    assert len(recs) == 240
    kept = [r for r in recs if B.size_class(r["width"], r["height"]) >= 0]
    classes = [B.size_class(r["width"], r["height"]) for r in kept]
    assert len(kept) == 64 and sum(c < 4 for c in classes) == 16 and classes.count(4) == 48
    lps = [B.edge_lp(r, oracle) for r in kept]
    out = batch.solve(lps, keep_tableaux=True)
    for i, (r, lp) in enumerate(zip(kept, lps)):
        B.check_lp(batch, i, out, G.expected(r), lp, label=E.label(r))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_every_instantiation_by_name(batch, oracle, name):
    cls, check, (M, N) = KERNELS[name]
    lps = [B.dense_lp(oracle, M, N, seed, check_cycles=check) for seed in (3, 4)]
    out = batch.solve(lps, keep_tableaux=True)
    for i, lp in enumerate(lps):
        B.check_lp(batch, i, out, B.oracle_answer(oracle, lp), lp, label=name)
    assert launches_of(batch.info()) == [(name, cls, 2)]


def small_lps(oracle, count):
    rng = np.random.default_rng(7)
    return [B.dense_lp(oracle, int(rng.integers(3, 15)), int(rng.integers(3, 15)), 1 + i) for i in range(count)]


@pytest.mark.gpu
def test_queue_hands_out_more_lps_than_workgroups(batch, oracle):
    lps = small_lps(oracle, 5200)
    refs = [B.oracle_answer(oracle, lp) for lp in lps]
    out = batch.solve(lps, keep_tableaux=True)
    info = batch.info()
    assert info["launches"] == 1 and info["kernels"][0]["lps"] == 5200 > info["kernels"][0]["grid"]
    for i, (lp, ref) in enumerate(zip(lps, refs)):
        B.check_lp(batch, i, out, ref, lp)
    shuffled = list(np.random.default_rng(11).permutation(len(lps)))
    for order in (list(range(len(lps)))[::-1], shuffled):
        sub = [lps[j] for j in order]
        out = batch.solve(sub, keep_tableaux=True)
        for i, j in enumerate(order):
            B.check_lp(batch, i, out, refs[j], lps[j])
    out = batch.solve(lps[:1], keep_tableaux=True)
    B.check_lp(batch, 0, out, refs[0], lps[0])
    assert batch.info()["kernels"][0]["grid"] == 1
    statuses, results, pivots, _ = batch.solve([])
    assert statuses == [] and results.size == 0 and pivots.size == 0 and batch.info()["launches"] == 0


@pytest.mark.gpu
def test_mixed_launch_one_per_class_and_check(batch, oracle):
    lps, want = [], {}
    for cls, (M, N) in CLASS_SHAPES.items():
        for check in (False, True):
            if (cls, check) == (1, True):
                continue  # (an empty pair: no launch for it)
            n = 3 if cls < 4 else 1
            lps += [B.dense_lp(oracle, M, N, 10 * cls + s, check_cycles=check) for s in range(n)]
            want[(kernel_of(cls, check), cls)] = n
    order = list(np.random.default_rng(5).permutation(len(lps)))
    lps = [lps[j] for j in order]
    out = batch.solve(lps, keep_tableaux=True)
    for i, lp in enumerate(lps):
        B.check_lp(batch, i, out, B.oracle_answer(oracle, lp), lp)
    info = batch.info()
    assert info["launches"] == 9 and info["reruns"] == 0
    assert launches_of(info) == sorted((k, c, n) for (k, c), n in want.items())


@pytest.mark.gpu
def test_budgets_per_lp(batch, oracle):
    lps = []
    for M, N in ((30, 30), (96, 80), (300, 280)):
        for budget in (0, 2.5, 3, math.inf):
            for check in (False, True):
                lps.append(B.dense_lp(oracle, M, N, 21, max_pivots=budget, check_cycles=check))
    out = batch.solve(lps, keep_tableaux=True)
    refs = [B.oracle_answer(oracle, lp) for lp in lps]
    assert {r["n_pivots"] for r in refs} >= {0, 3} and "cycled" in {r["status"] for r in refs}
    for i, (lp, ref) in enumerate(zip(lps, refs)):
        B.check_lp(batch, i, out, ref, lp)


@pytest.mark.gpu
def test_history_rerun_only_for_the_lps_that_overflowed(gpu, oracle, monkeypatch):
    from yalps_amd.model import tableau_model
    cap = 8
    monkeypatch.setenv("YALPS_LPBATCH_HIST", str(cap))
    lps = []
    for name in ("Chvatal Cycling", "ChenhuaWANG22 2"):
        case = K.load(name)
        lps.append(B.model_lp(tableau_model(case["model"], sparse=True), dict(case["options"], checkCycles=True)))
    lps.append(B.dense_lp(oracle, 96, 80, 9, check_cycles=True))       # long, no cycle
    lps.append(B.dense_lp(oracle, 300, 280, 5, check_cycles=True))     # the same in the HBM form
    lps.append(B.dense_lp(oracle, 30, 30, 2, check_cycles=False))
    lps.append(B.dense_lp(oracle, 96, 80, 9, check_cycles=False))
    lps.append(B.dense_lp(oracle, 30, 30, 2, check_cycles=True, max_pivots=3))
    lps.append(B.dense_lp(oracle, 300, 280, 5, check_cycles=True, max_pivots=3))
    refs = [B.oracle_answer(oracle, lp) for lp in lps]
    b = gpu.LpBatch(0)
    try:
        out = b.solve(lps, keep_tableaux=True)
        for i, (lp, ref) in enumerate(zip(lps, refs)):
            B.check_lp(b, i, out, ref, lp)
        info = b.info()
    finally:
        b.close()
    rerun = set(info["rerun_lps"])
    # a phase holds at most `cap` pivots before the history is full: more than 2 * cap pivots must have overflowed,
    # at most `cap` pivots (or no checkCycles) cannot have
    must = {i for i, (lp, r) in enumerate(zip(lps, refs)) if lp[7] and r["n_pivots"] > 2 * cap}
    never = {i for i, (lp, r) in enumerate(zip(lps, refs)) if not lp[7] or r["n_pivots"] <= cap}
    assert {2, 3} <= must and {4, 5, 6, 7} <= never
    assert must <= rerun and not rerun & never, (sorted(rerun), sorted(must), sorted(never))
    assert info["reruns"] == len(info["rerun_lps"]) >= len(must)
    later = [k for k in info["kernels"] if k["pass"] > 0]
    assert later and all("check" in k["kernel"] and k["hist_cap"] == cap * 4 ** k["pass"] for k in later)
    assert sum(k["lps"] for k in later) == info["reruns"]
    assert refs[0]["status"] == "cycled"


@pytest.mark.gpu
def test_info_of_a_batch_with_thousands_of_reruns(gpu, oracle, monkeypatch):
    """The info text names every rerun LP, so it outgrows any fixed buffer: LpBatch.info asks again with the length returned."""
    monkeypatch.setenv("YALPS_LPBATCH_HIST", "1")
    lps = [B.dense_lp(oracle, 6, 6, 1 + s, check_cycles=True) for s in range(1500)]
    refs = [B.oracle_answer(oracle, lp) for lp in lps]
    b = gpu.LpBatch(0)
    try:
        out = b.solve(lps)
        for i in range(0, len(lps), 97):
            B.check_lp(b, i, out, refs[i], lps[i], tableau=False)
        info = b.info()
    finally:
        b.close()
    assert len(info["text"]) > 1 << 12 and info["text"].endswith("\n")
    assert info["reruns"] == len(info["rerun_lps"]) > 1000
    assert {i for i, r in enumerate(refs) if r["n_pivots"] > 2} <= set(info["rerun_lps"])


@pytest.mark.gpu
def test_handle_reuse_grows_and_shrinks(gpu, oracle):
    b = gpu.LpBatch(0)
    try:
        first = small_lps(oracle, 40)
        second = small_lps(oracle, 300)[::-1] + [B.dense_lp(oracle, 300, 280, 5), B.dense_lp(oracle, 130, 120, 6)]
        third = [B.dense_lp(oracle, 60, 50, 8), B.dense_lp(oracle, 300, 280, 7, max_pivots=40)]
        for lps in (first, second, third):
            out = b.solve(lps, keep_tableaux=True)
            assert len(out[0]) == len(lps)
            for i, lp in enumerate(lps):
                B.check_lp(b, i, out, B.oracle_answer(oracle, lp), lp)
            with pytest.raises(gpu.NativeError, match="no such LP"):
                b.solution(len(lps))
        b.solve(third)
        with pytest.raises(gpu.NativeError, match="keep_tableaux"):
            b.tableau(0)
        # a refused batch launches nothing and leaves no last solve behind
        with pytest.raises(gpu.NativeError, match="LP 1: .*above the batch limit"):
            b.solve([third[0], (1024, 513, *third[0][2:])])
    finally:
        b.close()


@pytest.mark.gpu
def test_solve_many_equals_solve_on_every_case(gpu):
    from yalps_amd import solve as S
    cases = [K.load(n) for n in K.names()]
    assert len(cases) == 46
    cases.insert(20, {"name": "large LP", "model": large_lp_model(), "options": dict(S.default_options), "expected": None})
    stats = {}
    got = S.solve_many([c["model"] for c in cases], [c["options"] for c in cases], stats)
    assert stats["batched"] + stats["milp"] + stats["large"] == 47 and stats["milp"] > 0 and stats["large"] == 1
    assert stats["launches"] >= 1
    for c, g in zip(cases, got):
        e = S.solve(c["model"], c["options"])
        assert same_solution(g, e), (c["name"], g, e)
        if c["expected"] is not None:
            assert K.valid_solution_and_status(g, c["expected"], c["model"], c["options"]), c["name"]
    assert got[20]["status"] == "optimal"
