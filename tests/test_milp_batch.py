"""Batches of MILPs (include/yalps_milpbatch.h, yalps_amd.solve.solve_many): libyalps_milpbatch.so's boundary and its kernels
by name, the lockstep branch-and-cut driver on the MILP records with the C oracle as its node evaluator, and solve_many's
routing, on the CPU; on the GPU the root pass and milp_node_kernel on every recorded node, every instantiation by name, the
whole solve against the records, the work queue over thousands of mixed trees, the history rerun, handle reuse and
solve_many against solve.  Comparisons are bit for bit: status, result, pivot counts, permutations, column 0 and whole
matrices by value bits or SHA-256.

The records' coverage is counted here (test_what_the_records_cover) and asserted, so a changed golden file shows."""
import os
import re

import numpy as np
import pytest

from tests import _bnc as BN
from tests import _cases as K
from tests import _golden as G
from tests import _lp_batch as LB
from tests import _milp_batch as MB
from tests import _milps as ML
from tests.test_lp_batch import large_lp_model, oracle_backend, oracle_batch_backend, same_solution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RECORDS = MB.batchable_records()
NODE_BATCHES = (1, 3, 32)

# kernel spelling -> (node size class, checkCycles, a seeded packing model (m, n, n_int, seed, density) whose nodes are of that class)
KERNELS = {
    "milp_node_kernel<256,lds>": (1, False, (60, 60, 6, 1, 0.6)),
    "milp_node_kernel<256,check,lds>": (2, True, (80, 70, 6, 1, 0.6)),
    "milp_node_kernel<1024,lds>": (3, False, (100, 100, 6, 3, 0.6)),
    "milp_node_kernel<1024,check,lds>": (3, True, (100, 100, 6, 3, 0.6)),
    "milp_node_kernel<1024>": (4, False, (150, 150, 8, 7, 0.3)),
    "milp_node_kernel<1024,check>": (4, True, (150, 150, 8, 7, 0.3)),
}
ROOT_KERNELS = {"lp_batch_kernel<256,lds>", "lp_batch_kernel<256,check,lds>", "lp_batch_kernel<1024,lds>",
                "lp_batch_kernel<1024,check,lds>", "lp_batch_kernel<1024>", "lp_batch_kernel<1024,check>"}
# the issue's shapes for the 256-lane classes and the 1024-lane LDS class, with the class their nodes fall in
PACKINGS = {(40, 40, 6): 0, (60, 60, 6): 1, (80, 70, 6): 2, (100, 100, 6): 3}
PACKING_SEEDS = {(40, 40, 6): 3, (60, 60, 6): 1, (80, 70, 6): 1, (100, 100, 6): 3}


def _label(rec):
    return ML.label(rec["family"], rec["seed"], rec["variant"])


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_milpbatch()
    return _native


@pytest.fixture(scope="module")
def roots(oracle):
    return [MB.Root(oracle, MB.record_model(r), r["options"]) for r in RECORDS]


# ---------------------------------------------------------------------------------------------------------- CPU

def test_what_the_records_cover():
    every = G.records("milp")
    assert len(every) == 72 and len(RECORDS) == 71
    assert [_label(r) for r in every if r not in RECORDS] == ["big-s0"]
    nodes = [(r, n) for r in RECORDS for n in r["nodes"]]
    assert len(nodes) == 880
    assert sum(bool(r["options"].get("checkCycles")) for r, _ in nodes) == 26
    assert sum(n["status"] == "optimal" for _, n in nodes) == 554 and sum(n["status"] == "infeasible" for _, n in nodes) == 326
    assert all(r["root"]["status"] == "optimal" for r in RECORDS) and sum(bool(r["nodes"]) for r in RECORDS) == 64
    classes = [LB.size_class(r["width"], r["height"] + len(n["cuts"])) for r, n in nodes]
    assert classes.count(0) == 866 and classes.count(4) == 14 and len(classes) == 880


def test_header_symbols_are_exported(nat):
    text = open(os.path.join(ROOT, "include", "yalps_milpbatch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text)) - {"yalps_milpbatch_eval_fn", "yalps_milpbatch_consumed_fn"}
    assert declared and all(s.startswith("yalps_milpbatch_") for s in declared), declared
    L = nat.milpbatch_lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, missing
    assert declared == set(nat.SYMBOLS_MILPBATCH)
    assert not set(nat.SYMBOLS_MILPBATCH) & (set(nat.SYMBOLS) | set(nat.SYMBOLS_LPBATCH))


def test_no_cpu_fallback(nat):
    from yalps_amd import build
    build.build_hip()
    if nat.lib().yalps_device_count() > 0:
        nat.MilpBatch(0).close()
        return
    with pytest.raises(nat.NativeError, match="no HIP device"):
        nat.MilpBatch(0)


def test_kernels_are_the_table_and_the_other_libraries_keep_theirs(nat):
    from yalps_amd import build
    ks = build.kernel_metadata(lib=build.LIB_MILPBATCH)
    spelt = {MB.spelling(s): md for s, md in ks.items()}
    assert len(spelt) == len(ks)
    assert set(spelt) == set(KERNELS) | ROOT_KERNELS, sorted(set(spelt) ^ (set(KERNELS) | ROOT_KERNELS))
    for name, md in spelt.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0, (name, md)
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (name, md["group_segment_fixed_size"])
    build.check_register_budgets(lib=build.LIB_MILPBATCH, min_resident=0)
    build.build_lpbatch()
    assert {LB.spelling(s) for s in build.kernel_metadata(lib=build.LIB_LPBATCH)} == ROOT_KERNELS
    build.build_hip()
    assert not [s for s in build.kernel_metadata() if "milp_node" in s or "lp_batch" in s]


def test_kernel_table_models_have_trees_of_their_class(oracle):
    for name, (cls, check, (m, n, k, seed, density)) in KERNELS.items():
        model = ML._packing(np.random.RandomState(seed), m, n, k, density=density)
        root, run = MB.oracle_tree(oracle, model, {"checkCycles": check, "maxIterations": 24})
        assert run is not None and 2 <= len(run["nodes"]) <= 24, name
        assert {LB.size_class(root.w, root.h + len(x["cuts"])) for x in run["nodes"]} == {cls}, name
    for shape, cls in PACKINGS.items():
        root, run = MB.oracle_tree(oracle, MB.packing_model(*shape, PACKING_SEEDS[shape]))
        assert 4 <= len(run["nodes"]) <= 16 and {LB.size_class(root.w, root.h + len(x["cuts"])) for x in run["nodes"]} == {cls}, shape


def _disagreements(recs, rts, out, nodes):
    return {_label(r): d for r, root, o, n in zip(recs, rts, out, nodes) for d in [MB.disagreement(r, root, o, n)] if d}


@pytest.mark.parametrize("node_batch", NODE_BATCHES)
def test_records_through_the_lockstep_driver_as_one_batch(nat, oracle, roots, node_batch):
    """Every batchable record in ONE milp_search: per model the nodes consumed, in order, are the record's nodes (cuts with
    value bits, initial and final tableau, status, result bits, pivots, basis), their number its iterations; the best
    tableau, status, result and the marshalled Solution (and solution_flip) are the record's."""
    out, nodes, ev, rounds = MB.run_search(nat, oracle, roots, node_batch)
    assert _disagreements(RECORDS, roots, out, nodes) == {}
    assert sum(o[6] for o in out) == 880 <= sum(o[7] for o in out) == ev.evaluated
    assert ev.calls == rounds >= 1
    if node_batch == 1:
        assert ev.evaluated == 880  # (nothing is evaluated ahead of its turn)


@pytest.mark.parametrize("node_batch", NODE_BATCHES)
def test_grouping_changes_nothing(nat, oracle, roots, node_batch):
    half = len(RECORDS) // 2
    for idx in (list(range(half)), list(range(half, len(RECORDS))), list(range(len(RECORDS)))[::-1]):
        recs, rts = [RECORDS[i] for i in idx], [roots[i] for i in idx]
        out, nodes, _, _ = MB.run_search(nat, oracle, rts, node_batch)
        assert _disagreements(recs, rts, out, nodes) == {}


@pytest.mark.parametrize("mutant", ["permuted", "wrong_model"])
def test_the_record_comparison_rejects_a_grouping_bug(nat, oracle, roots, mutant):
    """An evaluator that hands results back in another order, or a node's result to another model, is what a lockstep driver
    can get wrong: the comparison of test_records_through_the_lockstep_driver_as_one_batch must fail on it."""
    out, nodes, _, _ = MB.run_search(nat, oracle, roots, 3, mutant)
    assert _disagreements(RECORDS, roots, out, nodes), mutant


def test_solve_many_routing_with_the_oracle(nat, oracle):
    from yalps_amd import solve as S
    from yalps_amd.model import tableau_model
    cases = [K.load(n) for n in K.names()]
    assert len(cases) == 46
    cases.insert(20, {"name": "large LP", "model": large_lp_model(), "options": dict(S.default_options)})
    models, opts = [c["model"] for c in cases], [c["options"] for c in cases]
    tms = [tableau_model(m, sparse=True) for m in models]
    merged = [MB.options({k: v for k, v in (o or {}).items() if v is not None}) for o in opts]
    fits = [MB.batchable(tm.tableau.width, tm.tableau.height, len(tm.integers), o) and bool(tm.integers) for tm, o in zip(tms, merged)]
    milp = sum(1 for tm in tms if tm.integers)
    assert milp == 15 and sum(fits) == 11
    one = oracle_backend(oracle)
    routed, log = [], []

    def solve_one(model, options):
        routed.append(model)
        return S._solve_with(one, model, options)

    expected = [S._solve_with(one, m, o) for m, o in zip(models, opts)]
    for node_batch in NODE_BATCHES:
        del routed[:], log[:]
        stats = {}
        got = S._solve_many_with(oracle_batch_backend(oracle), solve_one, models, opts, stats,
                                 milp_backend=MB.oracle_milp_backend(nat, oracle, node_batch, log))
        for c, g, e in zip(cases, got, expected):
            assert same_solution(g, e), (c["name"], g["status"], e["status"])
        sequential = sum(run["iterations"] for (root, run) in (MB.oracle_tree(oracle, None, o, tabmod=tableau_model(m))
                                                              for m, o, f in zip(models, merged, fits) if f) if run is not None)
        assert stats["milp"] == milp and stats["milp_batched"] == 11 and stats["large"] == 1
        assert stats["batched"] + stats["milp"] + stats["large"] == 47
        assert stats["nodes_used"] == sequential > 0 and stats["nodes_evaluated"] >= stats["nodes_used"] and stats["node_rounds"] >= 1
        assert len(log) == 1 and len(log[0][0]) == 11
        names = [c["name"] for c, m in zip(cases, models) if any(m is r for r in routed)]
        assert {"Fancy Stock Cutting Problem", "Large Farm MIP", "Monster 2", "Vendor Selection", "large LP"} <= set(names), names
        assert len(routed) == milp - 11 + 1
    # without a MILP backend nothing changes: the three keys, every model with integers to solve_one
    stats = {}
    S._solve_many_with(oracle_batch_backend(oracle), solve_one, models[:12], opts[:12], stats)
    assert set(stats) == {"batched", "milp", "large"}


def test_argument_errors_name_the_model_or_node_before_any_device_call(nat):
    good = MB.milp_of(ML.make("ties", 0)[0])
    w, h = good[0], good[1]
    nat.PackedMilps([good, good]).validate()
    with pytest.raises(nat.NativeError, match="model 1: .*integer variable %d out of range" % w):
        nat.PackedMilps([good, (*good[:5], [1, w], *good[6:])]).validate()
    with pytest.raises(nat.NativeError, match="model 1: .*integer variable 0 out of range"):
        nat.PackedMilps([good, (*good[:5], [0], *good[6:])]).validate()
    tall = (1024, 500, *good[2:5], list(range(1, 14)), *good[6:])  # 500 + 26 rows of 1024 doubles: above 4 MiB
    with pytest.raises(nat.NativeError, match="model 2: .*above the batch limit"):
        nat.PackedMilps([good, good, tall]).validate()
    with pytest.raises(nat.NativeError, match="node_batch"):
        nat.PackedMilps([good]).validate(node_batch=0)
    p = nat.PackedMilps([good, good])
    p.int_offsets[2] = p.int_offsets[1] - 1
    with pytest.raises(nat.NativeError, match="model 1: .*integer offsets decrease"):
        p.validate()
    # nodes
    rw, rh = [w, 1024], [h, 511]
    cut = [(1, 1, 2.0)]
    nat.milp_validate_nodes(rw, rh, [0, 0, 1], [cut, cut + cut, cut])
    with pytest.raises(nat.NativeError, match="node 2: .*root index 2 out of range"):
        nat.milp_validate_nodes(rw, rh, [0, 1, 2], [cut, cut, cut])
    with pytest.raises(nat.NativeError, match="node 1: .*root index -1 out of range"):
        nat.milp_validate_nodes(rw, rh, [0, -1], [cut, cut])
    with pytest.raises(nat.NativeError, match="node 1: .*above the batch limit"):
        nat.milp_validate_nodes(rw, rh, [0, 1], [cut, cut + cut])  # 513 rows of 1024 doubles
    with pytest.raises(nat.NativeError, match="node 1: .*cut on variable %d out of range" % w):
        nat.milp_validate_nodes(rw, rh, [0, 0], [cut, [(1, w, 2.0)]])
    with pytest.raises(nat.NativeError, match="node 0: .*cut on variable 0 out of range"):
        nat.milp_validate_nodes(rw, rh, [0, 0], [[(-1, 0, 2.0)], cut])
    off, sg, vr, vl = nat._pack_cuts([cut, cut, cut])
    off[2] = 0
    with pytest.raises(nat.NativeError, match="node 1: .*cut offsets decrease"):
        nat.milp_validate_nodes(rw, rh, [0, 0, 0], (off, sg, vr, vl))


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu(nat):
    assert nat.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return nat


@pytest.fixture(scope="module")
def batch(gpu):
    b = gpu.MilpBatch(0)
    yield b
    b.close()


def record_milps():
    return [MB.milp_of(MB.record_model(r), r["options"]) for r in RECORDS]


def check_roots(batch, out, recs):
    statuses, results, pivots = out
    for i, r in enumerate(recs):
        assert (statuses[i], BN.hexd(results[i]), int(pivots[i])) == (r["root"]["status"], r["root"]["result"], r["root"]["n_pivots"]), _label(r)
        col0, pos, var, m = batch.root(i, matrix=True)
        assert G.sha256(m) == r["root"]["final_sha256"], _label(r)
        assert MB.same_words(col0, m[::r["width"]]), _label(r)


def check_record_nodes(batch, recs, which, max_pivots=None):
    """All nodes of recs[which] in one nodes() call on the last root pass; every key a record holds of a node."""
    idx, cuts, want = [], [], []
    for i in which:
        for n in recs[i]["nodes"]:
            idx.append(i), cuts.append(MB.cuts_of(n)), want.append((recs[i], n))
    statuses, results, pivots, heights = batch.nodes(idx, cuts, max_pivots=max_pivots, keep_tableaux=True)
    for k, (r, n) in enumerate(want):
        tag = (_label(r), k)
        assert heights[k] == r["height"] + len(n["cuts"]), tag
        m = batch.node_tableau(k)
        col0, pos, var = batch.node(k)
        assert MB.same_words(col0, m[::r["width"]]), tag
        if max_pivots is not None:
            assert (statuses[k], int(pivots[k])) == ("cycled", 0) and G.sha256(m) == n["init_sha256"], tag
            w, h0 = r["width"], r["height"]
            assert np.array_equal(pos[w + h0:], np.arange(w + h0, w + heights[k])) and np.array_equal(var[w + h0:], pos[w + h0:]), tag
            continue
        assert (statuses[k], BN.hexd(results[k]), int(pivots[k])) == (n["status"], n["result"], n["n_pivots"]), tag
        assert BN.sha(pos, var) == n["perm_sha256"] and G.sha256(m) == n["final_sha256"], tag
    return len(want)


@pytest.mark.gpu
def test_node_kernel_on_every_recorded_node(batch):
    milps = record_milps()
    check_roots(batch, batch.roots([MB.lp_of(m) for m in milps]), RECORDS)
    assert check_record_nodes(batch, RECORDS, range(len(RECORDS))) == 880
    info = batch.info()
    first = [k for k in info["kernels"] if k["pass"] == 0]
    assert sum(k["nodes"] for k in first) == 880 and len(first) == len({(k["class"], "check" in k["kernel"]) for k in first})
    mid = {bool(r["options"].get("checkCycles")): len(r["nodes"]) for r in RECORDS if r["family"] == "mid"}
    assert {k["class"] for k in first} == {0, 4} and {"check" in k["kernel"]: k["nodes"] for k in first if k["class"] == 4} == mid
    assert sum(mid.values()) == 14
    # a budget of 0: every node's initial tableau, and so the sign of the zeros applyCuts writes
    assert check_record_nodes(batch, RECORDS, range(len(RECORDS)), max_pivots=0.0) == 880


def node_launches(info):
    return sorted((k["kernel"], k["class"]) for k in info["kernels"] if k["kernel"].startswith("milp_node_kernel"))


def check_against_oracle_tree(batch, i, out, root, run):
    statuses, results, used, evaluated, _ = out
    assert (statuses[i], BN.hexd(results[i]), int(used[i])) == (run["status"], BN.hexd(run["result"]), run["iterations"]), i
    assert used[i] <= evaluated[i]
    height, col0, pos, var = batch.solution(i)
    assert (height, BN.sha(col0), BN.sha(pos, var)) == (run["best_height"], run["best_col0"], run["best_perm"]), i


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_every_instantiation_by_name(batch, oracle, name):
    cls, check, (m, n, k, seed, density) = KERNELS[name]
    extra = {"checkCycles": check, "maxIterations": 24}
    models = [ML._packing(np.random.RandomState(s), m, n, k, density=density) for s in (seed, seed + 1)]
    root, run = MB.oracle_tree(oracle, models[0], extra)
    # node by node: the whole tree of the first model against the scalar branch and cut's nodes
    batch.roots([MB.lp_of(MB.milp_of(models[0], extra))])
    cuts = [MB.cuts_of(x) for x in run["nodes"]]
    statuses, results, pivots, heights = batch.nodes([0] * len(cuts), cuts, keep_tableaux=True)
    assert node_launches(batch.info()) == [(name, cls)]
    for j, x in enumerate(run["nodes"]):
        assert (statuses[j], BN.hexd(results[j]), int(pivots[j])) == (x["status"], x["result"], x["n_pivots"]), (name, j)
        _, pos, var = batch.node(j)
        assert BN.sha(pos, var) == x["perm_sha256"] and G.sha256(batch.node_tableau(j)) == x["final_sha256"], (name, j)
    # the whole solve
    out = batch.solve([MB.milp_of(mod, extra) for mod in models], node_batch=3)
    for i, mod in enumerate(models):
        r, t = MB.oracle_tree(oracle, mod, extra)
        if t is not None:
            check_against_oracle_tree(batch, i, out, r, t)
    assert (name, cls) in node_launches(batch.info())


@pytest.mark.gpu
@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("shape", sorted(PACKINGS))
def test_packing_trees_of_every_lds_class(batch, oracle, shape, check):
    extra = {"checkCycles": check}
    model = MB.packing_model(*shape, PACKING_SEEDS[shape])
    root, run = MB.oracle_tree(oracle, model, extra)
    out = batch.solve([MB.milp_of(model, extra)], node_batch=2)
    check_against_oracle_tree(batch, 0, out, root, run)
    lanes = 1024 if PACKINGS[shape] == 3 else 256
    assert set(node_launches(batch.info())) == {("milp_node_kernel<%d%s,lds>" % (lanes, ",check" if check else ""), PACKINGS[shape])}


def check_solve_against_records(batch, out, recs):
    statuses, results, used, evaluated, call = out
    for i, r in enumerate(recs):
        tag = _label(r)
        assert (statuses[i], BN.hexd(results[i]), int(used[i])) == (r["best"]["status"], r["best"]["result"], r["iterations"]), tag
        assert used[i] <= evaluated[i], tag
        height, col0, pos, var = batch.solution(i)
        assert (height, BN.sha(col0), BN.sha(pos, var)) == (r["best"]["height"], r["best"]["col0_sha256"], r["best"]["perm_sha256"]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("node_batch", NODE_BATCHES)
def test_whole_solve_equals_the_records(batch, roots, node_batch):
    out = batch.solve(record_milps(), node_batch=node_batch)
    check_solve_against_records(batch, out, RECORDS)
    for i, (r, root) in enumerate(zip(RECORDS, roots)):
        sol = MB.view_solution(root, root.opt, out[0][i], float(out[1][i]), *batch.solution(i))
        assert MB.marshal(sol) == r["solution"], _label(r)
    info = batch.info()
    assert info["rounds"] == out[4]["rounds"] >= 1 and info["launches"] == out[4]["launches"] == len(info["kernels"])
    assert sum(out[2]) == 880 and (node_batch > 1 or sum(out[3]) == 880)


def mixed_models(count):
    """`count` small trees over fresh seeds, every 75th place taken by a model whose nodes are of class 1, 2, 3 or 4."""
    small = MB.small_family_models(count)
    larger = [((60, 60, 6), 0.6, {}), ((80, 70, 6), 0.6, {}), ((100, 100, 6), 0.6, {}), ((150, 150, 8), 0.3, {"maxIterations": 24})]
    out = []
    for k, (model, opt) in enumerate(small):
        if k % 75 == 0:
            (m, n, ki), density, extra = larger[(k // 75) % 4]
            model, opt = ML._packing(np.random.RandomState(500 + k), m, n, ki, density=density), extra
        out.append((model, opt))
    return out


@pytest.mark.gpu
def test_queue_and_mixing_over_thousands_of_trees(batch):
    from yalps_amd import solve as S
    from yalps_amd.model import tableau_model
    mixed = mixed_models(3000)
    milps = [MB.milp_of(m, o) for m, o in mixed]
    out = batch.solve(milps, node_batch=4)
    info = batch.info()
    assert {k["class"] for k in info["kernels"] if k["kernel"].startswith("milp_node")} == {0, 1, 2, 3, 4}
    assert max(k["nodes"] for k in info["kernels"] if "nodes" in k) > max(k["grid"] for k in info["kernels"])
    sols = [batch.solution(i) for i in range(len(milps))]
    sample = np.random.default_rng(13).choice(len(mixed), 200, replace=False)
    for i in sample:
        model, opt = mixed[i]
        tm = tableau_model(model)
        view_root = type("R", (), dict(w=tm.tableau.width, tm=tm))
        got = MB.view_solution(view_root, MB.options(opt), out[0][i], float(out[1][i]), *sols[i])
        assert same_solution(got, S.solve(model, opt)), i
    order = np.random.default_rng(17).permutation(len(milps))
    again = batch.solve([milps[j] for j in order], node_batch=4)
    for i, j in enumerate(order):
        assert again[0][i] == out[0][j] and G.same_number(float(again[1][i]), float(out[1][j])) and again[2][i] == out[2][j], (i, j)
        a, b = batch.solution(i), sols[j]
        assert a[0] == b[0] and all(MB.same_words(x, y) for x, y in zip(a[1:], b[1:])), (i, j)


@pytest.mark.gpu
def test_history_rerun_of_nodes(gpu, monkeypatch):
    monkeypatch.setenv("YALPS_MILPBATCH_HIST", "2")
    recs = [r for r in RECORDS if r["family"] == "cycles" or _label(r) == "mid-s1"]
    assert len(recs) == 4 and all(r["options"]["checkCycles"] for r in recs)
    b = gpu.MilpBatch(0)
    try:
        check_roots(b, b.roots([MB.lp_of(MB.milp_of(MB.record_model(r), r["options"])) for r in recs]), recs)
        assert check_record_nodes(b, recs, range(len(recs))) == sum(len(r["nodes"]) for r in recs) == 26
        info = b.info()
        pivots = [n["n_pivots"] for r in recs for n in r["nodes"]]
        must = {k for k, p in enumerate(pivots) if p > 4}   # a phase holds at most 2 pivots before the history is full
        never = {k for k, p in enumerate(pivots) if p <= 2}
        assert must and must <= set(info["rerun_nodes"]) and not never & set(info["rerun_nodes"]), (info["rerun_nodes"], pivots)
        later = [k for k in info["kernels"] if k["pass"] > 0]
        assert later and all("check" in k["kernel"] and k["hist_cap"] == 2 * 4 ** k["pass"] for k in later)
        # the whole solve under the same hook
        check_solve_against_records(b, b.solve([MB.milp_of(MB.record_model(r), r["options"]) for r in recs], node_batch=3), recs)
        assert b.info()["reruns"] > 0 and all(isinstance(x, tuple) for x in b.info()["rerun_nodes"])
    finally:
        b.close()


@pytest.mark.gpu
def test_handle_reuse(gpu):
    b = gpu.MilpBatch(0)
    try:
        first = record_milps()[:30]
        second = [MB.milp_of(m, o) for m, o in mixed_models(160)]
        third = [MB.milp_of(MB.packing_model(100, 100, 6, 3)), MB.milp_of(ML.make("mid", 0)[0], ML.make("mid", 0)[1])]
        runs = []
        for milps in (first, second, third, first):
            out = b.solve(milps, node_batch=3)
            runs.append((out[0], [BN.hexd(x) for x in out[1]], list(out[2]), [tuple(BN.sha(a) for a in b.solution(i)[1:]) for i in range(len(milps))]))
            with pytest.raises(gpu.NativeError, match="no such model"):
                b.solution(len(milps))
        assert runs[0] == runs[3]
        check_solve_against_records(b, out, RECORDS[:30])
        with pytest.raises(gpu.NativeError, match="model 1: .*out of range"):
            b.solve([first[0], (*first[0][:5], [first[0][0]], *first[0][6:])])
        with pytest.raises(gpu.NativeError, match="no such model"):
            b.solution(0)  # (a refused batch leaves no last solve behind)
    finally:
        b.close()


@pytest.mark.gpu
def test_solve_many_equals_solve_on_every_case(gpu):
    from yalps_amd import solve as S
    cases = [K.load(n) for n in K.names()]
    cases.insert(20, {"name": "large LP", "model": large_lp_model(), "options": dict(S.default_options)})
    stats = {}
    got = S.solve_many([c["model"] for c in cases], [c["options"] for c in cases], stats)
    assert stats["batched"] + stats["milp"] + stats["large"] == 47 and stats["milp"] == 15 and stats["milp_batched"] == 11
    assert stats["node_rounds"] >= 1 and 0 < stats["nodes_used"] <= stats["nodes_evaluated"]
    for c, g in zip(cases, got):
        assert same_solution(g, S.solve(c["model"], c["options"])), (c["name"], g)


@pytest.mark.gpu
def test_solve_many_on_milps_mixed_with_lps(gpu):
    from yalps_amd import solve as S
    milps = MB.small_family_models(300, first_seed=400)
    rng = np.random.RandomState(9)
    models, opts = [], []
    for k, (model, opt) in enumerate(milps):
        lp = ML._packing(np.random.RandomState(2000 + k), int(rng.randint(3, 12)), int(rng.randint(3, 12)), 0)
        assert "integers" not in lp
        models += [model, lp]
        opts += [opt, {}]
    stats = {}
    got = S.solve_many(models, opts, stats)
    assert stats["batched"] == 300 and stats["milp"] == stats["milp_batched"] == 300
    for k, (m, o, g) in enumerate(zip(models, opts, got)):
        assert same_solution(g, S.solve(m, o)), k
