"""Whole branch-and-cut trees on the device (include/yalps_milptree.h, yalps_amd.solve.solve_many(milp_search="device")).

On the CPU: libyalps_milptree.so's boundary and its kernels by name; the search rules of milp_tree_rules.cuh through
yalps_milptree_search -- on the MILP records with the C oracle as evaluator, against the lockstep driver
(yalps_milpbatch_search at node_batch 1) with a synthetic evaluator, the heap against Python's heapq, the arena and its
reruns, and four mutants of a Python restatement; solve_many's routing with oracle-driven backends.
On the GPU: milp_tree_kernel on the records with its trace, every instantiation by name, one workgroup walking many trees,
the reruns, the shapes at the class bounds, thousands of mixed trees against MilpBatch, handle and stream, solve_many.
Comparisons are bit for bit."""
import heapq
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _bnc as BN
from tests import _cases as K
from tests import _golden as G
from tests import _lp_batch as LB
from tests import _milp_batch as MB
from tests import _milp_tree as MT
from tests import _milps as ML
from tests.test_lp_batch import large_lp_model, oracle_backend, oracle_batch_backend, same_solution
from tests.test_milp_batch import KERNELS, ROOT_KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = MB.batchable_records()
TREE_KERNELS = {k.replace("milp_node_kernel", "milp_tree_kernel"): v for k, v in KERNELS.items()}
NAN, INF = math.nan, math.inf


def _label(rec):
    return ML.label(rec["family"], rec["seed"], rec["variant"])


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_milptree()
    build.build_milpbatch()
    return _native


@pytest.fixture(scope="module")
def roots(oracle):
    return [MB.Root(oracle, MB.record_model(r), r["options"]) for r in RECORDS]


# ---------------------------------------------------------------------------------------------------------- CPU

def test_header_symbols_are_exported(nat):
    text = open(os.path.join(ROOT, "include", "yalps_milptree.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text)) - {"yalps_milptree_eval_fn", "yalps_milptree_consumed_fn"}
    assert declared and all(s.startswith("yalps_milptree_") for s in declared), declared
    L = nat.milptree_lib()
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert declared == set(nat.SYMBOLS_MILPTREE)
    others = set(nat.SYMBOLS) | set(nat.SYMBOLS_LPBATCH) | set(nat.SYMBOLS_MILPBATCH) | set(nat.SYMBOLS_LPVAR) | \
        set(nat.SYMBOLS_LPSENS) | set(nat.SYMBOLS_LPWARM)
    assert not set(nat.SYMBOLS_MILPTREE) & others


def test_kernels_are_the_table_and_milpbatch_keeps_its_own(nat):
    from yalps_amd import build
    ks = build.kernel_metadata(lib=build.LIB_MILPTREE)
    spelt = {MT.spelling(s): md for s, md in ks.items()}
    assert len(spelt) == len(ks)
    assert set(spelt) == set(TREE_KERNELS) | ROOT_KERNELS, sorted(set(spelt) ^ (set(TREE_KERNELS) | ROOT_KERNELS))
    for name, md in spelt.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0, (name, md)
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (name, md["group_segment_fixed_size"])
    build.check_register_budgets(lib=build.LIB_MILPTREE, min_resident=0)
    assert "milp_tree_kernel" in build.NO_SCRATCH
    assert {MB.spelling(s) for s in build.kernel_metadata(lib=build.LIB_MILPBATCH)} == set(KERNELS) | ROOT_KERNELS
    assert not [d for d in build.HIP_DEPS if "milp_tree" in d]


def test_no_cpu_fallback_and_argument_errors_name_the_model(nat):
    from yalps_amd import build
    build.build_hip()
    if nat.lib().yalps_device_count() > 0:
        nat.MilpTree(0).close()
    else:
        with pytest.raises(nat.NativeError, match="no HIP device"):
            nat.MilpTree(0)
    good = MB.milp_of(ML.make("ties", 0)[0])
    w = good[0]
    nat.milptree_validate(nat.PackedMilps([good, good]))
    with pytest.raises(nat.NativeError, match="model 1: .*integer variable %d out of range" % w):
        nat.milptree_validate(nat.PackedMilps([good, (*good[:5], [1, w], *good[6:])]))
    tall = (1024, 500, *good[2:5], list(range(1, 14)), *good[6:])
    with pytest.raises(nat.NativeError, match="model 2: .*above the batch limit"):
        nat.milptree_validate(nat.PackedMilps([good, good, tall]))
    with pytest.raises(nat.NativeError, match="model 1: .*timeout"):
        nat.milptree_validate(nat.PackedMilps([good, (*good[:7], dict(good[7], timeout=5.0))]))
    nat.milptree_validate(nat.PackedMilps([(*good[:7], dict(good[7], timeout=t)) for t in (0, -1.0, INF)]))


def _disagreements(recs, rts, out, nodes):
    return {_label(r): d for r, root, o, n in zip(recs, rts, out, nodes) for d in [MB.disagreement(r, root, o, n)] if d}


def test_records_through_the_host_search(nat, oracle, roots):
    """Every batchable record (71 models, 880 nodes) in one milp_tree_search: MB.disagreement compares the consumed nodes in
    order (eval bits, cuts, tableaux, status, result bits, pivots), their number, the best tableau, status, result, Solution."""
    assert len(RECORDS) == 71 and sum(len(r["nodes"]) for r in RECORDS) == 880
    out, nodes, ev, reruns = MT.run_tree_search(nat, oracle, roots)
    assert _disagreements(RECORDS, roots, out, nodes) == {}
    assert sum(o[6] for o in out) == 880 == ev.evaluated and reruns == 0
    half = len(RECORDS) // 2
    for idx in (list(range(half)), list(range(half, len(RECORDS))), list(range(len(RECORDS)))[::-1]):
        recs, rts = [RECORDS[i] for i in idx], [roots[i] for i in idx]
        out, nodes, _, _ = MT.run_tree_search(nat, oracle, rts)
        assert _disagreements(recs, rts, out, nodes) == {}


def _check_both(nat, trees):
    (a, seq_a), (b, seq_b) = MT.both_drivers(nat, trees)
    assert MT.same_outputs(a, b) is None, MT.same_outputs(a, b)
    assert seq_a == seq_b
    return a, seq_a


def test_differential_against_the_lockstep_driver(nat):
    small = MT.synthetic_trees(240, seed0=1, opt={"maxIterations": 400})
    out, seq = _check_both(nat, small)
    large = MT.synthetic_trees(24, seed0=2, p_frac=0.62, opt={"maxIterations": 3000})
    out2, seq2 = _check_both(nat, large)
    sizes = [len(s) for s in seq + seq2]
    assert len(sizes) == 264 and max(sizes) >= 2000 and min(sizes) == 0 and sum(s > 50 for s in sizes) >= 10, (sum(sizes), max(sizes))
    statuses = {o[0] for o in out + out2}
    assert {"optimal", "infeasible", "timedout"} <= statuses, statuses
    assert any(MT.bits(o[1]) == BN.hexd(-0.0) for o in out + out2)
    evals = [e for s in seq + seq2 for e, _ in s]
    assert len(set(evals)) <= 12  # (heavy ties: every order among equals is heapq's)


@pytest.mark.parametrize("max_iter", [0, 1, 2.5, NAN, INF])
@pytest.mark.parametrize("tolerance", [0, 0.5, NAN, INF])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_differential_on_the_option_edges(nat, max_iter, tolerance, sign):
    opt = {"maxIterations": max_iter, "tolerance": tolerance}
    trees = MT.synthetic_trees(12, seed0=3, opt=opt, sign=sign)
    trees += [MT.Synthetic(900 + k, 4, opt=dict(opt, timeout=t), sign=sign) for k, t in enumerate((0, -5.0))]
    _check_both(nat, trees)


def test_differential_on_the_root_edges(nat):
    trees = [MT.Synthetic(50, 3, root_status="infeasible", root_result=NAN), MT.Synthetic(51, 3, root_status="unbounded", root_result=2.0),
             MT.Synthetic(52, 3, root_status="cycled", root_result=NAN), MT.Synthetic(53, 5, root_result=NAN),
             MT.Synthetic(54, 5, root_result=INF), MT.Synthetic(55, 5, root_result=-INF), MT.Synthetic(56, 5, root_result=-0.0)]
    integral = MT.Synthetic(57, 4)
    integral.col0 = np.round(integral.col0)
    zero = MT.Synthetic(58, 1)
    zero.ints = []
    nan_precision = MT.Synthetic(59, 4, opt={"precision": NAN, "maxIterations": 50})
    out, seq = _check_both(nat, trees + [integral, zero, nan_precision] + MT.synthetic_trees(5, seed0=4))
    assert [o[0] for o in out[:3]] == ["infeasible", "unbounded", "cycled"] and seq[7] == [] and seq[8] == []
    assert out[7][0] == "optimal" and out[8][0] == "optimal"


def test_heap_rules_against_heapq(nat):
    """A tree whose every node is fractional pops and pushes as heapq does: the consumed evaluations of the search equal those
    of a heapq of (eval, push order is NOT a key) items, for heaps that pass through sizes 0 .. 16 and beyond."""
    class Item:
        def __init__(self, ev, cuts):
            self.eval, self.cuts = ev, cuts

        def __lt__(self, other):
            return self.eval < other.eval

    reached = set()
    for seed in range(12):
        wide = seed % 2  # (six integers and fewer integral nodes: heaps beyond 16)
        t = MT.Synthetic(7000 + seed, 6 if wide else 3, p_frac=0.9 if wide else 0.8, opt={"maxIterations": 40})
        log = []
        out, _ = nat.milp_tree_search([t.packed()], MT.synthetic_evaluator([t], log))
        # replay with heapq over what the evaluator returns
        variable, value, frac = MT._mfv(t.w, t.col0, t.pos, t.ints, ())
        if frac <= t.opt["precision"]:
            assert log == []
            continue
        heap, seq, best, it = [], [], INF, 0
        heapq.heappush(heap, Item(t.result, [(-1, variable, float(np.ceil(value)))]))
        heapq.heappush(heap, Item(t.result, [(1, variable, float(math.floor(value)))]))
        sizes = set()
        while it < 40 and heap and best >= t.result:
            sizes.add(len(heap))
            br = heapq.heappop(heap)
            if br.eval > best:
                break
            seq.append((0, tuple((s, v, BN.hexd(x)) for s, v, x in br.cuts)))
            st, res, c0, p, _ = t.node(br.cuts)
            if st == "optimal" and res < best:
                variable, value, frac = MT._mfv(t.w, c0, p, t.ints, ())
                if frac <= t.opt["precision"]:
                    best = res
                else:
                    up = [c for c in br.cuts if not (c[1] == variable and c[0] < 0)] + [(-1, variable, float(np.ceil(value)))]
                    lo = [c for c in br.cuts if not (c[1] == variable and c[0] >= 0)] + [(1, variable, float(math.floor(value)))]
                    heapq.heappush(heap, Item(res, up))
                    heapq.heappush(heap, Item(res, lo))
            it += 1
        assert log == seq, seed
        reached |= sizes
    # (the library's own heap, in whole searches, popped at each of these sizes)
    assert {1, 2, 3, 7, 8, 15, 16} <= reached, sorted(reached)
    # the raw push / pop order on sizes 0, 1, 2, 3, 7, 8, 15, 16: the restatement the mutants are cut from is heapq's
    rng = np.random.RandomState(5)
    for size in (0, 1, 2, 3, 7, 8, 15, 16):
        for _ in range(20):
            a, b, order = [], [], []
            for k in range(size + 8):
                it = MT._Item(float(rng.randint(0, 3)) * (-0.0 if rng.randint(2) else 1.0), k)
                MT._push(a, it)
                heapq.heappush(b, Item(it.eval, k))
                if len(a) > size:
                    order.append((MT._pop(a, ()).cuts, heapq.heappop(b).cuts))
            while a:
                order.append((MT._pop(a, ()).cuts, heapq.heappop(b).cuts))
            assert all(x == y for x, y in order)


def _python_runs(trees, rules=frozenset()):
    return [MT.python_search(t.packed(), t.node, rules) for t in trees]


def test_python_restatement_equals_the_search_and_mutants_are_rejected(nat, oracle, roots):
    trees = MT.synthetic_trees(80, seed0=6, opt={"maxIterations": 300})
    (out, seq), _ = MT.both_drivers(nat, trees)
    want = [(o[0], MT.bits(o[1]), s) for o, s in zip(out, seq)]
    assert _python_runs(trees) == want
    rec_want = None
    for mutant in MT.MUTANTS:
        rejected = _python_runs(trees, frozenset([mutant])) != want
        if not rejected:  # ... or by a record
            if rec_want is None:
                rec_want = [(r["best"]["status"], [n["eval"] for n in r["nodes"]], [n["cuts"] for n in r["nodes"]]) for r in RECORDS]
            got = []
            for r in roots:
                ev = MB.OracleEvaluator(oracle, [r])
                st, _, s = MT.python_search(r.packed(), lambda cuts: ev.one(0, cuts), frozenset([mutant]))
                got.append((st, [e for e, _ in s], [[list(c) for c in cuts] for _, cuts in s]))
            rejected = got != rec_want
        assert rejected, mutant


def test_arena(nat):
    trees = MT.synthetic_trees(60, seed0=8, p_frac=0.6, opt={"maxIterations": 200})
    roots_ = [t.packed() for t in trees]
    ev = MT.synthetic_evaluator(trees)
    free, _ = nat.milp_tree_search(roots_, ev, arena=4096)
    # the largest frontier of every tree, by the Python restatement's heap: capacity exactly reached is no overflow
    peaks = []
    for t in trees:
        peak = [0]
        orig_push = MT._push

        def counting(heap, item, peak=peak):
            orig_push(heap, item)
            peak[0] = max(peak[0], len(heap))
        MT._push = counting
        try:
            MT.python_search(t.packed(), t.node)
        finally:
            MT._push = orig_push
        peaks.append(peak[0])
    assert max(peaks) >= 16
    for i in np.argsort(peaks)[-6:]:
        t, peak = trees[i], peaks[i]
        if peak < 2:
            continue
        exact, r0 = nat.milp_tree_search([t.packed()], MT.synthetic_evaluator([t]), arena=peak, arena_max=peak)
        assert r0 == 0 and MT.same_outputs(exact, [free[i]]) is None
        if peak > 2:
            under, r1 = nat.milp_tree_search([t.packed()], MT.synthetic_evaluator([t]), arena=peak - 1, arena_max=peak - 1)
            assert under[0][0] == "overflow" and math.isnan(under[0][1]) and r1 == 0
            assert under[0][2] == t.h and MB.same_words(under[0][3], t.col0)  # (nothing of the lost tree is reported)
    # reruns at x 4 give the same trees; slots are reused (a 200-node tree in an arena of its peak)
    seq = []
    again, reruns = nat.milp_tree_search(roots_, ev, arena=2, consumed=lambda m, e, c: seq.append(m))
    assert reruns > 0 and MT.same_outputs(again, free) is None
    assert sum(o[6] for o in free) == len(seq) > 4 * max(peaks)
    capped, _ = nat.milp_tree_search(roots_, ev, arena=2, arena_max=8)
    for o, f, peak in zip(capped, free, peaks):
        assert (o[0] == "overflow") == (peak > 8), (o[0], peak)
        assert o[0] == "overflow" or MT.same_outputs([o], [f]) is None
    with pytest.raises(nat.NativeError, match="arena"):
        nat.milp_tree_search(roots_[:1], ev, arena=1)


def test_solve_many_routing_with_the_oracle(nat, oracle):
    from yalps_amd import solve as S
    cases = [K.load(n) for n in K.names()]
    cases.insert(20, {"name": "large LP", "model": large_lp_model(), "options": dict(S.default_options)})
    models, opts = [c["model"] for c in cases], [c["options"] for c in cases]
    one = oracle_backend(oracle)
    expected = [S._solve_with(one, m, o) for m, o in zip(models, opts)]
    solve_one = lambda model, options: S._solve_with(one, model, options)
    host = {}
    S._solve_many_with(oracle_batch_backend(oracle), solve_one, models, opts, host, milp_backend=MB.oracle_milp_backend(nat, oracle, 4))

    class OracleTree:
        """MilpTree's face over the host search: what milptree_solve calls of a handle."""
        def __init__(self, arena_max):
            self.arena_max = arena_max

        def solve(self, packed):
            roots_ = [MB.Root(oracle, None, opt, tabmod=tm) for tm, opt in self.items]
            self.out, self.reruns = nat.milp_tree_search([r.packed() for r in roots_], MB.OracleEvaluator(oracle, roots_), arena=2,
                                                         arena_max=self.arena_max)
            return ([o[0] for o in self.out], [o[1] for o in self.out], np.array([o[6] for o in self.out]), None,
                    {"launches": 1, "reruns": self.reruns})

        def solution(self, i):
            return self.out[i][2:6]

        def info(self):
            return {"reruns": self.reruns}

    for arena_max, overflows in ((65536, False), (4, True)):
        tree, spliced = OracleTree(arena_max), []

        def backend(items, stats=None):
            tree.items = items

            def fallback(sub, st=None):
                spliced.extend(sub)
                return MB.oracle_milp_backend(nat, oracle, 4)(sub, st)
            return S.milptree_solve(items, stats, fallback=fallback, make=lambda: tree)
        stats = {}
        got = S._solve_many_with(oracle_batch_backend(oracle), solve_one, models, opts, stats, milp_backend=backend)
        for c, g, e in zip(cases, got, expected):
            assert same_solution(g, e), (c["name"], g["status"], e["status"])
        assert {k: stats[k] for k in ("batched", "milp", "large", "milp_batched")} == {k: host[k] for k in ("batched", "milp", "large", "milp_batched")}
        assert stats["milp_batched"] == 11 and stats["nodes_used"] == host["nodes_used"] > 0
        assert (stats["tree_overflows"] > 0) == overflows == bool(spliced) and stats["tree_overflows"] == len(spliced)
        assert stats["tree_reruns"] == tree.reruns and (tree.reruns > 0) == (not overflows) and stats["tree_launches"] == 1
    with pytest.raises(ValueError, match="milp_search"):
        S.solve_many(models[:1], opts[:1], milp_search="gpu")


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu(nat):
    assert nat.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return nat


@pytest.fixture(scope="module")
def tree(gpu):
    t = gpu.MilpTree(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def batch(gpu):
    b = gpu.MilpBatch(0)
    yield b
    b.close()


def record_milps():
    return [MB.milp_of(MB.record_model(r), r["options"]) for r in RECORDS]


def same_as_batch(tree, batch, milps, out=None, trace_cap=0):
    """tree.solve(milps) against batch.solve(milps) tree for tree: status, result bits, nodes used, solution bit for bit."""
    a = out if out is not None else tree.solve(milps, trace_cap=trace_cap)
    b = batch.solve(milps, node_batch=4)
    for i in range(len(milps)):
        assert (a[0][i], MT.bits(a[1][i]), int(a[2][i])) == (b[0][i], MT.bits(b[1][i]), int(b[2][i])), i
        x, y = tree.solution(i), batch.solution(i)
        assert x[0] == y[0] and all(MB.same_words(p, q) for p, q in zip(x[1:], y[1:])), i
    return a


@pytest.mark.gpu
def test_records_on_the_device_with_their_trace(tree, batch):
    milps = record_milps()
    out = tree.solve(milps, trace_cap=64)
    for i, r in enumerate(RECORDS):
        tag = _label(r)
        assert (out[0][i], BN.hexd(out[1][i]), int(out[2][i])) == (r["best"]["status"], r["best"]["result"], r["iterations"]), tag
        height, col0, pos, var = tree.solution(i)
        assert (height, BN.sha(col0), BN.sha(pos, var)) == (r["best"]["height"], r["best"]["col0_sha256"], r["best"]["perm_sha256"]), tag
        trace = tree.trace(i)
        assert len(trace) == min(64, len(r["nodes"])), tag
        for got, n in zip(trace, r["nodes"]):
            assert (BN.hexd(got["eval"]), [[s, v, BN.hexd(x)] for s, v, x in got["cuts"]], got["status"], BN.hexd(got["result"]),
                    got["n_pivots"], got["height"]) == (n["eval"], n["cuts"], n["status"], n["result"], n["n_pivots"],
                                                        r["height"] + len(n["cuts"])), tag
        assert int(out[3][i]) == sum(n["n_pivots"] for n in r["nodes"]), tag
    assert sum(out[2]) == 880 and out[4]["reruns"] == 0
    same_as_batch(tree, batch, milps, out)
    info = tree.info()
    walks = [k for k in info["kernels"] if k["kernel"].startswith("milp_tree_kernel")]
    assert len(walks) == len({(k["class"], "check" in k["kernel"]) for k in walks}) and sum(k["trees"] for k in walks) == 71
    assert info["launches"] == out[4]["launches"] == len(info["kernels"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TREE_KERNELS))
def test_every_instantiation_by_name(tree, oracle, name):
    cls, check, (m, n, k, seed, density) = TREE_KERNELS[name]
    extra = {"checkCycles": check, "maxIterations": 24}
    models = [ML._packing(np.random.RandomState(s), m, n, k, density=density) for s in (seed, seed + 1)]
    out = tree.solve([MB.milp_of(mod, extra) for mod in models], trace_cap=24)
    assert [(x["kernel"], x["class"]) for x in tree.info()["kernels"] if x["kernel"].startswith("milp_tree")] == [(name, cls)]
    for i, mod in enumerate(models):
        root, run = MB.oracle_tree(oracle, mod, extra)
        assert run is not None
        assert (out[0][i], BN.hexd(out[1][i]), int(out[2][i])) == (run["status"], BN.hexd(run["result"]), run["iterations"]), (name, i)
        height, col0, pos, var = tree.solution(i)
        assert (height, BN.sha(col0), BN.sha(pos, var)) == (run["best_height"], run["best_col0"], run["best_perm"]), (name, i)
        for got, x in zip(tree.trace(i), run["nodes"]):
            assert (BN.hexd(got["eval"]), got["status"], BN.hexd(got["result"]), got["n_pivots"]) == \
                (x["eval"], x["status"], x["result"], x["n_pivots"]), (name, i)


def solve_alone(model, opt):
    from yalps_amd import solve as S
    return S.solve(model, opt)


def tree_solution(nat_out, tree, i, model, opt):
    from yalps_amd.model import tableau_model
    tm = tableau_model(model)
    view_root = type("R", (), dict(w=tm.tableau.width, tm=tm))
    return MB.view_solution(view_root, MB.options(opt), nat_out[0][i], float(nat_out[1][i]), *tree.solution(i))


@pytest.mark.gpu
@pytest.mark.parametrize("check", [False, True])
def test_one_workgroup_many_trees(gpu, oracle, monkeypatch, check):
    monkeypatch.setenv("YALPS_MILPTREE_GRID", "1")
    rows = [(name, model, dict(opt, checkCycles=check)) for name, model, opt in MT.grid_one_models()]
    heights = MT.incumbent_heights(oracle, rows[0][1], rows[0][2])[1]
    assert len(heights) == 2 and heights[0] != heights[1]  # (chosen for this: two incumbents, one after the other, of other heights)
    assert MT.incumbent_heights(oracle, rows[5][1], rows[5][2])[0] == 20
    t = gpu.MilpTree(0)
    try:
        # every tree of one class and one checkCycles: ONE workgroup walks them all, largest first
        milps = [MB.milp_of(m, o) for _, m, o in rows]
        out = t.solve(milps + milps[::-1], trace_cap=4)
        walks = [k for k in t.info()["kernels"] if k["kernel"].startswith("milp_tree")]
        assert all(k["grid"] == 1 for k in walks) and max(k["trees"] for k in walks) >= 4
        for i, (name, model, opt) in enumerate(rows + rows[::-1]):
            assert same_solution(tree_solution(out, t, i, model, opt), solve_alone(model, opt)), name
        statuses = dict(zip([r[0] for r in rows], out[0]))
        assert statuses["root infeasible"] == "infeasible" and statuses["timeout <= 0"] == "timedout" and statuses["maxIterations 0"] == "timedout"
        assert int(out[2][1]) == 0 and statuses["integral root"] == "optimal"
    finally:
        t.close()


@pytest.mark.gpu
def test_reruns_and_overflow(gpu, batch, monkeypatch):
    from yalps_amd import solve as S
    models = [MB.packing_model(60, 60, 6, 1), MB.packing_model(40, 40, 6, 3)] + [m for m, _ in MB.small_family_models(24)]
    opts = [{"maxIterations": 64}] * 2 + [o for _, o in MB.small_family_models(24)]
    milps = [MB.milp_of(m, o) for m, o in zip(models, opts)]
    monkeypatch.setenv("YALPS_MILPTREE_ARENA", "2")
    t = gpu.MilpTree(0)
    try:
        out = same_as_batch(t, batch, milps, trace_cap=8)
        info = t.info()
        assert info["reruns"] == len(info["rerun_trees"]) > 0 and {0, 1} <= set(info["rerun_trees"]) and info["overflows"] == 0
        later = [k for k in info["kernels"] if k["pass"] > 0]
        assert later and all(k["arena"] == 2 * 4 ** k["pass"] for k in later)
    finally:
        t.close()
    # a grown arena beyond the byte bound of a pass: those trees come back OVERFLOW, the call does not fail
    monkeypatch.setenv("YALPS_MILPTREE_ARENA_BYTES", "64")
    t = gpu.MilpTree(0)
    try:
        cut = t.solve(milps)
        info = t.info()
        assert cut[0][0] == cut[0][1] == "overflow" and info["overflows"] == cut[0].count("overflow") and info["reruns"] == 0
        for i in range(len(milps)):
            assert cut[0][i] == "overflow" or (cut[0][i], MT.bits(cut[1][i]), int(cut[2][i])) == (out[0][i], MT.bits(out[1][i]), int(out[2][i])), i
    finally:
        t.close()
    monkeypatch.delenv("YALPS_MILPTREE_ARENA_BYTES")
    monkeypatch.setenv("YALPS_MILPTREE_ARENA_MAX", "2")
    t = gpu.MilpTree(0)
    try:
        out = t.solve(milps)
        assert out[0][0] == out[0][1] == "overflow" and math.isnan(out[1][0]) and t.info()["overflows"] == out[0].count("overflow")
    finally:
        t.close()
    # ... and solve_many on a handle of its own made under that cap: the lost trees come from the lockstep driver, dict for dict solve()'s
    monkeypatch.setattr(S, "_milptree", None)
    try:
        stats = {}
        got = S.solve_many(models, opts, stats, milp_search="device")
    finally:
        if S._milptree is not None:
            S._milptree.close()
            S._milptree = None
    assert stats["tree_overflows"] >= 2 and stats["milp_batched"] == len(models)
    for i, (g, m, o) in enumerate(zip(got, models, opts)):
        assert same_solution(g, S.solve(m, o)), i
    monkeypatch.delenv("YALPS_MILPTREE_ARENA")
    monkeypatch.delenv("YALPS_MILPTREE_ARENA_MAX")
    monkeypatch.setenv("YALPS_MILPTREE_HIST", "1")
    recs = [r for r in RECORDS if r["family"] == "cycles"]
    assert recs and all(r["options"]["checkCycles"] for r in recs)
    t = gpu.MilpTree(0)
    try:
        cyc = [MB.milp_of(MB.record_model(r), r["options"]) for r in recs]
        out = t.solve(cyc, trace_cap=64)
        for i, r in enumerate(recs):
            assert (out[0][i], BN.hexd(out[1][i]), int(out[2][i])) == (r["best"]["status"], r["best"]["result"], r["iterations"]), _label(r)
            assert [x["n_pivots"] for x in t.trace(i)] == [n["n_pivots"] for n in r["nodes"]]
        info = t.info()
        assert info["reruns"] > 0 and [k for k in info["kernels"] if k["pass"] > 0 and k["hist_cap"] == 4 ** k["pass"]]
    finally:
        t.close()


@pytest.mark.gpu
def test_shapes_at_the_class_and_aux_bounds(tree, batch, oracle):
    rows = MT.shape_models()
    milps = [MB.milp_of(m, o) for _, m, o in rows]
    for (name, _, _), milp in zip(rows, milps):
        w, h, n = milp[0], milp[1], len(milp[5])
        if name.startswith("under bound"):
            k = int(name[-1])
            assert LB.size_class(w, h) == k and MT.largest_class(milp) == k + 1, name
        if "aux bound" in name:
            assert not MT.BS.aux_hbm(w, h) and MT.BS.aux_hbm(w, h + 2 * n), name
    out = same_as_batch(tree, batch, milps, trace_cap=16)
    walks = {k["class"] for k in tree.info()["kernels"] if k["kernel"].startswith("milp_tree")}
    assert walks == {0, 1, 2, 3, 4}
    assert sum(out[2]) > 30
    # cuts on a variable that is basic and on one that is non-basic at the root, among the traced nodes; the negzero family, whose
    # results and column 0 hold -0.0, for the signed zeros the kernel itself reads
    seen = {"basic": 0, "nonbasic": 0}
    for i, (name, model, opt) in enumerate(rows):
        root = MB.Root(oracle, model, opt)
        for node in tree.trace(i):
            for s, v, x in node["cuts"]:
                seen["basic" if MT.BS.basic_at(root, v) else "nonbasic"] += 1
    same_as_batch(tree, batch, [MB.milp_of(*ML.make("negzero", s)) for s in range(12)], trace_cap=16)
    for i in range(12):
        root = MB.Root(oracle, *ML.make("negzero", i))
        for node in tree.trace(i):
            for s, v, x in node["cuts"]:
                seen["basic" if MT.BS.basic_at(root, v) else "nonbasic"] += 1
    assert seen["basic"] > 0 and seen["nonbasic"] > 0, seen
    # -0.0 cut values: Math.ceil of a column 0 entry in (-1, 0), which an optimal node has where `precision` is so coarse that
    # phase 2's ratio test passes over the coefficients at or below it.  tree_fill's sign * value then is +0.0 where a 0.0 cut gives
    # -0.0: trace, result and solution against the scalar search over the oracle and against MilpBatch
    rows = MT.negzero_cut_models()
    out = same_as_batch(tree, batch, [MB.milp_of(m, o) for _, m, o in rows], trace_cap=16)
    for i, (name, model, opt) in enumerate(rows):
        root, run = MB.oracle_tree(oracle, model, opt)
        assert run is not None and 0 < len(run["nodes"]) <= 16, name
        assert (out[0][i], BN.hexd(out[1][i]), int(out[2][i])) == (run["status"], BN.hexd(run["result"]), run["iterations"]), name
        height, col0, pos, var = tree.solution(i)
        assert (height, BN.sha(col0), BN.sha(pos, var)) == (run["best_height"], run["best_col0"], run["best_perm"]), name
        trace = tree.trace(i)
        assert [(BN.hexd(g["eval"]), [[s, v, BN.hexd(x)] for s, v, x in g["cuts"]], g["status"], BN.hexd(g["result"]), g["n_pivots"])
                for g in trace] == [(x["eval"], [list(c) for c in x["cuts"]], x["status"], x["result"], x["n_pivots"]) for x in run["nodes"]], name
        assert [-1, BN.hexd(-0.0)] in [[s, BN.hexd(x)] for g in trace for s, v, x in g["cuts"]], name


@pytest.mark.gpu
def test_mixing_over_thousands_of_trees(gpu, tree, batch, monkeypatch):
    small = MB.small_family_models(2048)
    models = [(m, o) for m, o in small] + [(MB.packing_model(*s, MT_SEEDS[s]), {"maxIterations": 32}) for s in MT_SEEDS]
    order = np.random.default_rng(3).permutation(len(models))
    milps = [MB.milp_of(*models[j]) for j in order]
    out = same_as_batch(tree, batch, milps)
    assert tree.info()["reruns"] == 0
    # ... and on 64 workgroups per launch: each walks dozens of trees, one after the other
    monkeypatch.setenv("YALPS_MILPTREE_GRID", "64")
    few = gpu.MilpTree(0)
    try:
        again = few.solve(milps)
        info = few.info()
        walks = [k for k in info["kernels"] if k["kernel"].startswith("milp_tree")]
        assert max(k["grid"] for k in walks) == 64 and max(k["trees"] for k in walks) > 1024
        for i in range(len(milps)):
            assert (again[0][i], MT.bits(again[1][i]), int(again[2][i])) == (out[0][i], MT.bits(out[1][i]), int(out[2][i])), i
            x, y = few.solution(i), tree.solution(i)
            assert x[0] == y[0] and all(MB.same_words(p, q) for p, q in zip(x[1:], y[1:])), i
    finally:
        few.close()


MT_SEEDS = {(40, 40, 6): 3, (60, 60, 6): 1, (80, 70, 6): 1, (100, 100, 6): 3}


@pytest.mark.gpu
def test_handle_reuse_and_a_callers_stream(gpu, batch, tmp_path):
    first = MT.stream_milps()
    second = [MB.milp_of(m, o) for m, o in MB.small_family_models(160)]
    third = [MB.milp_of(MB.packing_model(100, 100, 6, 3), {"maxIterations": 16}), MB.milp_of(*ML.make("mid", 0))]
    handle = gpu.MilpTree(0)
    try:
        runs = []
        for milps in (first, second, third, first):
            out = handle.solve(milps)
            runs.append((out[0], [MT.bits(x) for x in out[1]], list(out[2]), [tuple(BN.sha(a) for a in handle.solution(i)[1:]) for i in range(len(milps))]))
            with pytest.raises(gpu.NativeError, match="no such model"):
                handle.solution(len(milps))
        assert runs[0] == runs[3]
        mine = MT.outputs(handle, out, len(first))
        same_as_batch(handle, batch, third)
        with pytest.raises(gpu.NativeError, match="model 1: .*out of range"):
            handle.solve([first[0], (*first[0][:5], [first[0][0]], *first[0][6:])])
        with pytest.raises(gpu.NativeError, match="no such model"):
            handle.solution(0)  # (a refused batch leaves no last solve behind)
    finally:
        handle.close()
    # the same batch on a stream of the caller's, in a process where torch is loaded first
    path = str(tmp_path / "stream.npz")
    child = subprocess.run([sys.executable, "-m", "tests._milp_tree", path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    got = np.load(path)
    for key, value in mine.items():
        assert np.array_equal(np.asarray(value), got[key]), key


@pytest.mark.gpu
def test_nan_max_iterations_is_javascripts_on_every_path(gpu):
    """`iter >= maxIterations` (src/branchAndCut.ts:167) is false for NaN: a fractional root whose loop never runs ends
    "infeasible", not "timedout" -- in solve() (milp_host.inc), the lockstep driver and the device search alike."""
    from yalps_amd import solve as S
    models = [MB.packing_model(40, 40, 6, 3), MB.packing_model(60, 60, 6, 1)] + [m for m, _ in MB.small_family_models(8)]
    opts = [{"maxIterations": NAN}] * 2 + [dict(o or {}, maxIterations=NAN) for _, o in MB.small_family_models(8)]
    alone = [S.solve(m, o) for m, o in zip(models, opts)]
    assert alone[0]["status"] == alone[1]["status"] == "infeasible" and math.isnan(alone[0]["result"])
    assert "timedout" not in [a["status"] for a in alone]
    for search in ("host", "device"):
        stats = {}
        got = S.solve_many(models, opts, stats, milp_search=search)
        assert stats["milp_batched"] == len(models)
        for i, (g, a) in enumerate(zip(got, alone)):
            assert same_solution(g, a), (search, i, g["status"], a["status"])


@pytest.mark.gpu
def test_solve_many_device_equals_host(gpu):
    from yalps_amd import solve as S
    cases = [K.load(n) for n in K.names()]
    models, opts = [c["model"] for c in cases], [c["options"] for c in cases]
    stats, host = {}, {}
    got = S.solve_many(models, opts, stats, milp_search="device")
    want = S.solve_many(models, opts, host)
    assert got == want or all(same_solution(g, w) for g, w in zip(got, want))
    assert stats["milp_batched"] == host["milp_batched"] == 11 and stats["nodes_used"] == host["nodes_used"] > 0
    assert stats["tree_launches"] >= 2 and stats["tree_overflows"] == 0
    milps = MB.small_family_models(200, first_seed=400)
    rng = np.random.RandomState(9)
    models, opts = [], []
    for k, (model, opt) in enumerate(milps):
        models += [model, ML._packing(np.random.RandomState(2000 + k), int(rng.randint(3, 12)), int(rng.randint(3, 12)), 0)]
        opts += [opt, {}]
    got, want = S.solve_many(models, opts, milp_search="device"), S.solve_many(models, opts)
    assert all(same_solution(g, w) for g, w in zip(got, want))
