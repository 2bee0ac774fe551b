"""lp_batch_kernel and milp_node_kernel at the shapes and endings the record-driven tests do not reach (tests/_batch_shapes.py
holds the three tables): the aux form of the HBM class (colbuf / prow behind the tableau in HBM, pcols + h > 8192) next to the
LDS-aux form in one launch, an odd column count in the HBM form, the degenerate shapes the validators admit, the batch limit;
nodes with zero cuts, cuts on basic and non-basic variables, signed-zero cut values, both sides of a class bound from one
root, budgets that end a node inside phase 1 and inside phase 2; trees whose nodes a finite maxPivots ends as "cycled", trees
that grow across a class bound and across the aux bound, roots that are not optimal.

Every expectation is computed here by the C oracle and tests/_bnc.py; every comparison is bit for bit.  The tables' coverage is
counted and asserted (test_what_the_tables_cover), and the node comparison is shown to reject four wrong evaluators."""
import math
from collections import Counter

import numpy as np
import pytest

from tests import _batch_shapes as BS
from tests import _bnc as BN
from tests import _golden as G
from tests import _lp_batch as LB
from tests import _milp_batch as MB
from tests.test_lp_batch import same_solution


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpbatch()
    build.build_milpbatch()
    return _native


@pytest.fixture(scope="module")
def shapes(oracle):
    return BS.shape_table(oracle)


@pytest.fixture(scope="module")
def roots(oracle):
    return [BS.solve_root(oracle, model, extra) for _, model, extra in BS.node_roots()]


@pytest.fixture(scope="module")
def table(roots):
    return BS.node_table(roots)


@pytest.fixture(scope="module")
def trees(oracle):
    return [(name, model, extra, *MB.oracle_tree(oracle, model, extra)) for name, model, extra in BS.tree_table()]


def budget_of(root, budget):
    return float(root.opt["maxPivots"] if budget is None else budget)


def node_shape(roots, row):
    return roots[row[1]].w, roots[row[1]].h + len(row[2])


def node_disagreements(refs, gots):
    """The rows of the node table where what an evaluator returned is not, key for key, the reference's node."""
    return [k for k, (ref, got) in enumerate(zip(refs, gots)) if ref != got]


# ---------------------------------------------------------------------------------------------------------- CPU

def test_every_input_passes_the_validators(nat, shapes, roots, table, trees):
    nat.PackedLps([lp for _, lp in shapes]).validate()
    nat.PackedLps([BS.root_lp(m, e) for _, m, e in BS.node_roots()]).validate()
    nat.milp_validate_nodes([r.w for r in roots], [r.h for r in roots], [row[1] for row in table], [row[2] for row in table])
    for row in table:  # (as the whole-solve validator allows: at most two cuts per integer variable)
        assert len(row[2]) <= 2 * len(roots[row[1]].tm.integers), row[0]
    nat.PackedMilps([MB.milp_of(m, e) for _, m, e, _, _ in trees]).validate(node_batch=3)
    # the aux rule restated in _batch_shapes.py is the library's, at every shape of the three tables
    tree_shapes = [(root.w, root.h + k) for _, _, _, root, _ in trees for k in range(2 * len(root.tm.integers) + 1)
                   if 8 * root.w * (root.h + k) <= 4 << 20]
    for w, h in [(lp[0], lp[1]) for _, lp in shapes] + [node_shape(roots, row) for row in table] + tree_shapes:
        assert nat.lpbatch_aux_hbm(w, h) == int(LB.size_class(w, h) == 4 and BS.aux_hbm(w, h)), (w, h)


def test_what_the_tables_cover(oracle, shapes, roots, table, trees):
    # ---- the root pass
    cls = Counter(LB.size_class(lp[0], lp[1]) for _, lp in shapes)
    assert cls == {0: 9, 3: 2, 4: 62} and len(shapes) == 73
    hbm = [(name, lp) for name, lp in shapes if LB.size_class(lp[0], lp[1]) == 4]
    assert Counter(BS.aux_hbm(lp[0], lp[1]) for _, lp in hbm) == {True: 48, False: 14}
    assert Counter((lp[0] - 1) % 2 for _, lp in hbm) == {1: 47, 0: 15}  # n odd | even in the HBM form
    for check in (False, True):  # each HBM-class launch holds both forms
        assert {BS.aux_hbm(lp[0], lp[1]) for _, lp in hbm if lp[7] == check} == {False, True}
    assert {(lp[0], lp[1]) for _, lp in shapes} >= {(262144, 2), (64, 8191), (512, 1024), (1, 1), (2, 1), (1, 4000), (2, 6000)}
    assert {BS.pcols(lp[0]) + lp[1] for _, lp in hbm} >= {8192, 8193}
    answers = [LB.oracle_answer(oracle, lp) for _, lp in shapes]
    assert Counter(a["status"] for a in answers) == {"optimal": 31, "cycled": 34, "infeasible": 6, "unbounded": 2}
    for (name, lp), a in zip(shapes, answers):
        if "budget" in name and lp[6] != math.inf:  # the aux rows under a budget: ended by it, at once or mid-way (a budget holds per phase)
            assert a["status"] == "cycled" and (a["n_pivots"] == 0) == (lp[6] == 0) and a["n_pivots"] <= 2 * math.ceil(lp[6]), name
    # ---- the node table
    assert [r.status for r in roots] == ["optimal"] * 9 + ["cycled"] * 3 + ["optimal"] + ["cycled"] * 2
    assert [r.n_pivots for r in roots[-2:]] == [11, 11]  # (the E9c roots: ended by hasCycle, not by their budget of 8192)
    shape = [node_shape(roots, row) for row in table]
    ncls = Counter(LB.size_class(w, h) for w, h in shape)
    assert ncls == {0: 28, 1: 10, 2: 10, 3: 29, 4: 62} and len(table) == 139
    assert Counter(BS.aux_hbm(w, h) for w, h in shape if LB.size_class(w, h) == 4) == {False: 55, True: 7}
    assert Counter((w - 1) % 2 for w, h in shape if LB.size_class(w, h) == 4) == {1: 44, 0: 18}
    assert max(8 * w * h for w, h in shape) == 4 << 20
    branch = Counter(b for row in table for b in BS.takes_basic_branch(roots[row[1]], row[2]))
    assert branch[True] > 0 and branch[False] > 0 and branch == {True: 93, False: 145}
    zeros = Counter((s, math.copysign(1.0, x)) for row in table for s, _, x in row[2] if x == 0.0 and row[0] == "signed zero")
    assert set(zeros) == {(1, 1.0), (1, -1.0), (-1, 1.0), (-1, -1.0)}
    assert sum(not row[2] for row in table) == 17
    # one root on both sides of every class bound and of the aux bound
    for name in ("under bound 0", "under bound 1", "under bound 2", "under bound 3"):
        ri = [n for n, _, _ in BS.node_roots()].index(name)
        k = LB.size_class(roots[ri].w, roots[ri].h)
        assert {LB.size_class(*node_shape(roots, row)) for row in table if row[1] == ri} == {k, k + 1}, name
    for name in ("tall under the aux bound", "wide under the aux bound"):
        ri = [n for n, _, _ in BS.node_roots()].index(name)
        assert {BS.aux_hbm(*node_shape(roots, row)) for row in table if row[1] == ri} == {False, True}, name
    # the ending every row was built for
    ends = []
    for name, ri, cuts, budget, want in table:
        limit = name == "4 MiB node"  # (its replay is long: the status alone)
        end = BS.node_reference(oracle, roots[ri], cuts, budget)[0]["status"] if limit else BS.ending(oracle, roots[ri], cuts, budget)
        assert want is None or end == want, (name, ri, cuts, budget, end)
        ends.append((end, bool(roots[ri].opt["checkCycles"]), LB.size_class(*node_shape(roots, (name, ri, cuts))) == 4))
    count = Counter(e for e, _, _ in ends)
    assert count == {"optimal": 87, "cycled": 27, "hasCycle": 10, "phase 1": 8, "phase 2": 7}
    # (ending, checkCycles, HBM form) of the nodes a budget ends: both phases in the LDS and in the HBM form, with and without
    # checkCycles; and of the nodes hasCycle ends (see _batch_shapes.py): in both forms
    assert {e for e in ends if e[0].startswith("phase")} == {("phase 1", False, False), ("phase 1", False, True), ("phase 1", True, True),
                                                             ("phase 2", False, True), ("phase 2", True, False)}
    assert {e for e in ends if e[0] == "hasCycle"} == {("hasCycle", True, False), ("hasCycle", True, True)}
    assert BS.has_cycle_search(oracle) == (106920, [])  # (the MILP families have no node that hasCycle ends: E9c has)
    # ---- the trees
    endings = {name: Counter(x["status"] for x in run["nodes"]) for name, _, _, _, run in trees if run is not None}
    assert endings["cycles-0, maxPivots 5"] == {"infeasible": 3, "optimal": 3, "cycled": 2}
    assert endings["cycles-0, default budget"] == {"optimal": 4, "infeasible": 2}
    for name in ("ties-0, maxPivots 3", "break-0, maxPivots 4", "eqmm-0, maxPivots 5", "eqmm-3, maxPivots 5"):
        assert endings[name]["cycled"] >= 3, (name, endings[name])
    by_name = {name: (root, run) for name, _, _, root, run in trees}
    assert by_name["cycles-0, maxPivots 5"][1]["status"] == "infeasible" and by_name["cycles-0, default budget"][1]["status"] == "optimal"
    assert by_name["eqmm-0, maxPivots 5"][1]["status"] == "optimal"  # (a tree that drops cycled nodes and still finds a solution)
    classes = lambda name: (LB.size_class(by_name[name][0].w, by_name[name][0].h),
                            Counter(LB.size_class(by_name[name][0].w, by_name[name][0].h + len(x["cuts"])) for x in by_name[name][1]["nodes"]))
    assert classes("class 2 -> 3") == (2, {3: 4}) and classes("class 3 -> HBM") == (3, {4: 6}) and classes("odd n HBM") == (4, {4: 24})
    tall = by_name["tall across the aux bound"]
    assert Counter(BS.aux_hbm(tall[0].w, tall[0].h + len(x["cuts"])) for x in tall[1]["nodes"]) == {False: 2, True: 10}
    wide = by_name["wide across the aux bound"]
    assert (wide[0].w, wide[0].h, wide[1]["status"], wide[1]["iterations"]) == (8151, 41, "optimal", 18)
    assert Counter(BS.aux_hbm(wide[0].w, wide[0].h + len(x["cuts"])) for x in wide[1]["nodes"]) == {False: 2, True: 16}
    assert by_name["odd n HBM"][0].w % 2 == 0
    assert {name: root.status for name, _, _, root, run in trees if run is None} == {
        "root infeasible": "infeasible", "root unbounded": "unbounded", "root cycled by budget": "cycled",
        "root cycled by budget, ties-1": "cycled"}


WRONG = {
    "budget one too large": lambda o, root, cuts, budget: BS.node_reference(o, root, cuts, budget_of(root, budget) + 1.0),
    "-0.0 cut values as +0.0": lambda o, root, cuts, budget: BS.node_reference(o, root, [(s, v, x + 0.0) for s, v, x in cuts], budget),
    "a basic variable's cut as a non-basic one's": lambda o, root, cuts, budget: BS.node_reference(
        o, root, cuts, budget, apply=BS.apply_cuts_basic_as_nonbasic),
}


@pytest.mark.parametrize("mutant", sorted(WRONG) + ["the neighbouring model's budget"])
def test_the_node_comparison_rejects_a_wrong_evaluator(oracle, roots, table, mutant):
    """node_disagreements is what the GPU test runs on milp_node_kernel's output: an evaluator wrong in one of the new ways must
    not pass it (and the right one must)."""
    refs = [BS.node_reference(oracle, roots[ri], cuts, budget)[0] for _, ri, cuts, budget, _ in table]
    assert node_disagreements(refs, [BS.node_reference(oracle, roots[ri], cuts, budget)[0] for _, ri, cuts, budget, _ in table]) == []
    if mutant in WRONG:
        gots = [WRONG[mutant](oracle, roots[ri], cuts, budget)[0] for _, ri, cuts, budget, _ in table]
    else:  # a node without a budget of its own takes its root's: here the next root's
        gots = [BS.node_reference(oracle, roots[ri], cuts, budget_of(roots[(ri + 1) % len(roots)], None) if budget is None else budget)[0]
                for _, ri, cuts, budget, _ in table]
    assert node_disagreements(refs, gots), mutant


@pytest.mark.parametrize("node_batch", (1, 3))
def test_trees_through_the_lockstep_driver(nat, oracle, trees, node_batch):
    rts = [root for _, _, _, root, _ in trees]
    out, nodes, ev, _ = MB.run_search(nat, oracle, rts, node_batch)
    for (name, _, _, root, run), o, seq in zip(trees, out, nodes):
        assert BS.tree_disagreement(o, root, run) is None, (name, BS.tree_disagreement(o, root, run))
        if run is not None:  # node by node, in the order the tree consumed them
            assert [(n["status"], n["result"], n["n_pivots"], n["final_sha256"]) for n in seq] == \
                   [(n["status"], n["result"], n["n_pivots"], n["final_sha256"]) for n in run["nodes"]], name
    # the budget of the neighbouring model: the comparison must notice
    shifted = [MB.Root(oracle, m, dict(e, maxPivots=MB.options(trees[(i + 1) % len(trees)][2])["maxPivots"]))
               for i, (_, m, e, _, _) in enumerate(trees[:7])]
    out, _, _, _ = MB.run_search(nat, oracle, shifted, node_batch)
    assert sum(BS.tree_disagreement(o, root, run) is not None for (_, _, _, root, run), o in zip(trees[:7], out)) >= 4


def test_solve_many_on_the_trees_with_the_oracle(nat, oracle, trees):
    from yalps_amd import solve as S
    from tests.test_lp_batch import oracle_backend, oracle_batch_backend
    models, opts = [m for _, m, _, _, _ in trees], [e for _, _, e, _, _ in trees]
    one = oracle_backend(oracle)
    stats = {}
    got = S._solve_many_with(oracle_batch_backend(oracle), lambda m, o: S._solve_with(one, m, o), models, opts, stats,
                             milp_backend=MB.oracle_milp_backend(nat, oracle, 3))
    assert stats["milp_batched"] == len(trees)
    for (name, m, e, _, _), g in zip(trees, got):
        assert same_solution(g, S._solve_with(one, m, e)), name


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu(nat):
    assert nat.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return nat


@pytest.mark.gpu
def test_shape_table_as_one_batch(gpu, oracle, shapes):
    order = list(np.random.default_rng(23).permutation(len(shapes)))
    lps = [shapes[j][1] for j in order]
    b = gpu.LpBatch(0)
    try:
        out = b.solve(lps, keep_tableaux=True)
        info = b.info()
        for i, j in enumerate(order):
            LB.check_lp(b, i, out, LB.oracle_answer(oracle, lps[i]), lps[i], label=shapes[j][0])
    finally:
        b.close()
    # one launch per (class, checkCycles): the HBM-class launches each held aux and non-aux members
    first = {(k["class"], "check" in k["kernel"]): k for k in info["kernels"] if k["pass"] == 0}
    assert info["reruns"] == 0 and len(first) == info["launches"]
    for check in (False, True):
        members = [lp for lp in lps if LB.size_class(lp[0], lp[1]) == 4 and lp[7] == check]
        aux = [BS.aux_hbm(lp[0], lp[1]) for lp in members]
        assert any(aux) and not all(aux)
        k = first[(4, check)]
        assert k["lps"] == len(members) and k["kernel"] == "lp_batch_kernel<1024%s>" % (",check" if check else "")
        # the launch's dynamic LDS is that of its non-aux members only
        lds = max(8 * (BS.pcols(lp[0]) + lp[1]) for lp, a in zip(members, aux) if not a)
        assert k["lds"] == (lds + 15) & ~15 <= BS.AUX_LDS_MAX


def gpu_nodes(batch, roots, table, budgets):
    statuses, results, pivots, heights = batch.nodes([row[1] for row in table], [row[2] for row in table], max_pivots=budgets,
                                                    keep_tableaux=True)
    out = []
    for k, row in enumerate(table):
        w = roots[row[1]].w
        m = batch.node_tableau(k)
        col0, pos, var = batch.node(k)
        assert MB.same_words(col0, m[::w]), (row[0], k)
        out.append(dict(height=int(heights[k]), status=statuses[k], result=BS.bits(float(results[k])), n_pivots=int(pivots[k]),
                        final_sha256=G.sha256(m), perm_sha256=BN.sha(pos, var), col0_sha256=BN.sha(col0)))
    return out


def check_node_roots(batch, roots):
    out = batch.roots([BS.root_lp(m, e) for _, m, e in BS.node_roots()])
    for i, r in enumerate(roots):
        assert (out[0][i], BS.bits(float(out[1][i])), int(out[2][i])) == (r.status, BS.bits(r.result), r.n_pivots), i
        col0, pos, var, m = batch.root(i, matrix=True)
        assert MB.same_words(m, r.matrix) and np.array_equal(pos, r.pos) and np.array_equal(var, r.var), i


@pytest.mark.gpu
def test_node_table(gpu, oracle, roots, table):
    refs = [BS.node_reference(oracle, roots[ri], cuts, budget)[0] for _, ri, cuts, budget, _ in table]
    b = gpu.MilpBatch(0)
    try:
        check_node_roots(b, roots)
        # budget 0: the initial tableau applyCuts leaves, signed zeros included
        zero = gpu_nodes(b, roots, table, 0.0)
        for k, (g, ref) in enumerate(zip(zero, refs)):
            assert (g["status"], g["n_pivots"], g["height"], g["final_sha256"]) == ("cycled", 0, ref["height"], ref["init_sha256"]), table[k][:4]
        # every node under its own budget, in one pass
        gots = gpu_nodes(b, roots, table, [budget_of(roots[row[1]], row[3]) for row in table])
        info = b.info()
    finally:
        b.close()
    for g, ref in zip(gots, refs):
        g["init_sha256"] = ref["init_sha256"]  # (compared above)
    bad = node_disagreements(refs, gots)
    assert bad == [], [(table[k][:4], refs[k], gots[k]) for k in bad[:3]]
    # one pass held the nodes of both sides of every bound: a launch per (class, checkCycles), its size from the table
    first = {(k["class"], "check" in k["kernel"]): k["nodes"] for k in info["kernels"] if k["pass"] == 0}
    want = Counter((LB.size_class(*node_shape(roots, row)), bool(roots[row[1]].opt["checkCycles"])) for row in table)
    assert first == dict(want) and {c for c, _ in first} == {0, 1, 2, 3, 4}
    lds4 = [k["lds"] for k in info["kernels"] if k["pass"] == 0 and k["class"] == 4 and "check" not in k["kernel"]]
    nonaux = [8 * (BS.pcols(w) + h) for w, h in (node_shape(roots, row) for row in table)
              if LB.size_class(w, h) == 4 and not BS.aux_hbm(w, h)]
    assert lds4 == [max(nonaux)] and max(nonaux) == BS.AUX_LDS_MAX  # (8192 doubles: the last shape that keeps them in LDS)


@pytest.mark.gpu
def test_history_rerun_of_aux_nodes(gpu, oracle, monkeypatch):
    monkeypatch.setenv("YALPS_MILPBATCH_HIST", "2")
    tall = BS.packing(8160, 30, 6, 1, 0.3)
    extra = {"checkCycles": True}
    root = MB.Root(oracle, tall, extra)
    cut_lists = [BS.bound_cuts(root, k) for k in (0, 1, 2, 3)]
    refs = [BS.node_reference(oracle, root, cuts)[0] for cuts in cut_lists]
    assert [BS.aux_hbm(root.w, r["height"]) for r in refs] == [False, False, True, True] and all(r["n_pivots"] > 4 for r in refs[1:])
    b = gpu.MilpBatch(0)
    try:
        b.roots([MB.lp_of(MB.milp_of(tall, extra))])
        table = [("aux rerun", 0, cuts, None, None) for cuts in cut_lists]
        gots = gpu_nodes(b, [root], table, None)
        info = b.info()
    finally:
        b.close()
    for g, ref in zip(gots, refs):
        g["init_sha256"] = ref["init_sha256"]
    assert node_disagreements(refs, gots) == []
    assert {1, 2, 3} <= set(info["rerun_nodes"]) and 0 not in info["rerun_nodes"]
    later = [k for k in info["kernels"] if k["pass"] > 0]
    assert later and all(k["kernel"] == "milp_node_kernel<1024,check>" and k["hist_cap"] == 2 * 4 ** k["pass"] for k in later)


@pytest.mark.gpu
@pytest.mark.parametrize("node_batch", (1, 3))
def test_trees_whole_solve(gpu, oracle, trees, node_batch):
    from tests.test_milp_batch import check_against_oracle_tree
    b = gpu.MilpBatch(0)
    try:
        out = b.solve([MB.milp_of(m, e) for _, m, e, _, _ in trees], node_batch=node_batch)
        info = b.info()
        for i, (name, _, _, root, run) in enumerate(trees):
            if run is not None:
                check_against_oracle_tree(b, i, out, root, run)
                continue
            # a root that is not optimal: its status and result, no node, and the root's own tableau as the solution
            assert (out[0][i], BS.bits(float(out[1][i])), int(out[2][i]), int(out[3][i])) == (root.status, BS.bits(root.result), 0, 0), name
            height, col0, pos, var = b.solution(i)
            assert height == root.h and MB.same_words(col0, root.matrix[::root.w][:root.h]), name
            assert np.array_equal(pos, root.pos) and np.array_equal(var, root.var), name
    finally:
        b.close()
    # every round's HBM-class launch held the nodes the driver gives it, its dynamic LDS that of the non-aux ones alone; the
    # first held the nodes at the very bound (8192 doubles of colbuf and prow in LDS), later ones held both forms
    want = BS.hbm_launches(gpu, oracle, [root for _, _, _, root, _ in trees], node_batch)
    got = {(k["round"], "check" in k["kernel"]): (k["nodes"], k["lds"]) for k in info["kernels"]
           if k["kernel"].startswith("milp_node_kernel") and k["class"] == 4 and k["pass"] == 0}
    assert got == {key: (n, lds) for key, (n, aux, lds) in want.items()}
    mixed = [(n, aux, lds) for n, aux, lds in want.values() if 0 < aux < n]
    assert len(mixed) >= 2 and want[(0, False)][1:] == (0, BS.AUX_LDS_MAX)
    launched = {(k["kernel"], k["class"]) for k in info["kernels"] if k["kernel"].startswith("milp_node_kernel")}
    # (class 3 and the HBM form: the trees that left their root's class)
    assert {c for _, c in launched} == {0, 3, 4} and ("milp_node_kernel<256,check,lds>", 0) in launched
    roots_launched = {k["class"] for k in info["kernels"] if k["kernel"].startswith("lp_batch_kernel")}
    assert roots_launched == {0, 1, 2, 3, 4}


@pytest.mark.gpu
def test_solve_many_equals_solve_on_the_trees(gpu, trees):
    from yalps_amd import solve as S
    models, opts = [m for _, m, _, _, _ in trees], [e for _, _, e, _, _ in trees]
    stats = {}
    got = S.solve_many(models, opts, stats)
    assert stats["milp_batched"] == len(trees) and stats["nodes_used"] == sum(run["iterations"] for *_, run in trees if run is not None)
    for (name, m, e, _, _), g in zip(trees, got):
        assert same_solution(g, S.solve(m, e)), name
