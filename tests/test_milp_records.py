"""The MILP records (tests/golden/simplex_milp.json.gz: the reference's solve() -- tableauModel, simplex, branchAndCut,
solution -- run on the models of tests/_milps.py) pin the host side of branch and cut on the CPU: the model builder, the
Python driver node by node with the C oracle as its node solver, the exit, the best tableau and the Solution.  A scalar
restatement (tests/_bnc.py) with one switch per decision site of branchAndCut.ts shows that the records reject each
wrong reading of it."""
import json
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import _bnc as B
from tests import _golden as G
from tests import _milps as ML
from yalps_amd import branch_and_cut as BC
from yalps_amd import model as M
from yalps_amd import solve as S

RECORDS = G.records("milp")
ALL = [pytest.param(r, id=ML.label(r["family"], r["seed"], r["variant"])) for r in RECORDS]


def options(rec):
    opt = dict(S.default_options)
    opt.update(rec["options"])
    return opt


def marshal(sol):
    return {"status": sol["status"], "result": B.hexd(sol["result"]), "variables": [[k, B.hexd(v)] for k, v in sol["variables"]]}


def test_records_cover_every_family_and_exit():
    assert sorted((r["family"], r["seed"], r["variant"]) for r in RECORDS) == sorted(ML.specs())
    assert {r["family"] for r in RECORDS} == set(ML.FAMILIES)
    assert {r["exit"] for r in RECORDS} == {"integral", "break", "iterations", "exhausted", "threshold", "timeout"}
    assert {r["solution"]["status"] for r in RECORDS} == {"optimal", "infeasible", "timedout"}
    # "timedout" with a solution and without one (NaN result)
    timed = [r for r in RECORDS if r["solution"]["status"] == "timedout"]
    assert {_is_nan(r["solution"]["result"]) for r in timed} == {True, False}
    # the iterations budget met on the very iteration the queue empties / the threshold is crossed
    assert {r["exit"] for r in RECORDS if r["family"] == "iters" and r["iterations"] == r["variant"]} >= {"iterations"}
    assert any(r["family"] == "iters" and r["exit"] == "iterations" and r["solution"]["status"] == "optimal" for r in RECORDS)
    # equal evaluations among the popped nodes, and checkCycles on nodes
    assert any(len({n["eval"] for n in r["nodes"]}) < len(r["nodes"]) for r in RECORDS)
    assert any(r["options"].get("checkCycles") and r["nodes"] for r in RECORDS)
    # a cut list as long as the node buffers allow (2 * n_integers)
    assert any(len(n["cuts"]) == 2 * len(r["integers"]) for r in RECORDS for n in r["nodes"])
    # root sizes: LDS-sized, 128 KB .. 4 MB, over 4 MB
    sizes = [8 * r["width"] * r["height"] for r in RECORDS if r["nodes"]]
    assert min(sizes) < 128 << 10 and any(128 << 10 < s <= 4 << 20 for s in sizes) and max(sizes) > 4 << 20


def _is_nan(hexstr):
    return bool(np.isnan(np.frombuffer(bytes.fromhex(hexstr), ">f8")[0]))


@pytest.mark.parametrize("rec", ALL)
def test_tableau_model_reproduces_the_initial_tableau(rec):
    model, opts = ML.make(rec["family"], rec["seed"], rec["variant"])
    assert opts == rec["options"]
    tm = M.tableau_model(model)
    assert (tm.tableau.width, tm.tableau.height) == (rec["width"], rec["height"])
    assert G.sha256(tm.tableau.matrix) == rec["init_sha256"]
    assert tm.sign == rec["sign"] and tm.integers == rec["integers"]


def _root(oracle, rec):
    tm = M.tableau_model(ML.make(rec["family"], rec["seed"], rec["variant"])[0])
    t = tm.tableau
    opt = options(rec)
    st, res, npiv, _ = oracle.simplex(t.matrix, t.width, t.height, t.position_of_variable, t.variable_at_position,
                                      precision=opt["precision"], max_pivots=opt["maxPivots"], check_cycles=opt["checkCycles"])
    assert (st, B.hexd(res), npiv, G.sha256(t.matrix)) == (rec["root"]["status"], rec["root"]["result"], rec["root"]["n_pivots"],
                                                           rec["root"]["final_sha256"])
    return tm, res


NODE_KEYS = {"eval", "cuts", "init_sha256", "status", "result", "n_pivots", "final_sha256", "perm_sha256"}


def _check_run(rec, nodes, best):
    """Every key of every node compared (a node that lacks one fails), the node count and the tableau solution() reads."""
    assert len(nodes) == rec["iterations"] == len(rec["nodes"])
    for i, (got, want) in enumerate(zip(nodes, rec["nodes"])):
        assert set(want) == set(got) == NODE_KEYS, (i, set(got), set(want))
        assert got == want, (i, got, want)
    assert best == (rec["best"]["height"], rec["best"]["col0_sha256"], rec["best"]["perm_sha256"])


@pytest.mark.parametrize("rec", ALL)
def test_python_driver_with_the_oracle_reproduces_the_record(oracle, rec, monkeypatch):
    """yalps_amd.solve's host flow (tableau_model, root simplex, branch_and_cut, solution) with the C oracle as the simplex:
    every node (cuts with the sign of zero, initial and final tableau, status, result bits, pivots, basis), the number of
    nodes, the tableau solution() reads and the Solution, names, order and value bits."""
    import heapq
    from tests.test_host_model import oracle_backend
    base = oracle_backend(oracle)
    calls, cuts_seen, popped, handed = [], [], [], []

    def spy(tableau, opt):
        init = G.sha256(tableau.matrix)
        st, res, npiv, _ = oracle.simplex(tableau.matrix, tableau.width, tableau.height, tableau.position_of_variable,
                                          tableau.variable_at_position, precision=opt["precision"],
                                          max_pivots=opt["maxPivots"], check_cycles=opt["checkCycles"])
        calls.append(dict(init_sha256=init, status=st, result=B.hexd(res), n_pivots=npiv, final_sha256=G.sha256(tableau.matrix),
                          perm_sha256=B.sha(tableau.position_of_variable, tableau.variable_at_position)))
        return st, res

    def apply_cuts(tableau, buf, cuts):
        cuts_seen.append([[int(s), int(v), B.hexd(x)] for s, v, x in cuts])
        return orig_apply(tableau, buf, cuts)

    def heappop(heap):
        br = heapq.heappop(heap)
        popped.append(B.hexd(br.eval))
        return br

    def solution(tabmod, status, result, opt):
        t = tabmod.tableau
        col0 = t.matrix[::t.width][:t.height] if t.matrix is not None else t.col0
        handed.append((t.height, B.sha(col0), B.sha(t.position_of_variable[:t.width + t.height],
                                                      t.variable_at_position[:t.width + t.height])))
        return orig_solution(tabmod, status, result, opt)

    orig_apply, orig_solution = BC.apply_cuts, S.solution
    monkeypatch.setattr(BC, "apply_cuts", apply_cuts)
    monkeypatch.setattr(S, "solution", solution)
    monkeypatch.setattr(BC, "heapq", types.SimpleNamespace(heappush=heapq.heappush, heappop=heappop, nsmallest=heapq.nsmallest))
    model = ML.make(rec["family"], rec["seed"], rec["variant"])[0]
    sol = S._solve_with(spy, model, rec["options"], node_batch=0, sparse=False, device_nodes=False, native=False)
    assert calls[0]["status"] == rec["root"]["status"] and calls[0]["result"] == rec["root"]["result"]
    assert calls[0]["final_sha256"] == rec["root"]["final_sha256"]
    nodes = [dict(c, cuts=k, eval=e) for c, k, e in zip(calls[1:], cuts_seen, popped)]
    assert len(cuts_seen) == len(calls) - 1
    # every pop is a node, but the one that breaks the loop (:119)
    assert popped[len(nodes):] == ([rec["break_eval"]] if rec["exit"] == "break" else [])
    _check_run(rec, nodes, handed[0])
    assert marshal(sol) == rec["solution"]
    if "solution_flip" in rec:
        flipped = dict(rec["options"], includeZeroVariables=not rec["options"].get("includeZeroVariables", False))
        sol = S._solve_with(base, model, flipped, node_batch=0, sparse=False, device_nodes=False, native=False)
        assert marshal(sol) == rec["solution_flip"]


def _restated(oracle, rec, rules=frozenset()):
    tm, res = _root(oracle, rec)
    t = tm.tableau
    return B.branch_and_cut(oracle, t.matrix, t.width, t.height, t.position_of_variable, t.variable_at_position, tm.sign,
                            tm.integers, res, options(rec), rules)


def _agrees(run, rec):
    try:
        _check_run(rec, [{k: v for k, v in n.items()} for n in run["nodes"]],
                   (run["best_height"], run["best_col0"], run["best_perm"]))
    except AssertionError:
        return False
    return run["exit"] == rec["exit"] and run["status"] == rec["best"]["status"] and B.hexd(run["result"]) == rec["best"]["result"]


@pytest.mark.parametrize("rec", [p for p in ALL if p.values[0]["root"]["status"] == "optimal"])
def test_restatement_reproduces_the_record(oracle, rec):
    run = _restated(oracle, rec)
    assert [n["eval"] for n in run["nodes"]] == [n["eval"] for n in rec["nodes"]]
    assert _agrees(run, rec)
    assert rec.get("break_eval") is None or rec["exit"] == "break"


MUTANT_RECORDS = [r for r in RECORDS if r["root"]["status"] == "optimal" and 8 * r["width"] * r["height"] <= 4096]


@pytest.mark.parametrize("mutant", sorted(set(B.MUTANTS) - {"ceil_plus_zero"}))
def test_each_mutant_is_rejected_by_a_record(oracle, mutant):
    assert any(not _agrees(_restated(oracle, r, {mutant}), r) for r in MUTANT_RECORDS), mutant


def test_ceil_sign_of_zero_is_not_reached_by_the_records(oracle):
    """No record has a cut value of -0 (tests/_milps.py NEGZERO_SEEDS): the ceil_plus_zero mutant agrees with them all, and
    the sign is pinned by test_cut_values_keep_the_sign_of_zero instead."""
    assert not any(c[2] == B.hexd(-0.0) for r in RECORDS for n in r["nodes"] for c in n["cuts"])
    assert all(_agrees(_restated(oracle, r, {"ceil_plus_zero"}), r) for r in MUTANT_RECORDS)


@pytest.mark.parametrize("driver", ["sequential", "batched", "device"])
def test_cut_values_keep_the_sign_of_zero(monkeypatch, driver):
    """Math.ceil (branchAndCut.ts:103, :155) and std::ceil (milp_host.inc) of a value in (-1, 0) are -0; each Python driver
    must hand the same cut to its node solver, or the node's tableau differs from the reference's in the sign of a zero.  A
    one-row root whose integer variable is basic at -0.5 makes the first two nodes (-1, x, ceil(-0.5)) and
    (1, x, floor(-0.5)).  The node solvers are stand-ins that record the cuts they get and report every node infeasible:
    the drivers' own code builds the cuts (branch_and_cut: apply_cuts; _batched: NodeBatch.solve; _device: node_solve)."""
    from yalps_amd import _native
    from yalps_amd.model import Tableau, TableauModel
    w, h = 2, 2
    matrix = np.array([0.0, 1.0, -0.5, 1.0])
    pos = np.array([0, 3, 2, 1], np.int32)  # variable 1 is basic on row 1 (position 3)
    var = np.array([0, 3, 2, 1], np.int32)
    opt = dict(S.default_options)
    cuts = []
    if driver == "sequential":
        orig = BC.apply_cuts
        monkeypatch.setattr(BC, "apply_cuts", lambda t, buf, c: cuts.append(list(c)) or orig(t, buf, c))
        tabmod = TableauModel(Tableau(matrix, w, h, pos, var), 1.0, [("x", {})], [1])
        BC.branch_and_cut(lambda tableau, o: ("infeasible", math.nan), tabmod, 0.0, opt)
    elif driver == "batched":
        class Batch:
            def __init__(self, ctx, width, root_height, max_cuts, max_nodes):
                self.root_height = root_height

            def set_root(self, *a):
                pass

            def solve(self, cut_lists, precision, max_pivots):
                cuts.extend(list(c) for c in cut_lists)
                n = len(cut_lists)
                return (["infeasible"] * n, np.full(n, np.nan), np.zeros(n, np.int64),
                        self.root_height + np.array([len(c) for c in cut_lists]), 0.0)

            def close(self):
                pass

        monkeypatch.setattr(_native, "Context", lambda device: types.SimpleNamespace(close=lambda: None))
        monkeypatch.setattr(_native, "NodeBatch", Batch)
        tabmod = TableauModel(Tableau(matrix, w, h, pos, var), 1.0, [("x", {})], [1])
        BC.branch_and_cut_batched(tabmod, 0.0, opt, 32)
    else:
        class Node:
            def node_solve(self, root, c, precision, max_pivots, check_cycles):
                cuts.append(list(c))
                return "infeasible", math.nan, h + len(c), None, None, None

        view = TableauModel(Tableau(None, w, h, pos, var, matrix[::w].copy()), 1.0, [("x", {})], [1])
        BC.branch_and_cut_device(view, object(), Node(), 0.0, opt)
    assert sorted(c[0][:2] for c in cuts) == [(-1, 1), (1, 1)]
    values = {c[0][0]: c[0][2] for c in cuts}
    assert B.hexd(values[-1]) == B.hexd(-0.0) and values[1] == -1.0


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_heap_stand_in_equals_heapq(tmp_path):
    """The generator's stand-in for npm heap (oracle/tools/gen_golden.py HEAP_MJS), run under node, pops in heapq's order
    on seeded push / pop sequences full of ties; heapq compares by the evaluation only, as the drivers' _Branch does."""
    import heapq
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(G.GOLDEN, "..", "..", "oracle", "tools",
                                                                              "gen_golden.py"))
    gg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gg)
    (tmp_path / "heap.mjs").write_text(gg.HEAP_MJS)
    (tmp_path / "driver.mjs").write_text(gg.HEAP_DRIVER)
    rng = np.random.RandomState(5)
    seqs = []
    for k in range(60):
        n = int(rng.randint(5, 200))
        evals = rng.randint(0, 1 + k % 6, size=n).astype(float)  # few distinct values: ties everywhere
        seqs.append([None if rng.random_sample() < 0.35 else float(e) for e in evals])
    (tmp_path / "ops.json").write_text(json.dumps(seqs))
    out = subprocess.run(["node", str(tmp_path / "driver.mjs"), str(tmp_path / "ops.json")], capture_output=True, text=True,
                         check=True, timeout=120).stdout.splitlines()
    assert len(out) == len(seqs)
    for ops, line in zip(seqs, out):
        heap, popped = [], []
        for i, op in enumerate(ops):
            if op is None:
                if heap:
                    popped.append(heapq.heappop(heap).cuts)
            else:
                heapq.heappush(heap, BC._Branch(op, i))
        while heap:
            popped.append(heapq.heappop(heap).cuts)
        assert json.loads(line) == popped
