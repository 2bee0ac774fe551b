"""milp_batch(lb=, ub=, upper=) and yalps_milpdense_solve_bounds on the GPU.  The work runs in child processes that import torch
first (tests/_milp_dense.py says why); every test here compares what a child wrote with tests/_np_milp_dense_bounds.py -- the C
oracle solves the root from the numpy restatement of the bounded tableau, the host search rules run with the oracle as node
evaluator, x and the objective are moved back -- bit for bit, all NaNs counted as one value.
tests/test_milp_dense_bounds_model.py shows, with the oracle alone, that the calls "hard n=65" and "hard n=129" tell the documented
order of summation and the documented read-out from every flaw of tests/_np_dense_bounds.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _milp_dense as MD
from tests import _milp_dense_bounds as MDB
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB
from tests.test_milp_dense import HOOKS, check_tensors, check_trees, of, same, tree_kernel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPILOGUE = "milp_dense_bounds_solution_kernel<256>"


def run_child(tmp_path_factory, which, env=None, tag=None):
    from yalps_amd import build
    for make in (build.build_milpdense, build.build_milptree, build.build_milpbatch, build.build_lpdense, build.build_hip):
        make()
    path = str(tmp_path_factory.mktemp("milp_dense_bounds") / ((tag or which) + ".npz"))
    clean = {k: v for k, v in os.environ.items() if k not in HOOKS}
    child = subprocess.run([sys.executable, "-m", "tests._milp_dense_bounds", which, path], cwd=ROOT, capture_output=True, text=True, timeout=600,
                           env=dict(clean, **(env or {})))
    assert child.returncode == 0, child.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native
    return _native


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    return run_child(tmp_path_factory, "table")


@pytest.fixture(scope="module")
def refs(nat, oracle):
    """name -> the expectation of a call, computed once and shared."""
    made = {}

    def get(name, call=None):
        if name not in made:
            made[name] = NB.expected(nat, oracle, call or MDB.table_call(name))
        return made[name]
    return get


def root_kernel(call):
    cls = LB.size_class(call.w, call.h)
    return "milp_dense_bounds_root_kernel<%d%s%s>" % (1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")


def kernels_of(call):
    return [root_kernel(call)] + ([tree_kernel(call)] if call.ints else []) + [EPILOGUE]


@pytest.mark.parametrize("name", MDB.names())
def test_call_against_the_oracle_search(ran, refs, name):
    call, got, rows = MDB.table_call(name), of(ran, name), refs(name)
    check_tensors(got, call, rows, name)
    check_trees(got, call, rows, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    assert int(got["overflows"]) == 0 and int(got["reruns"]) == 0, name
    kernels = kernels_of(call)
    assert str(got["kernels"]).split() == kernels and int(got["launches"]) == len(kernels), (name, got["kernels"])
    assert got["classes"].tolist()[:2] == [LB.size_class(call.w, call.h), LB.size_class(call.w, call.hmax)]
    if name.split(" check")[0] in MDB.SHAPES:
        assert int(got["aux"][0]) == int(name.startswith("aux form"))
    if name == "queue":
        assert got["grids"].tolist() == [2048, 2048, MDB.QUEUE_MILPS]


@pytest.mark.parametrize("name", MDB.names())
def test_trace_equals_the_oracle_node_sequence(ran, refs, name):
    traces = json.loads(str(of(ran, name)["traces"]))
    rows = refs(name)
    assert len(traces) == min(len(rows), 16)
    for i, (got, row) in enumerate(zip(traces, rows)):
        want = row["trace"][:MDB.TRACE_CAP]
        assert len(got) == len(want), (name, i, len(got), len(want))
        for k, (g, w) in enumerate(zip(got, want)):
            g = (g[0], tuple(tuple(c) for c in g[1]), g[2], g[3], g[4], g[5])
            assert g == tuple(w), (name, i, k, g, w)


def test_binaries_are_not_read(ran, refs):
    """Rule 2 on the device: NaN in lb and ub at the binary columns gives the bits of the call with clean numbers there."""
    poisoned, clean = of(ran, "NaN at binaries public"), of(ran, "clean at binaries")
    for key in MDB.OUTPUTS:
        assert poisoned[key].tobytes() == clean[key].tobytes(), key
    assert not np.isnan(poisoned["x"]).any()
    check_tensors(poisoned, MDB.table_call("NaN at binaries"), refs("NaN at binaries"), "NaN at binaries, public")


def test_no_integers_equals_linprog_batch_with_the_same_bounds(ran, nat, oracle):
    milp, lp = of(ran, "no integers/milp"), of(ran, "no integers/lp")
    for a, b in (("x", "x"), ("objective", "objective"), ("status", "status"), ("root_pivots", "pivots")):
        assert milp[a].tobytes() == lp[b].tobytes() and milp[a].dtype == lp[b].dtype, a
    assert not milp["nodes"].any() and not milp["node_pivots"].any()
    call = MDB.lp_call()
    call = NB.BCall(call.name, [(*lp_, lb, ub) for lp_, lb, ub in zip(call.lps, call.lbs, call.ubs)], upper=(0, 2, 5), maximize=True)
    rows = NB.expected(nat, oracle, call)
    check_tensors(milp, call, rows, "no integers")
    assert (milp["status"] == 0).any() and str(ran["no integers/kernels"]).split() == [root_kernel(call), EPILOGUE]


def test_boundless_call_is_what_it_was(ran, nat, oracle):
    """milp_batch without lb / ub, yalps_milpdense_solve_bounds with both descriptors NULL, and yalps_milpdense_solve: the same bits
    and the boundless kernels, by name."""
    call = MD.table_call("several nodes")
    rows = NM.expected(nat, oracle, call)
    solve, abi, public = of(ran, "boundless/solve"), of(ran, "boundless/abi"), of(ran, "boundless/public")
    check_tensors(solve, call, rows, "boundless, solve")
    for key in MDB.OUTPUTS:
        assert solve[key].tobytes() == abi[key].tobytes() == public[key].tobytes(), key
    names = ["milp_dense_root_kernel<256,lds>", tree_kernel(call), "milp_dense_solution_kernel<256>"]
    assert str(solve["kernels"]).split() == str(ran["boundless/abi kernels"]).split() == str(ran["boundless/public kernels"]).split() == names


def test_identity_block_route_agrees(ran, refs):
    bounded, rows = of(ran, "identity/bounded"), of(ran, "identity/rows")
    call = MDB.identity_call()
    check_tensors(bounded, call, refs("identity", call), "identity")
    assert np.array_equal(bounded["status"], rows["status"]) and (bounded["status"] == 0).all()
    assert np.array_equal(bounded["objective"], rows["objective"])  # (as numbers: the tableaux differ, and so may the vertex of a tie)
    assert bounded["nodes"].any() and rows["nodes"].any()


def test_views_shared_bounds_side_stream_and_empty_batch(ran, nat, oracle):
    per, shared = MDB.view_call()
    rows = NB.expected(nat, oracle, per)
    assert any(r["nodes"] > 0 for r in rows)
    check_tensors(of(ran, "views"), per, rows, "views")
    assert bool(ran["views/unchanged"]) and str(ran["views/kernels"]).split() == kernels_of(per)
    srows = NB.expected(nat, oracle, shared)
    for tag in ("shared", "shared copies"):
        check_tensors(of(ran, tag), shared, srows, tag)
    assert ran["stream/lb"].tobytes() == per.bounds_stacked()[0].tobytes()  # (the producer had finished when the call read it)
    check_tensors(of(ran, "stream"), per, rows, "stream")
    assert ran["empty/shapes"].tolist() == [0, 3, 0, 0, 0, 0, 0] and int(ran["empty/launches"]) == 0


def test_partial_outputs(ran, nat, oracle):
    call = MDB.partial_call()
    rows = NB.expected(nat, oracle, call)
    whole = {"x": np.stack([r["x"] for r in rows]), "objective": np.array([r["objective"] for r in rows]),
             "status": np.array([NM.STATUS.index(r["status"]) for r in rows], np.int32), "nodes": np.array([r["nodes"] for r in rows], np.int64),
             "node_pivots": np.array([r["node_pivots"] for r in rows], np.int64), "root_pivots": np.array([r["root_pivots"] for r in rows], np.int64)}
    for want in MDB.PARTIAL:
        got = of(ran, "partial %s" % ("+".join(want) or "none"))
        for key in MDB.OUTPUTS:
            if key in want:
                assert same(got[key], whole[key]) if key in ("x", "objective") else np.array_equal(got[key], whole[key]), (want, key)
            else:
                assert (got[key] == -7).all(), (want, key)  # (not passed: not written)
        check_trees(got, call, rows, "partial")


def test_refusals_name_the_bound(ran, refs, nat, oracle):
    msgs = [str(m) for m in ran["refusal/messages"]]
    for m, name in zip(msgs, ("lb", "ub")):
        assert "yalps_milpdense_solve_bounds: %s is " % name in m and ("this HIP runtime does not know" in m or "is host memory" in m), m
    assert "yalps_milpdense_solve_bounds: ub is host memory" in msgs[1], msgs[1]  # (pinned)
    assert all(m.endswith("launches=0") for m in msgs) and bool(ran["refusal/untouched"])
    call = MDB.partial_call()
    check_tensors(of(ran, "refusal/after"), call, NB.expected(nat, oracle, call), "after the refusals")


# ---------------------------------------------------------------------------------------------- the test hooks

@pytest.fixture(scope="module")
def mix_rows(nat, oracle):
    return NB.expected(nat, oracle, MDB.mix_call())


def test_one_workgroup_walks_many_trees(tmp_path_factory, mix_rows):
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_GRID": "1"}, "grid")
    check_tensors(got, MDB.mix_call(), mix_rows, "grid 1")
    kernels, grids = str(got["kernels"]).split(), got["grids"].tolist()
    assert [g for k, g in zip(kernels, grids) if k.startswith("milp_tree_kernel")] == [1] and int(got["reruns"]) == 0
    assert kernels[0].startswith("milp_dense_bounds_root_kernel") and kernels[-1] == EPILOGUE


def test_arena_rerun_of_some_trees(tmp_path_factory, nat, oracle, mix_rows):
    """An arena of 2: the trees that outgrow it run again, the two roots without a tree keep what the first pass wrote -- and the
    bounded epilogue, which runs after the last pass, reads both kinds."""
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_ARENA": "2"}, "arena")
    mix = MDB.mix_call()
    check_tensors(got, mix, mix_rows, "arena 2")
    small = NB.expected(nat, oracle, mix, arena=2)
    assert int(got["reruns"]) == small[0]["reruns"] > 0
    assert int(got["passes"]) >= 2 and int(got["overflows"]) == 0
    assert 0 < len(set(got["rerun_trees"].tolist())) < len(mix.lps)


def test_overflow_is_answered_by_the_host_and_moved_back(tmp_path_factory, nat, oracle, mix_rows):
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_ARENA": "2", "YALPS_MILPDENSE_ARENA_MAX": "2"}, "overflow")
    mix = MDB.mix_call()
    capped = NB.expected(nat, oracle, mix, arena=2, arena_max=2)
    over = {i for i, r in enumerate(capped) if r["status"] == "overflow"}
    assert 0 < len(over) < len(mix.lps) and int(got["overflows"]) == len(over)
    assert 5 not in got["status"].tolist()
    check_tensors(got, mix, mix_rows, "overflow", fallback=over)
    assert any(mix_rows[i]["low"].any() for i in over)  # (the host had something to move back)


def test_history_rerun(tmp_path_factory, nat, oracle):
    got = run_child(tmp_path_factory, "hist", {"YALPS_MILPDENSE_HIST": str(MDB.HIST)})
    call = MDB.hist_call()
    check_tensors(got, call, NB.expected(nat, oracle, call), "hist")
    assert int(got["reruns"]) >= 2 * len(call.lps) and int(got["passes"]) >= 2  # every root, and every tree
    assert all("check" in k for k in str(got["kernels"]).split() if not k.startswith("milp_dense_bounds_solution"))
