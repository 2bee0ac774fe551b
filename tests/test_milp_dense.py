"""libyalps_milpdense.so and milp_batch on the GPU.  The work runs in child processes that import torch first
(tests/_milp_dense.py says why); every test here compares what a child wrote with the oracle-driven search of
tests/_np_milp_dense.py -- the C oracle solves the root from the numpy tableau, the host search rules run with the oracle as node
evaluator -- bit for bit, all NaNs counted as one value."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _milp_dense as MD
from tests import _np_milp_dense as NM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("YALPS_MILPDENSE_ARENA", "YALPS_MILPDENSE_ARENA_MAX", "YALPS_MILPDENSE_HIST", "YALPS_MILPDENSE_GRID", "YALPS_MILPDENSE_CUS",
         "YALPS_MILPDENSE_PER_CU", "YALPS_LPDENSE_CUS", "YALPS_LPDENSE_PER_CU")


def run_child(tmp_path_factory, which, env=None, tag=None):
    from yalps_amd import build
    for make in (build.build_milpdense, build.build_milptree, build.build_milpbatch, build.build_lpdense, build.build_hip):
        make()
    path = str(tmp_path_factory.mktemp("milp_dense") / ((tag or which) + ".npz"))
    clean = {k: v for k, v in os.environ.items() if k not in HOOKS}
    child = subprocess.run([sys.executable, "-m", "tests._milp_dense", which, path], cwd=ROOT, capture_output=True, text=True, timeout=600,
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
            made[name] = NM.expected(nat, oracle, call or MD.table_call(name))
        return made[name]
    return get


def same(a, b):
    return np.array_equal(NM.words(a), NM.words(b))


def of(ran, name):
    return {k[len(name) + 1:]: v for k, v in ran.items() if k.startswith(name + "/")}


def check_tensors(got, call, rows, tag, fallback=()):
    """The six output tensors of a call against the expectation; fallback: rows the host answered (node_pivots = -1)."""
    B = len(call.lps)
    assert got["x"].shape == (B, call.n) and all(got[k].shape == (B,) for k in ("objective", "status", "nodes", "node_pivots", "root_pivots")), tag
    assert got["x"].dtype == got["objective"].dtype == np.float64 and got["status"].dtype == np.int32
    assert got["nodes"].dtype == got["node_pivots"].dtype == got["root_pivots"].dtype == np.int64
    for i, row in enumerate(rows):
        who = "%s MILP %d" % (tag, i)
        assert NM.STATUS[int(got["status"][i])] == row["status"], (who, got["status"][i], row["status"])
        assert int(got["nodes"][i]) == row["nodes"], (who, got["nodes"][i], row["nodes"])
        assert int(got["node_pivots"][i]) == (-1 if i in fallback else row["node_pivots"]), (who, got["node_pivots"][i], row["node_pivots"])
        assert int(got["root_pivots"][i]) == row["root_pivots"], (who, got["root_pivots"][i], row["root_pivots"])
        assert same(got["objective"][i], row["objective"]), (who, got["objective"][i], row["objective"])
        assert same(got["x"][i], row["x"]), (who, got["x"][i], row["x"])


def check_trees(got, call, rows, tag):
    """Status, result and best tableau of the trees a child kept, against the expectation."""
    for i in range(len(got["height"])):
        row, who = rows[i], "%s MILP %d" % (tag, i)
        h = int(got["height"][i])
        assert (NM.STATUS[int(got["tree_status"][i])], h) == (row["status"], row["height"]), (who, got["tree_status"][i], h, row["status"], row["height"])
        assert same(got["tree_result"][i], row["result"]), (who, got["tree_result"][i], row["result"])
        assert same(got["col0"][i][:h], row["col0"]), who
        assert np.array_equal(got["pos"][i][:call.w + h], row["pos"]) and np.array_equal(got["var"][i][:call.w + h], row["var"]), who


def tree_kernel(call):
    cls = LB.size_class(call.w, call.hmax)
    return "milp_tree_kernel<%d%s%s>" % (1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")


def root_kernel(call):
    cls = LB.size_class(call.w, call.h)
    return "milp_dense_root_kernel<%d%s%s>" % (1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")


@pytest.mark.parametrize("name", MD.names())
def test_call_against_the_oracle_search(ran, refs, name):
    call, got, rows = MD.table_call(name), of(ran, name), refs(name)
    check_tensors(got, call, rows, name)
    check_trees(got, call, rows, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    assert int(got["overflows"]) == 0 and int(got["reruns"]) == 0, name
    kernels = [root_kernel(call)] + ([tree_kernel(call)] if call.ints else []) + ["milp_dense_solution_kernel<256>"]
    assert str(got["kernels"]).split() == kernels and int(got["launches"]) == len(kernels), (name, got["kernels"])
    assert got["classes"].tolist()[:len(kernels) - 1] == [LB.size_class(call.w, call.h)] + ([LB.size_class(call.w, call.hmax)] if call.ints else [])
    if name == "queue":
        assert got["grids"].tolist() == [2048, 2048, MD.QUEUE_MILPS]


@pytest.mark.parametrize("name", [n for n in MD.names() if n != "no integers"])
def test_trace_equals_the_oracle_node_sequence(ran, refs, name):
    traces = json.loads(str(of(ran, name)["traces"]))
    rows = refs(name)
    assert len(traces) == min(len(rows), 16)
    for i, (got, row) in enumerate(zip(traces, rows)):
        want = row["trace"][:MD.TRACE_CAP]
        assert len(got) == len(want), (name, i, len(got), len(want))
        for k, (g, w) in enumerate(zip(got, want)):
            g = (g[0], tuple(tuple(c) for c in g[1]), g[2], g[3], g[4], g[5])
            assert g == tuple(w), (name, i, k, g, w)


def test_no_integers_equals_linprog_batch(ran, refs):
    milp, lp = of(ran, "no integers/milp"), of(ran, "no integers/lp")
    for a, b in (("x", "x"), ("objective", "objective"), ("status", "status"), ("root_pivots", "pivots")):
        assert milp[a].tobytes() == lp[b].tobytes() and milp[a].dtype == lp[b].dtype, a
    assert not milp["nodes"].any() and not milp["node_pivots"].any()
    check_tensors(milp, MD.table_call("no integers"), refs("no integers"), "no integers")


def test_views_side_stream_and_empty_batch(ran, nat, oracle):
    call = MD.view_call(MD.view_inputs())
    rows = NM.expected(nat, oracle, call)
    assert any(r["nodes"] > 0 for r in rows)
    for tag in ("views", "contiguous"):
        check_tensors(of(ran, tag), call, rows, tag)
    assert bool(ran["views/unchanged"])
    inp = MD.stream_inputs()
    A = inp["A_half"] * 2.0
    assert ran["stream/A"].tobytes() == A.tobytes()  # (the producer had finished when the call read it)
    call = NM.Call("stream", [(inp["c"][i], A[i], inp["b_ub"][i], None, None) for i in range(4)], integers=True, maximize=True)
    check_tensors(of(ran, "stream"), call, NM.expected(nat, oracle, call), "stream")
    assert int(ran["stream/handles"]) == 2 and str(ran["stream/kernels"]).split()[0].startswith("milp_dense_root_kernel")
    assert ran["empty/shapes"].tolist() == [0, 3, 0, 0, 0, 0, 0] and int(ran["empty/launches"]) == 0
    assert str(ran["empty/dtypes"]) == "torch.float64 torch.float64 torch.int32 torch.int64 torch.int64 torch.int64"


def test_refusals_name_the_argument(ran, refs):
    msgs = [str(m) for m in ran["refusal/messages"]]
    # (pageable host memory: unknown to the runtime, or known as host memory, depending on what the allocator registered)
    for m, name in zip(msgs, ("c", "b_ub", "x_out", "nodes_out")):
        assert "yalps_milpdense_solve: %s is " % name in m and ("this HIP runtime does not know" in m or "is host memory" in m), m
    assert "yalps_milpdense_solve: b_ub is host memory" in msgs[1], msgs[1]  # (pinned)
    assert all(m.endswith("launches=0") for m in msgs) and bool(ran["refusal/x_untouched"])
    got = of(ran, "refusal/after")
    check_tensors(got, MD.table_call("n=2"), refs("n=2"), "after the refusals")


@pytest.mark.parametrize("name", ["several nodes", "under bound 2", "tolerance"])
def test_milp_tree_on_the_packed_milps_agrees(ran, name):
    """The parent route: the same MILPs as packed cell lists through _native.MilpTree."""
    dense, tree = of(ran, name), of(ran, "tree/" + name)
    assert np.array_equal(dense["status"], tree["status"]) and np.array_equal(dense["tree_status"], tree["status"])
    assert same(dense["tree_result"], tree["result"]) and np.array_equal(dense["nodes"], tree["nodes"])
    assert np.array_equal(dense["node_pivots"], tree["node_pivots"]) and np.array_equal(dense["height"], tree["height"])
    for i, h in enumerate(tree["height"]):
        assert same(dense["col0"][i][:h], tree["col0"][i][:h])
        assert np.array_equal(dense["pos"][i], tree["pos"][i]) and np.array_equal(dense["var"][i], tree["var"][i])


# ---------------------------------------------------------------------------------------------- the test hooks

@pytest.fixture(scope="module")
def mix_rows(nat, oracle):
    return NM.expected(nat, oracle, MD.mix_call())


def test_one_workgroup_walks_many_trees(tmp_path_factory, mix_rows):
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_GRID": "1"}, "grid")
    check_tensors(got, MD.mix_call(), mix_rows, "grid 1")
    kernels, grids = str(got["kernels"]).split(), got["grids"].tolist()
    assert [g for k, g in zip(kernels, grids) if k.startswith("milp_tree_kernel")] == [1] and int(got["reruns"]) == 0


def test_arena_rerun_of_some_trees(tmp_path_factory, nat, oracle, mix_rows):
    """An arena of 2: the trees that outgrow it run again, the others keep what the first pass wrote -- and the epilogue, which
    runs after the last pass, reads both kinds."""
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_ARENA": "2"}, "arena")
    mix = MD.mix_call()
    check_tensors(got, mix, mix_rows, "arena 2")
    small = NM.expected(nat, oracle, mix, arena=2)
    assert int(got["reruns"]) == small[0]["reruns"] and 0 < int(got["reruns"]) < len(mix.lps)
    assert int(got["passes"]) >= 2 and int(got["overflows"]) == 0
    assert 0 < len(set(got["rerun_trees"].tolist())) < len(mix.lps)


def test_overflow_is_answered_by_the_host(tmp_path_factory, nat, oracle, mix_rows):
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_ARENA": "2", "YALPS_MILPDENSE_ARENA_MAX": "2"}, "overflow")
    mix = MD.mix_call()
    capped = NM.expected(nat, oracle, mix, arena=2, arena_max=2)
    over = {i for i, r in enumerate(capped) if r["status"] == "overflow"}
    assert 0 < len(over) < len(mix.lps) and int(got["overflows"]) == len(over)
    assert 5 not in got["status"].tolist()
    check_tensors(got, mix, mix_rows, "overflow", fallback=over)


def test_history_rerun(tmp_path_factory, nat, oracle):
    got = run_child(tmp_path_factory, "hist", {"YALPS_MILPDENSE_HIST": str(MD.HIST)})
    call = MD.hist_call()
    check_tensors(got, call, NM.expected(nat, oracle, call), "hist")
    assert int(got["reruns"]) >= 2 * len(call.lps) and int(got["passes"]) >= 2  # every root, and every tree
    assert all("check" in k for k in str(got["kernels"]).split() if not k.startswith("milp_dense_solution"))
