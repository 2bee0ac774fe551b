"""milp_batch_free(free=) and yalps_milpdense_solve_free on the GPU.  The work runs in child processes that import torch first
(tests/_milp_dense.py says why); every test here compares what a child wrote with tests/_np_milp_dense_free.py -- the C oracle
solves the root from the numpy restatement of the split tableau, the host search rules run with the oracle as node evaluator on the
integer columns of rule 4, x and the objective are moved back -- bit for bit, all NaNs counted as one value.
tests/test_milp_dense_free_model.py shows, with the oracle alone, which calls of the table tell each flaw of NF.FLAWS."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _milp_dense as MD
from tests import _milp_dense_bounds as MDB
from tests import _milp_dense_free as MF
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB
from tests import _np_milp_dense_free as NF
from tests.test_milp_dense import HOOKS, check_tensors, check_trees, of, tree_kernel
from tests.test_milp_dense_bounds import kernels_of as bounded_kernels_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPILOGUE = "milp_dense_free_solution_kernel<256>"


def run_child(tmp_path_factory, which, env=None, tag=None):
    from yalps_amd import build
    for make in (build.build_milpdense, build.build_milptree, build.build_milpbatch, build.build_lpdense, build.build_hip):
        make()
    path = str(tmp_path_factory.mktemp("milp_dense_free") / ((tag or which) + ".npz"))
    clean = {k: v for k, v in os.environ.items() if k not in HOOKS}
    child = subprocess.run([sys.executable, "-m", "tests._milp_dense_free", which, path], cwd=ROOT, capture_output=True, text=True, timeout=600,
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
            made[name] = NF.expected(nat, oracle, call or MF.table_call(name))
        return made[name]
    return get


def root_kernel(call):
    cls = LB.size_class(call.w, call.h)
    return "milp_dense_free_root_kernel<%d%s%s>" % (1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")


def kernels_of(call):
    return [root_kernel(call)] + ([tree_kernel(call)] if call.ints else []) + [EPILOGUE]


@pytest.mark.parametrize("name", MF.names())
def test_call_against_the_oracle_search(ran, refs, name):
    call, got, rows = MF.table_call(name), of(ran, name), refs(name)
    check_tensors(got, call, rows, name)
    check_trees(got, call, rows, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    assert int(got["overflows"]) == 0 and int(got["reruns"]) == 0, name
    kernels = kernels_of(call)
    assert str(got["kernels"]).split() == kernels and int(got["launches"]) == len(kernels), (name, got["kernels"])
    assert got["classes"].tolist()[:2] == [LB.size_class(call.w, call.h), LB.size_class(call.w, call.hmax)]
    if name.split(" check")[0] in MF.SHAPES:
        assert int(got["aux"][0]) == int(name.startswith("aux form"))


def test_the_table_names_every_form(ran):
    """All six compiled forms of the root kernel: LDS 256, LDS 1024 and HBM, each with and without `check`; and the aux form."""
    roots = {str(of(ran, name)["kernels"]).split()[0] for name in MF.names()}
    forms = ("256,lds", "256,check,lds", "1024,lds", "1024,check,lds", "1024", "1024,check")
    assert {"milp_dense_free_root_kernel<%s>" % t for t in forms} == roots, roots
    assert int(of(ran, "aux form")["aux"][0]) == 1 and int(of(ran, "HBM")["aux"][0]) == 0


@pytest.mark.parametrize("name", MF.names())
def test_trace_equals_the_oracle_node_sequence(ran, refs, name):
    traces = json.loads(str(of(ran, name)["traces"]))
    rows = refs(name)
    assert len(traces) == min(len(rows), 16)
    for i, (got, row) in enumerate(zip(traces, rows)):
        want = row["trace"][:MF.TRACE_CAP]
        assert len(got) == len(want), (name, i, len(got), len(want))
        for k, (g, w) in enumerate(zip(got, want)):
            g = (g[0], tuple(tuple(c) for c in g[1]), g[2], g[3], g[4], g[5])
            assert g == tuple(w), (name, i, k, g, w)


def test_lb_is_not_read_at_the_free_columns(ran, refs):
    """Rule 2 on the device: NaN in lb at the free columns gives the bits of the call with clean numbers there."""
    poisoned, clean = of(ran, "NaN in lb at free public"), of(ran, "clean at free")
    for key in MF.OUTPUTS:
        assert poisoned[key].tobytes() == clean[key].tobytes(), key
    assert not np.isnan(poisoned["x"]).any()
    check_tensors(poisoned, MF.table_call("NaN in lb at free"), refs("NaN in lb at free"), "NaN in lb at free, public")


def test_no_integers_equals_linprog_batch_with_the_same_free_variables(ran, nat, oracle):
    milp, lp = of(ran, "no integers/milp"), of(ran, "no integers/lp")
    for a, b in (("x", "x"), ("objective", "objective"), ("status", "status"), ("root_pivots", "pivots")):
        assert milp[a].tobytes() == lp[b].tobytes() and milp[a].dtype == lp[b].dtype, a
    assert not milp["nodes"].any() and not milp["node_pivots"].any()
    call = MF.lp_call()
    call = NF.FCall(call.name, [(*lp_, lb, ub) for lp_, lb, ub in zip(call.lps, call.lbs, call.ubs)], (0, 1, 5), call.free, maximize=True)
    rows = NF.expected(nat, oracle, call)
    check_tensors(milp, call, rows, "no integers")
    assert (milp["status"] == 0).any() and (milp["x"] < 0.0).any() and str(ran["no integers/kernels"]).split() == [root_kernel(call), EPILOGUE]


def test_a_call_without_free_variables_is_what_it_was(ran, nat, oracle):
    """free=(), yalps_milpdense_solve_free with n_free = 0 and yalps_milpdense_solve_bounds: the same bits and the bounded kernels by
    name; and without bounds yalps_milpdense_solve's bits and the boundless kernels."""
    call = MF.plain_call()
    rows = NB.expected(nat, oracle, call)
    bounds, entry, public, empty = (of(ran, "plain/" + k) for k in ("bounds", "free entry", "public", "public free=()"))
    check_tensors(bounds, call, rows, "plain, bounds")
    check_trees(entry, call, rows, "plain, free entry")
    for key in MF.OUTPUTS:
        assert bounds[key].tobytes() == entry[key].tobytes() == public[key].tobytes() == empty[key].tobytes(), key
    names = bounded_kernels_of(call)
    assert str(bounds["kernels"]).split() == str(entry["kernels"]).split() == str(ran["plain/public kernels"]).split() \
        == str(ran["plain/public free=() kernels"]).split() == names
    assert json.loads(str(bounds["traces"])) == json.loads(str(entry["traces"]))
    base = MD.table_call("several nodes")
    rows = NM.expected(nat, oracle, base)
    solve, entry, public = (of(ran, "boundless/" + k) for k in ("solve", "free entry", "public"))
    check_tensors(solve, base, rows, "boundless, solve")
    for key in MF.OUTPUTS:
        assert solve[key].tobytes() == entry[key].tobytes() == public[key].tobytes(), key
    names = ["milp_dense_root_kernel<256,lds>", tree_kernel(base), "milp_dense_solution_kernel<256>"]
    assert str(solve["kernels"]).split() == str(entry["kernels"]).split() == str(ran["boundless/public kernels"]).split() == names


def test_concatenated_route_agrees(ran, refs):
    free, cat = of(ran, "concat/free"), of(ran, "concat/cat")
    call = MF.concat_call()
    check_tensors(free, call, refs("concat", call), "concat")
    assert np.array_equal(free["status"], cat["status"]) and (free["status"] == 0).all()
    assert np.array_equal(free["objective"], cat["objective"])  # (as numbers: the tableaux differ in their row order, and so may the vertex of a tie)
    assert free["nodes"].any() and cat["nodes"].any() and cat["x"].shape[1] == call.n + call.f


def test_views_shared_bounds_side_stream_and_empty_batch(ran, nat, oracle):
    per, shared = MF.view_call()
    rows = NF.expected(nat, oracle, per)
    assert any(r["nodes"] > 0 for r in rows)
    check_tensors(of(ran, "views"), per, rows, "views")
    assert bool(ran["views/unchanged"]) and str(ran["views/kernels"]).split() == kernels_of(per)
    check_tensors(of(ran, "shared"), shared, NF.expected(nat, oracle, shared), "shared")
    assert ran["stream/A_ub"].tobytes() == per.stacked()[1].tobytes()  # (the producer had finished when the call read it)
    check_tensors(of(ran, "stream"), per, rows, "stream")
    assert ran["empty/shapes"].tolist() == [0, 3, 0, 0, 0, 0, 0] and int(ran["empty/launches"]) == 0


def test_refusals_name_the_entry_and_launch_nothing(ran, refs):
    msgs = [str(m) for m in ran["refusal/messages"]]
    for m, name in zip(msgs, ("lb", "ub")):
        assert "yalps_milpdense_solve_free: %s is " % name in m and ("this HIP runtime does not know" in m or "is host memory" in m), m
    assert "yalps_milpdense_solve_free: ub is host memory" in msgs[1], msgs[1]  # (pinned)
    assert "free_idx[0]: variable 1 is binary" in msgs[2] and "free_idx: variable 6 out of range" in msgs[3] and "not strictly ascending" in msgs[4], msgs[2:]
    assert all(m.endswith("launches=0") for m in msgs) and bool(ran["refusal/untouched"])
    check_tensors(of(ran, "refusal/after"), MF.table_call("binary rows and twins"), refs("binary rows and twins"), "after the refusals")


# ---------------------------------------------------------------------------------------------- the test hooks

def test_history_rerun_refills_the_split_tableau(tmp_path_factory, nat, oracle):
    """Under YALPS_MILPDENSE_HIST=4 every root outgrows its checkCycles history and runs again on the split tableau, refilled from the
    operands; so does every tree with a node of more pivots than that; the free epilogue runs after the last pass.  Bit for bit
    against the oracle-driven search."""
    got = run_child(tmp_path_factory, "hist", {"YALPS_MILPDENSE_HIST": str(MF.HIST)})
    call = MF.hist_call()
    rows = NF.expected(nat, oracle, call)
    check_tensors(got, call, rows, "hist")
    assert all(r["root_pivots"] > MF.HIST for r in rows) and any(r["nodes"] > 0 for r in rows)
    assert any((r["x_split"][call.n:] > 0.0).any() and (r["x"] < 0.0).any() for r in rows)  # (a twin is basic: x of a free variable is negative)
    long_trees = sum(any(node[4] > MF.HIST for node in r["trace"]) for r in rows)
    assert int(got["reruns"]) >= len(call.lps) + long_trees > len(call.lps) and int(got["passes"]) >= 2 and int(got["overflows"]) == 0
    kernels = str(got["kernels"]).split()
    assert all("check" in k for k in kernels if k != EPILOGUE) and kernels[-1] == EPILOGUE and kernels.count(EPILOGUE) == 1
    assert kernels[0] == root_kernel(call) == "milp_dense_free_root_kernel<256,check,lds>" and kernels.count(kernels[0]) >= 2


@pytest.fixture(scope="module")
def mix_rows(nat, oracle):
    return NF.expected(nat, oracle, MF.mix_call())


def test_one_workgroup_walks_many_trees(tmp_path_factory, mix_rows):
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_GRID": "1"}, "grid")
    check_tensors(got, MF.mix_call(), mix_rows, "grid 1")
    kernels, grids = str(got["kernels"]).split(), got["grids"].tolist()
    assert [g for k, g in zip(kernels, grids) if k.startswith("milp_tree_kernel")] == [1] and int(got["reruns"]) == 0
    assert kernels[0].startswith("milp_dense_free_root_kernel") and kernels[-1] == EPILOGUE


def test_arena_rerun_of_some_trees(tmp_path_factory, nat, oracle, mix_rows):
    """An arena of 2: the trees that outgrow it run again, the roots without a tree keep what the first pass wrote -- and the free
    epilogue, which runs after the last pass, reads both kinds."""
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_ARENA": "2"}, "arena")
    mix = MF.mix_call()
    check_tensors(got, mix, mix_rows, "arena 2")
    small = NF.expected(nat, oracle, mix, arena=2)
    assert int(got["reruns"]) == small[0]["reruns"] > 0
    assert int(got["passes"]) >= 2 and int(got["overflows"]) == 0
    assert 0 < len(set(got["rerun_trees"].tolist())) < len(mix.lps)


def test_overflow_is_answered_by_the_host_which_subtracts_the_halves(tmp_path_factory, nat, oracle, mix_rows):
    got = run_child(tmp_path_factory, "mix", {"YALPS_MILPDENSE_ARENA": "2", "YALPS_MILPDENSE_ARENA_MAX": "2"}, "overflow")
    mix = MF.mix_call()
    capped = NF.expected(nat, oracle, mix, arena=2, arena_max=2)
    over = {i for i, r in enumerate(capped) if r["status"] == "overflow"}
    assert 0 < len(over) < len(mix.lps) and int(got["overflows"]) == len(over)
    assert 5 not in got["status"].tolist()
    check_tensors(got, mix, mix_rows, "overflow", fallback=over)
    assert any((mix_rows[i]["x_split"][mix.n:] > 0.0).any() and (mix_rows[i]["x"] < 0.0).any() for i in over)  # (the host had halves to subtract)
