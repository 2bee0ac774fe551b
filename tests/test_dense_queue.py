"""The dense LP kernels with workgroups that take several LPs, on the GPU: every call of tests/_dense_queue.py twice, on a grid of
one workgroup (YALPS_LPDENSE_CUS=1, _PER_CU=1: the queue's order is the workgroup's order) and on a grid of two that share the
counter, and the checkCycles calls once more with a history of 4 pivots, whose reruns again find fewer workgroups than items.
Every item is compared with the C oracle word for word (tests/test_dense_queue_model.py shows what these words can tell):
status, pivots, x, the objective, the four marginals, column 0, both permutations and the kept matrix.  Then milp_batch: the `mix` and `hist`
calls of the three MILP families' own tables with the root pass on one workgroup, and the 30 MILP calls of tests/_dense_queue.py
-- every root form and every tree form -- with the roots on grids of 1 and 2 (YALPS_MILPDENSE_CUS, _PER_CU), with the trees on
one workgroup as well (YALPS_MILPDENSE_GRID=1), and the check calls under YALPS_MILPDENSE_HIST=4, against the oracle-driven search:
the six tensors, every tree's best tableau, and the node trace."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _dense_queue as Q
from tests.test_lp_dense import check_answers, of
from tests.test_lp_dense_bounds import check_marginals
from tests.test_milp_dense import HOOKS, check_tensors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP_HOOKS = HOOKS + ("YALPS_LPDENSE_HIST",)


def run_child(tmp_path_factory, which, tag, env):
    from yalps_amd import build
    build.build_lpdense()
    build.build_hip()
    path = str(tmp_path_factory.mktemp("dense_queue") / (tag + ".npz"))
    clean = {k: v for k, v in os.environ.items() if k not in LP_HOOKS}
    child = subprocess.run([sys.executable, "-m", "tests._dense_queue", which, path], cwd=ROOT, capture_output=True, text=True, timeout=300,
                           env=dict(clean, **env))
    assert child.returncode == 0, child.stderr[-4000:]
    return dict(np.load(path))


def grid_env(cus):
    return {"YALPS_LPDENSE_CUS": str(cus), "YALPS_LPDENSE_PER_CU": "1"}


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    return {cus: run_child(tmp_path_factory, "lp", "grid%d" % cus, grid_env(cus)) for cus in Q.GRIDS}


@pytest.fixture(scope="module")
def hist(tmp_path_factory):
    return run_child(tmp_path_factory, "lphist", "hist", dict(grid_env(1), YALPS_LPDENSE_HIST=str(Q.HIST)))


@pytest.fixture(scope="module")
def calls(oracle):
    return {c.name: c for c in Q.lp_calls(oracle)}


def check_call(got, call, oracle, tag):
    refs = check_answers(got, call, oracle, tag)  # status, pivots, x, objective, column 0, both permutations, the kept matrix
    check_marginals(got, call, refs, tag)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    return refs


@pytest.mark.parametrize("cus", Q.GRIDS)
@pytest.mark.parametrize("name", Q.lp_names())
def test_call_against_the_oracle(ran, calls, oracle, name, cus):
    call, got = calls[name], of(ran[cus], name)
    check_call(got, call, oracle, "%s grid %d" % (name, cus))
    kernels = str(got["q_kernels"]).split()
    assert kernels == [call.kernel] and got["q_classes"].tolist() == [call.cls] and got["q_aux"].tolist() == [call.aux], (name, kernels)
    assert got["q_grids"].tolist() == [cus] and got["q_items"].tolist() == [Q.ITEMS] and Q.ITEMS > cus  # every workgroup takes several
    assert int(got["q_reruns"]) == 0 and got["q_passes"].tolist() == [0]


@pytest.mark.parametrize("name", Q.lp_names())
def test_both_grids_leave_the_same_bits(ran, name):
    a, b = of(ran[Q.GRIDS[0]], name), of(ran[Q.GRIDS[1]], name)
    assert set(a) == set(b)
    for key in a:
        if key not in ("q_grids", "grids"):  # (the grid itself, twice; the children store no time)
            assert a[key].tobytes() == b[key].tobytes() and a[key].dtype == b[key].dtype, (name, key)


@pytest.mark.parametrize("name", [n for n in Q.lp_names() if n.endswith("check")])
def test_history_reruns_on_a_grid_of_one(hist, calls, oracle, name):
    """YALPS_LPDENSE_HIST=4 on one workgroup: the items whose phase outruns the history run again, in later passes that still hold
    more items than workgroups, over the slice of the history pool, the workspace and the output slots the pass before used."""
    call, got = calls[name], of(hist, name)
    refs = check_call(got, call, oracle, name + " hist")
    passes, items, grids, caps = (got[k].tolist() for k in ("q_passes", "q_items", "q_grids", "q_hist_caps"))
    assert set(str(got["q_kernels"]).split()) == {call.kernel} and "check" in call.kernel
    assert passes == list(range(len(passes))) and len(passes) >= 2 and grids == [1] * len(passes)
    assert caps == [Q.HIST * 4 ** p for p in passes], caps
    assert items[0] == Q.ITEMS and items[1] >= 2 and all(n >= 1 for n in items) and items[1] > grids[1]
    again = got["q_rerun_ids"].tolist()
    assert int(got["q_reruns"]) == len(again) == sum(items[1:]) >= 2
    assert len(set(again[:items[1]])) == items[1] < Q.ITEMS, "at least one item is not to overflow"
    assert all(refs[i]["n_pivots"] > Q.HIST for i in again)


def test_the_hooks_unset_leave_the_grid_alone(tmp_path_factory, calls, oracle):
    """No hook: a class-3 call of two LPs runs on two workgroups, one each, as before."""
    got = run_child(tmp_path_factory, "unset", "unset", {})
    call = Q.lp_call(oracle, "plain", "c3", False)
    call.lps, call.lbs, call.ubs = call.lps[:2], call.lbs[:2], call.ubs[:2]
    check_call(got, call, oracle, "unset")
    assert got["q_grids"].tolist() == [2] and got["q_items"].tolist() == [2] and got["q_classes"].tolist() == [3]


MILP_FAMILIES = {"plain": ("_milp_dense", "_np_milp_dense", "test_milp_dense", "milp_dense_root_kernel"),
                 "bounded": ("_milp_dense_bounds", "_np_milp_dense_bounds", "test_milp_dense_bounds", "milp_dense_bounds_root_kernel"),
                 "free": ("_milp_dense_free", "_np_milp_dense_free", "test_milp_dense_free", "milp_dense_free_root_kernel")}


@pytest.mark.parametrize("which", ("mix", "hist"))
@pytest.mark.parametrize("family", Q.FAMILIES)
def test_milp_roots_on_a_grid_of_one(tmp_path_factory, oracle, family, which):
    """YALPS_MILPDENSE_CUS=1, _PER_CU=1: one workgroup of each family's root kernel takes all roots of a call in turn -- `mix`: eight,
    an integral and an infeasible one among roots that branch, <256,lds>; `hist`: checkCycles under _HIST=4, every root runs again
    in a second pass of the same single workgroup, <256,check,lds> --; the trees keep the grid they had."""
    import importlib
    from yalps_amd import _native as nat
    helper, model, test, root = (importlib.import_module("tests." + m) if k < 3 else m for k, m in enumerate(MILP_FAMILIES[family]))
    env = {"YALPS_MILPDENSE_CUS": "1", "YALPS_MILPDENSE_PER_CU": "1"}
    if which == "hist":
        env["YALPS_MILPDENSE_HIST"] = str(helper.HIST)
    got = test.run_child(tmp_path_factory, which, env, "roots grid 1 " + which)
    call = helper.mix_call() if which == "mix" else helper.hist_call()
    rows = model.expected(nat, oracle, call)
    check_tensors(got, call, rows, "%s %s roots grid 1" % (family, which))
    kernels, grids = str(got["kernels"]).split(), got["grids"].tolist()
    form = "<256,check,lds>" if which == "hist" else "<256,lds>"
    roots = [g for k, g in zip(kernels, grids) if k.startswith(root)]
    assert kernels[0] == root + form and roots == [1] * len(roots) and len(call.lps) > 1
    if which == "mix":
        assert [g for k, g in zip(kernels, grids) if k.startswith("milp_tree_kernel")] == [len(call.lps)] and int(got["reruns"]) == 0
    else:
        long_roots = sum(r["root_pivots"] > helper.HIST for r in rows)  # (each outgrows its history: the second pass holds them all)
        assert len(roots) >= 2 and int(got["reruns"]) >= long_roots >= 2 and int(got["passes"]) >= 2


# ---------------------------------------------------------------------------------------------- the MILP calls
MILP_RUNS = {"roots grid 1": {"YALPS_MILPDENSE_CUS": "1", "YALPS_MILPDENSE_PER_CU": "1"},
             "roots grid 2": {"YALPS_MILPDENSE_CUS": "2", "YALPS_MILPDENSE_PER_CU": "1"},
             "roots and trees grid 1": {"YALPS_MILPDENSE_CUS": "1", "YALPS_MILPDENSE_PER_CU": "1", "YALPS_MILPDENSE_GRID": "1"}}
MILP_HIST = dict(MILP_RUNS["roots and trees grid 1"], YALPS_MILPDENSE_HIST=str(Q.HIST))


def run_milp_child(tmp_path_factory, which, tag, env):
    from yalps_amd import build
    for make in (build.build_milpdense, build.build_hip):
        make()
    path = str(tmp_path_factory.mktemp("dense_queue_milp") / (tag.replace(" ", "_") + ".npz"))
    clean = {k: v for k, v in os.environ.items() if k not in LP_HOOKS}
    child = subprocess.run([sys.executable, "-m", "tests._dense_queue", which, path], cwd=ROOT, capture_output=True, text=True, timeout=300,
                           env=dict(clean, **env))
    assert child.returncode == 0, child.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def milp_ran(tmp_path_factory):
    return {tag: run_milp_child(tmp_path_factory, "milp", tag, env) for tag, env in MILP_RUNS.items()}


@pytest.fixture(scope="module")
def milp_hist(tmp_path_factory):
    return run_milp_child(tmp_path_factory, "milphist", "hist", MILP_HIST)


@pytest.fixture(scope="module")
def milp_calls():
    return {c.name: c for c in Q.milp_calls()}


def check_milp(got, call, oracle, tag):
    """The six tensors, every tree's status, result and best tableau, and the trace against the oracle's node sequence."""
    import json
    from yalps_amd import _native as nat
    from tests.test_milp_dense import check_trees
    rows = Q.milp_rows(nat, oracle, call)
    check_tensors(got, call, rows, tag)
    check_trees(got, call, rows, tag)
    traces = json.loads(str(got["traces"]))
    assert len(traces) == len(rows)
    for i, (seen, row) in enumerate(zip(traces, rows)):
        want = row["trace"][:24]
        assert len(seen) == len(want), (tag, i, len(seen), len(want))
        for k, (g, w) in enumerate(zip(seen, want)):
            assert (g[0], tuple(tuple(c) for c in g[1]), g[2], g[3], g[4], g[5]) == tuple(w), (tag, i, k, g, w)
    assert bool(got["unchanged"]) and int(got["overflows"]) == 0, tag
    return rows


def launches_of(got, prefix):
    kernels = str(got["q_kernels"]).split()
    return [(k, int(got["q_grids"][j]), int(got["q_items"][j]), int(got["q_passes"][j]), int(got["q_hist_caps"][j]), int(got["q_classes"][j]))
            for j, k in enumerate(kernels) if k.startswith(prefix)]


@pytest.mark.parametrize("tag", list(MILP_RUNS))
@pytest.mark.parametrize("name", Q.milp_names())
def test_milp_call_against_the_oracle_search(milp_ran, milp_calls, oracle, name, tag):
    call, got = milp_calls[name], of(milp_ran[tag], name)
    check_milp(got, call, oracle, "%s, %s" % (name, tag))
    cus = int(MILP_RUNS[tag]["YALPS_MILPDENSE_CUS"])
    roots, trees = launches_of(got, Q.MILP_ROOT[call.family]), launches_of(got, "milp_tree_kernel")
    assert [(r[0], r[1], r[2], r[3], r[5]) for r in roots] == [(call.root_kernel, cus, Q.ITEMS, 0, call.cls)] and Q.ITEMS > cus, (name, roots)
    assert [t[0] for t in trees] == [call.tree_kernel] * len(trees) and [t[5] for t in trees] == [call.tree_cls] * len(trees) and trees, (name, trees)
    if "YALPS_MILPDENSE_GRID" in MILP_RUNS[tag]:  # one workgroup walks the call's trees in turn
        assert all(t[1] == 1 for t in trees) and trees[0][2] == Q.ITEMS, (name, trees)
    else:                                         # the trees keep the grid they had
        assert all(t[1] == t[2] for t in trees) and trees[0][2] == Q.ITEMS, (name, trees)
    assert str(got["q_kernels"]).split()[-1] == Q.MILP_EPILOGUE[call.family]


@pytest.mark.parametrize("name", Q.milp_names())
def test_milp_grids_leave_the_same_bits(milp_ran, name):
    first = of(milp_ran["roots grid 1"], name)
    for tag in ("roots grid 2", "roots and trees grid 1"):
        other = of(milp_ran[tag], name)
        assert set(first) == set(other)
        for key in first:
            if key not in ("q_grids", "grids"):
                assert first[key].tobytes() == other[key].tobytes(), (name, tag, key)


@pytest.mark.parametrize("name", [n for n in Q.milp_names() if n.endswith("check")])
def test_milp_history_reruns_on_grids_of_one(milp_hist, milp_calls, oracle, name):
    """YALPS_MILPDENSE_HIST=4 with one workgroup for the roots and one for the trees: every root of more than 4 pivots in a phase runs
    again in a pass that still holds more roots than workgroups; so do the trees with such a node."""
    call, got = milp_calls[name], of(milp_hist, name)
    rows = check_milp(got, call, oracle, name + " hist")
    roots, trees = launches_of(got, Q.MILP_ROOT[call.family]), launches_of(got, "milp_tree_kernel")
    assert {r[0] for r in roots} == {call.root_kernel} and {t[0] for t in trees} == {call.tree_kernel}
    assert [r[3] for r in roots] == list(range(len(roots))) and len(roots) >= 2 and all(r[1] == 1 for r in roots) and all(t[1] == 1 for t in trees)
    assert [r[4] for r in roots] == [Q.HIST * 4 ** r[3] for r in roots], roots
    assert roots[0][2] == Q.ITEMS and roots[1][2] >= 2 and roots[1][2] > roots[1][1]
    assert int(got["q_reruns"]) >= 2 and sum(r["root_pivots"] > Q.HIST for r in rows) >= roots[1][2]


def test_every_milp_form_was_seen(milp_ran, milp_hist):
    """Equality, not inclusion: the root and tree spellings the launches report are the 18 + 6 the model test counted."""
    seen = {k for out in (*milp_ran.values(), milp_hist) for key, v in out.items() if key.endswith("/q_kernels") for k in str(v).split()}
    roots, trees = Q.milp_spellings()
    assert seen - set(Q.MILP_EPILOGUE.values()) == roots | trees and len(roots) == 18 and len(trees) == 6, sorted(seen ^ (roots | trees))


def test_every_form_was_seen(ran, hist):
    """Equality, not inclusion: the spellings the children's launches report, over all calls, are the 18 the model test counted."""
    seen = {k for out in (*ran.values(), hist) for key, v in out.items() if key.endswith("/q_kernels") for k in str(v).split()}
    assert seen == Q.lp_spellings() and len(seen) == 18, sorted(seen ^ Q.lp_spellings())
