"""libyalps_milpdense.so and milp_batch without a GPU: the tableau of a dense MILP against tableauModel's, the argument checks
of the library and of milp_batch, the package's host fallback, and the expectation the GPU tests use -- the oracle-driven search
of tests/_np_milp_dense.py -- against solve() of the equivalent models."""
import math
import os
import re

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _milp_dense as MD
from tests import _np_dense as ND
from tests import _np_milp_dense as NM
from tests.test_lp_batch import oracle_backend
from yalps_amd import model as M
from yalps_amd import solve as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = lambda *v: np.array(v, np.float64)


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native, build
    build.build_milpdense()
    build.build_milptree()
    return _native


def test_header_symbols_are_exported(nat):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yalps_milpdense.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", text))
    assert declared == set(nat.SYMBOLS_MILPDENSE), declared ^ set(nat.SYMBOLS_MILPDENSE)
    lib = nat.milpdense_lib()
    assert all(hasattr(lib, s) for s in declared)


def test_build_lists_the_new_library():
    from yalps_amd import build
    names = [os.path.basename(p) for p in build.HIP_DEPS]
    assert not {"milp_dense_kernel.cuh", "milp_tree_host.inc"} & set(names), names
    assert "milp_dense_root_kernel" in build.NO_SCRATCH
    deps = [os.path.basename(p) for p in build.MILPDENSE_DEPS]
    assert {"milp_dense_kernel.cuh", "milp_tree_host.inc", "milp_tree_kernel.cuh", "wg_queue.cuh"} <= set(deps)
    assert "milp_tree_host.inc" in [os.path.basename(p) for p in build.MILPTREE_DEPS]


def test_code_object_holds_the_three_kernels(nat):
    from yalps_amd import build
    ks = build.kernel_metadata(build.LIB_MILPDENSE)
    for kernel, forms in (("milp_dense_root_kernel", 6), ("milp_tree_kernel", 6), ("milp_dense_solution_kernel", 1)):
        mine = {k: v for k, v in ks.items() if kernel in k}
        assert len(mine) == forms, (kernel, sorted(mine))
        for k, v in mine.items():
            assert int(v["private_segment_fixed_size"]) == 0 and int(v["agpr_count"]) == 0, (k, v)
            if kernel != "milp_dense_solution_kernel":
                assert int(v["group_segment_fixed_size"]) % 16 == 0 and int(v["vgpr_count"]) <= 128, (k, v)
    assert not any("lp_batch_kernel" in k or "lp_dense_kernel" in k for k in ks), sorted(ks)
    # milp_tree_kernel is the same text in both libraries: the same registers and LDS
    tree = build.kernel_metadata(build.LIB_MILPTREE)
    keys = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")
    for k, v in ks.items():
        if "milp_tree_kernel" in k:
            assert {x: v[x] for x in keys} == {x: tree[k][x] for x in keys}, k


# ---------------------------------------------------------------------------------------------- the tableau

def small_lp(n, m_ub, m_eq, seed=0):
    rng = np.random.default_rng([20261020, n, m_ub, m_eq, seed])
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    return (ints(-3, 6, n), ints(-2, 5, m_ub, n) if m_ub else None, ints(-1, 8, m_ub) if m_ub else None,
            ints(-2, 5, m_eq, n) if m_eq else None, ints(0, 6, m_eq) if m_eq else None)


TABLEAU_CASES = [
    ("binaries only", small_lp(5, 3, 2), (), [4, 1], False),
    ("integers only", small_lp(5, 3, 2), [3, 0], (), True),
    ("both, one variable in both", small_lp(6, 2, 1), [1, 4], [4, 2, 5], False),
    ("True integers", small_lp(4, 2, 0), True, (), True),
    ("True binaries", small_lp(4, 2, 1), (), True, False),
    ("m_ub = 0", small_lp(3, 0, 2), [0], [2], False),
    ("m_eq = 0", small_lp(3, 2, 0), [2], [0], True),
    ("n = 1", small_lp(1, 1, 1), [0], [0], False),
    ("no rows at all", small_lp(2, 0, 0), (), [1], True),
    ("a minimised zero cost", (f(0.0, 2.0, 0.0), np.array([[1.0, 0.0, 2.0]]), f(3.0), None, None), [0, 2], [1], False),
]


@pytest.mark.parametrize("name,lp,integers,binaries,maximize", TABLEAU_CASES, ids=[c[0] for c in TABLEAU_CASES])
def test_tableau_equals_tableau_model(name, lp, integers, binaries, maximize):
    got, w, h, int_cols = NM.dense_milp_tableau(lp, integers, binaries, maximize)
    tm = M.tableau_model(NM.equivalent_milp_model(lp, integers, binaries, maximize))
    t = tm.tableau
    t.dense()
    assert (w, h) == (t.width, t.height), name
    assert LB.same_words(got, np.asarray(t.matrix[:w * h], np.float64)), name
    assert int_cols == list(tm.integers) and tm.sign == (1.0 if maximize else -1.0), (name, int_cols, tm.integers)
    n_bin = len(NM.sets_of(len(lp[0]), integers, binaries)[1])
    assert h == 1 + (0 if lp[2] is None else len(lp[2])) + 2 * (0 if lp[4] is None else len(lp[4])) + n_bin
    if name == "a minimised zero cost":  # -1 * 0.0 is -0.0, a written cell
        assert math.copysign(1.0, got[1]) == -1.0 and got[1] == 0.0 and math.copysign(1.0, got[0]) == 1.0


@pytest.mark.parametrize("name,lp,integers,binaries,maximize", TABLEAU_CASES, ids=[c[0] for c in TABLEAU_CASES])
def test_host_fallback_packs_the_same_tableau(nat, name, lp, integers, binaries, maximize):
    from yalps_amd import milp_dense
    ref, w, h, int_cols = NM.dense_milp_tableau(lp, integers, binaries, maximize)
    ints, bins = milp_dense.integer_sets(len(lp[0]), integers, binaries)
    assert (ints, bins) == NM.sets_of(len(lp[0]), integers, binaries)
    assert LB.same_words(milp_dense.dense_tableau(*lp, binaries=bins, maximize=maximize), ref)
    opt = dict(S.default_options, maxIterations=7.0, tolerance=0.25)
    milp = milp_dense.packed_milp(lp, ints, bins, maximize, opt)
    packed = nat.PackedMilps([milp])
    row, col, val = LB.cells_of(ref, w, h)
    assert (int(packed.lps.width[0]), int(packed.lps.height[0])) == (w, h)
    assert np.array_equal(packed.lps.row, row) and np.array_equal(packed.lps.col, col) and LB.same_words(packed.lps.val, val)
    assert packed.integers.tolist() == int_cols and packed.sign[0] == (1.0 if maximize else -1.0)
    assert (packed.tolerance[0], packed.max_iterations[0], packed.timeout[0]) == (0.25, 7.0, math.inf)
    nat.milptree_validate(packed)


def test_dense_solution_reads_a_timed_out_tree():
    from yalps_amd import milp_dense
    col0, pos, var = f(-5.0, 2.5, 1.0), np.array([0, 4, 2, 3, 1, 5], np.int32), np.array([0, 4, 2, 3, 1, 5], np.int32)
    for fn in (NM.dense_solution, milp_dense.dense_solution):
        x, obj = fn(col0, pos, var, "timedout", -5.0, 1.0, 1e-8, 2)
        assert x.tolist() == [2.5, 0.0] and obj == 5.0
        x, obj = fn(col0, pos, var, "timedout", math.nan, 1.0, 1e-8, 2)
        assert np.isnan(x).all() and math.isnan(obj)
        x, obj = fn(col0, pos, var, "unbounded", 4.0, -1.0, 1e-8, 2)
        assert x.tolist() == [math.inf, 0.0] and obj == -math.inf


# ---------------------------------------------------------------------------------------------- the argument checks

OPS = ((8, 3, 1, 0), (8, 6, 3, 1), (8, 2, 1, 0), (8, 3, 3, 1), (8, 1, 1, 0))  # B = 2, n = 3, m_ub = 2, m_eq = 1 (never dereferenced)


def refusal(nat, *args, **kw):
    with pytest.raises(nat.NativeError) as e:
        nat.milpdense_validate(*args, **kw)
    return str(e.value)


def test_validate_refuses_by_name(nat):
    nat.milpdense_validate(2, 3, 2, 1, OPS, [0, 2], [2])
    nat.milpdense_validate(0, 3, 2, 1, (None,) * 5, [0], [])
    nat.milpdense_validate(2, 3, 2, 1, OPS)
    assert "count < 0" in refusal(nat, -1, 3, 2, 1, OPS)
    assert "at least 0" in refusal(nat, 2, 3, -2, 1, OPS)
    for k, name in enumerate(("c", "A_ub", "b_ub", "A_eq", "b_eq")):
        bad = list(OPS)
        bad[k] = None
        assert "yalps_milpdense: %s is NULL" % name in refusal(nat, 2, 3, 2, 1, bad)
        bad[k] = (8, -1, 1, 0)
        assert "yalps_milpdense: %s: negative stride" % name in refusal(nat, 2, 3, 2, 1, bad)
    assert "integers: variable 3 out of range" in refusal(nat, 2, 3, 2, 1, OPS, [0, 3])
    assert "integers: variable -1 out of range" in refusal(nat, 2, 3, 2, 1, OPS, [-1])
    assert "binaries: variable 7 out of range" in refusal(nat, 2, 3, 2, 1, OPS, [0], [7])
    assert "integers is not strictly ascending at variable 1" in refusal(nat, 2, 3, 2, 1, OPS, [1, 1])
    assert "integers is not strictly ascending at variable 0" in refusal(nat, 2, 3, 2, 1, OPS, [2, 0])
    assert "binaries is not strictly ascending at variable 1" in refusal(nat, 2, 3, 2, 1, OPS, [1, 2], [2, 1])
    assert "binary variable 1 is not in integers" in refusal(nat, 2, 3, 2, 1, OPS, [0, 2], [1])


def test_largest_node_bound_on_both_sides(nat):
    """w = 1024: 512 rows of the largest node are 4 MiB exactly.  One integer variable (two cuts), then one binary (a row and two
    cuts)."""
    ops = lambda m: ((8, 1023, 1, 0), (8, m * 1023, 1023, 1), (8, m, 1, 0), None, None)
    nat.milpdense_validate(1, 1023, 509, 0, ops(509), [5])
    assert "largest node of 513 x 1024" in refusal(nat, 1, 1023, 510, 0, ops(510), [5])
    nat.milpdense_validate(1, 1023, 508, 0, ops(508), [5], [5])
    assert "above the limit of 4194304 bytes" in refusal(nat, 1, 1023, 509, 0, ops(509), [5], [5])
    nat.milpdense_validate(1, 1023, 511, 0, ops(511))  # (no integer variable: the tableau itself)
    assert "largest node" in refusal(nat, 1, 1023, 512, 0, ops(512))


def test_milp_batch_argument_checks():
    torch = pytest.importorskip("torch")
    from yalps_amd import tensors
    z = lambda *s: torch.zeros(s, dtype=torch.float64)
    c, A, b = z(4, 3), z(4, 2, 3), z(4, 2)
    cases = [(dict(integers=[0, 0]), ValueError, "integers names variable 0 twice"),
             (dict(binaries=[1, 2, 1]), ValueError, "binaries names variable 1 twice"),
             (dict(integers=[3]), ValueError, "integers names variable 3, outside 0 .. 2"),
             (dict(binaries=[-1]), ValueError, "binaries names variable -1, outside 0 .. 2"),
             (dict(integers=[0.5]), TypeError, "variable indices are integers"),
             (dict(integers=3), TypeError, "must be a sequence of variable indices or True")]
    for kw, exc, text in cases:
        with pytest.raises(exc, match=re.escape(text)):
            tensors.milp_batch(c, A, b, **kw)
    # what linprog_batch refuses, under this call's name
    with pytest.raises(TypeError, match="milp_batch: c is torch.float32"):
        tensors.milp_batch(c.float(), A, b)
    with pytest.raises(ValueError, match="milp_batch: A_ub and b_ub come together"):
        tensors.milp_batch(c, A)
    with pytest.raises(ValueError, match="milp_batch: the operands disagree about B"):
        tensors.milp_batch(c, z(5, 2, 3), b)
    with pytest.raises(ValueError, match="milp_batch: A_ub has 2 columns, c has 3 variables"):
        tensors.milp_batch(c, z(4, 2, 2), b)
    # CPU tensors: refused after the shape is known to fit, before the library is touched
    for kw in (dict(), dict(integers=[0, 1], binaries=[1]), dict(integers=True)):
        with pytest.raises(ValueError, match="milp_batch: the operands are read on the GPU where they lie: a CPU tensor was given"):
            tensors.milp_batch(c, A, b, **kw)
    # the 4 MiB bound on the largest node, on both sides (under it the call goes on to refuse the CPU tensors)
    wide = lambda m: (z(1023), z(m, 1023), z(m))
    with pytest.raises(ValueError, match="a CPU tensor was given"):
        tensors.milp_batch(*wide(509), integers=[5])
    with pytest.raises(ValueError, match=re.escape("milp_batch: the largest possible node, 513 x 1024 doubles (4202496 bytes: 511 rows and two "
                                                   "cuts for each of 1 integer variables), is above the batch limit of 4194304 bytes; solve() is")):
        tensors.milp_batch(*wide(510), integers=[5])
    with pytest.raises(ValueError, match="a CPU tensor was given"):
        tensors.milp_batch(*wide(508), binaries=[5])
    with pytest.raises(ValueError, match="the largest possible node"):
        tensors.milp_batch(*wide(509), binaries=[5])


def test_status_names_learns_timedout():
    pytest.importorskip("torch")
    from yalps_amd import tensors
    assert tensors.status_names([0, 1, 2, 3, 4]) == ["optimal", "infeasible", "unbounded", "cycled", "timedout"]
    with pytest.raises(IndexError):
        tensors.status_names([5])
    assert tensors.MilpBatchResult._fields == ("x", "objective", "status", "nodes", "node_pivots", "root_pivots")


# ---------------------------------------------------------------------------------------------- the expectation itself

def model_answer(sol, n):
    """solve()'s dict (includeZeroVariables) as (status, x[n], objective): NaN everywhere without a solution."""
    if sol["status"] != "unbounded" and math.isnan(sol["result"]):
        return sol["status"], np.full(n, math.nan), math.nan
    x = np.zeros(n, np.float64)
    for key, value in sol["variables"]:
        x[int(key[1:])] = value
    return sol["status"], x, sol["result"]


SOLVE_LIMIT = 48  # MILPs of a call that also go through solve() (the queue call: its first ones; they come from one generator)
CPU_CALLS = [n for n in MD.names() if n != "nonfinite"] + ["mix", "hist"]


def call_of(name):
    return {"mix": MD.mix_call, "hist": MD.hist_call}.get(name, lambda: MD.table_call(name))()


@pytest.mark.parametrize("name", CPU_CALLS + ["nonfinite"])
def test_trees_are_small(nat, oracle, name):
    """The condition on the tables: every tree ends within NODE_LIMIT consumed nodes and fits the first arena."""
    rows = NM.expected(nat, oracle, call_of(name))
    assert max(r["nodes"] for r in rows) <= NM.NODE_LIMIT, (name, max(r["nodes"] for r in rows))
    assert rows[0]["reruns"] == 0 and "overflow" not in [r["status"] for r in rows], name


@pytest.mark.parametrize("name", CPU_CALLS)
def test_oracle_search_equals_solve(nat, oracle, name):
    call = call_of(name)
    rows = NM.expected(nat, oracle, call)
    one = oracle_backend(oracle)
    opt = dict(call.options, includeZeroVariables=True)
    for i, (model, row) in enumerate(list(zip(call.models(), rows))[:SOLVE_LIMIT]):
        status, x, objective = model_answer(S._solve_with(one, model, opt), call.n)
        assert status == row["status"], (name, i, status, row["status"])
        assert np.array_equal(NM.words(x), NM.words(row["x"])), (name, i, x, row["x"])
        assert np.array_equal(NM.words(objective), NM.words(row["objective"])), (name, i, objective, row["objective"])


def test_table_reaches_its_endings(nat, oracle):
    E = lambda name: NM.expected(nat, oracle, call_of(name))
    assert [r["status"] for r in E("root infeasible")] == ["infeasible"] and E("root infeasible")[0]["nodes"] == 0
    r = E("root unbounded at the last variable")[0]
    assert r["status"] == "unbounded" and r["x"].tolist() == [0.0, 0.0, math.inf] and r["objective"] == math.inf
    assert [r["status"] for r in E("root cycled")] == ["cycled"] * 2
    r = E("root integral")[0]
    assert (r["status"], r["nodes"], r["height"]) == ("optimal", 0, 3)
    assert all(r["status"] == "optimal" and r["nodes"] > 2 and r["height"] > 9 for r in E("several nodes"))
    r = E("no integer point")[0]
    assert (r["status"], r["nodes"]) == ("infeasible", 2) and math.isnan(r["objective"])
    with_sol = E("timedout with a solution")
    assert all(r["status"] == "timedout" for r in with_sol) and not math.isnan(with_sol[0]["result"]) and with_sol[0]["height"] > 11
    assert all(r["status"] == "timedout" and math.isnan(r["result"]) and r["nodes"] == 1 for r in E("timedout without a solution"))
    exact = NM.expected(nat, oracle, MD.packing_call("exact", [(10, 10, 8, s) for s in (1, 2, 3)]))
    assert sum(r["nodes"] for r in E("tolerance")) < sum(r["nodes"] for r in exact)  # the search ends early
    assert E("maximize")[0]["objective"] != E("minimize")[0]["objective"]
    assert all(r["nodes"] > 0 for name in ("binaries only", "both sets, one variable in both", "binaries all n=65") for r in E(name))
    # the forced reruns: with an arena of 2 some trees of the mix run again and some do not; with a cap of 2 those overflow
    mix = MD.mix_call()
    again = NM.expected(nat, oracle, mix, arena=2)
    assert 0 < again[0]["reruns"] < len(mix.lps)
    over = [r["status"] for r in NM.expected(nat, oracle, mix, arena=2, arena_max=2)]
    assert 0 < over.count("overflow") < len(mix.lps)
    # the history rerun: roots, and in every tree a node, of more pivots than a history of HIST holds
    hist = NM.expected(nat, oracle, MD.hist_call())
    assert all(r["root_pivots"] > MD.HIST and max(t[4] for t in r["trace"]) > MD.HIST for r in hist)
    # class placement: a root in one class whose largest node falls in the next
    for k in range(4):
        c = call_of("under bound %d" % k)
        assert (LB.size_class(c.w, c.h), LB.size_class(c.w, c.hmax)) == (k, k + 1), (k, c.w, c.h, c.hmax)
    for k in (2, 3):
        c = call_of("over bound %d" % k)
        assert LB.size_class(c.w, c.h) == k + 1
    c = call_of("HBM odd n")
    assert LB.size_class(c.w, c.h) == 4 and c.n % 2 == 1
    from tests import _batch_shapes as BS
    c = call_of("aux form")
    assert BS.aux_hbm(c.w, c.hmax) and LB.size_class(c.w, c.h) == 4
