"""milp_batch_free(free=) and yalps_milpdense_solve_free without a GPU: the split MILP tableau against three references, the rules that
come from a free variable being integer, the argument checks of the library and of milp_batch_free, the package's host fallback, the
build, and the expectation the GPU tests use -- tests/_np_milp_dense_free.py -- against solve() of the equivalent models.  Last,
what makes the GPU table mean something: under every flaw of NF.FLAWS a named call of that table gets another expected answer."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _milp_dense_free as MF
from tests import _np_dense_bounds as BD
from tests import _np_dense_free as FD
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB
from tests import _np_milp_dense_free as NF
from tests.test_lp_batch import oracle_backend
from tests.test_milp_dense_bounds_model import FAKE, OPS, VEC, grid_lp, words
from tests.test_milp_dense_model import model_answer
from yalps_amd import model as M
from yalps_amd import solve as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = lambda *v: np.array(v, np.float64)


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native, build
    build.build_milpdense()
    build.build_milptree()
    build.build_lpdense()
    return _native


# ------------------------------------------------------------------------------------------------------------ the tableau

def sets(n):
    """(integers, binaries, free): a free integer, a free continuous, both, all free, True beside a binary."""
    last = n - 1
    out = [([0], (), [0]), ([0], (), [last]), ((), (), [0]), (True, (), True)]
    if n > 1:
        out += [([0, last], [last], [0]), ([last], [last], True), ([0], [last], [0]), ([0, last], (), [last, 0])]
    return out


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("mode", ("lb", "ub", "both", "none"))
@pytest.mark.parametrize("m_eq", (0, 2))
@pytest.mark.parametrize("m_ub", (0, 3))
@pytest.mark.parametrize("n", (1, 2, 5))
def test_free_milp_tableau_against_three_references(n, m_ub, m_eq, mode, maximize):
    from yalps_amd import milp_dense
    lp, lb, ub = grid_lp(n, m_ub, m_eq, "both", 0)
    lb, ub = (lb if mode in ("lb", "both") else None), (ub if mode in ("ub", "both") else None)
    for integers, binaries, free in sets(n):
        ints, bins = NM.sets_of(n, integers, binaries)
        fidx = NF.free_set(n, free, bins)
        for upper in ((True,) if ub is None else (True, (), tuple(fidx[:1]), tuple(j for j in range(n) if j not in bins and j not in fidx))):
            who = (n, m_ub, m_eq, mode, maximize, integers, binaries, free, upper)
            idx = NB.bound_rows(n, upper, ub is not None, bins)
            got, w, h, int_cols = NF.free_milp_tableau(lp, lb, ub, upper, free, integers, binaries, maximize)
            twins = [1 + n + t for t, j in enumerate(fidx) if j in ints]
            assert (w, h, got.size) == (1 + n + len(fidx), 1 + m_ub + 2 * m_eq + len(idx) + len(bins), w * h), who
            assert int_cols == [j + 1 for j in ints] + twins and int_cols == sorted(int_cols), who  # rule 4
            # tableauModel's matrix of the equivalent model in x'
            tm = M.tableau_model(NF.equivalent_model(lp, lb, ub, upper, free, integers, binaries, maximize))
            t = tm.tableau
            t.dense()
            assert (t.width, t.height) == (w, h) and np.array_equal(words(got), words(np.asarray(t.matrix[:w * h], np.float64))), who
            assert int_cols == list(tm.integers), who
            # the boundless tableau of the concatenated operands, its unit rows moved to their place
            ops, wide_ints, rows = NF.explicit_milp_operands(lp, lb, ub, upper, free, integers, binaries)
            explicit, ew, eh, ecols = NM.dense_milp_tableau(ops, wide_ints, binaries, maximize)
            assert (ew, eh, ecols) == (w, h, int_cols), who
            assert np.array_equal(words(got), words(explicit.reshape(h, w)[rows].ravel())), who
            # the package: what the host fallback packs
            mine = milp_dense.dense_tableau(*lp, binaries=bins, maximize=maximize, integers=ints, lb=lb, ub=ub, upper=idx, free=fidx)
            assert np.array_equal(words(got), words(mine)), who
            assert milp_dense.integer_columns(n, ints, fidx) == int_cols, who
            packed = milp_dense.packed_milp(lp, ints, bins, maximize, dict(S.default_options), lb=lb, ub=ub, upper=idx, free=fidx)
            row, col, val = LB.cells_of(got, w, h)
            assert packed[:2] == (w, h) and np.array_equal(packed[2], row) and np.array_equal(packed[3], col) and LB.same_words(packed[4], val)
            assert list(packed[5]) == int_cols, who
            # free=(): the bounded tableau, the bounded integer columns
            none = NF.free_milp_tableau(lp, lb, ub, upper, (), integers, binaries, maximize)
            want = NB.bounded_milp_tableau(lp, lb, ub, upper, integers, binaries, maximize)
            assert np.array_equal(words(none[0]), words(want[0])) and none[1:] == want[1:], who


# ---------------------------------------------------------------------------------------------------------------- the rules

def test_rule_1_the_twin_cells():
    lp = (f(1.0, -2.0, 0.0), np.array([[1.0, 0.0, -3.0]]), f(9.0), np.array([[2.0, -0.0, 1.0]]), f(4.0))
    m = NF.free_milp_tableau(lp, None, f(5.0, 6.0, 7.0), (1, 2), [1, 2], [1], [0], True)[0].reshape(7, 6)
    # twins of x1 and x2 behind the three originals: the negation of the cell, a zero's sign flipped, the equality pair flipped twice
    assert words(m[0])[4:].tolist() == words([2.0, -0.0]).tolist()
    assert words(m[1])[4:].tolist() == words([-0.0, 3.0]).tolist()
    assert words(m[2])[4:].tolist() == words([0.0, -1.0]).tolist() and words(m[3])[4:].tolist() == words([-0.0, 1.0]).tolist()
    # the bound rows of x1 and x2 carry -1.0 at their twins and +0.0 at the other's; the binary row of x0 +0.0 at both
    assert m[4].tolist() == [6.0, 0.0, 1.0, 0.0, -1.0, 0.0] and m[5].tolist() == [7.0, 0.0, 0.0, 1.0, 0.0, -1.0]
    assert words(m[6]).tolist() == words([1.0, 1.0, 0.0, 0.0, 0.0, 0.0]).tolist()


def test_rule_2_lb_is_not_read_at_a_free_variable():
    from yalps_amd import milp_dense
    lb = f(0.5, -1.5, math.nan, 0.25, 7.0)
    ints, bins, fidx = [0, 1, 4], [4], (1, 2)
    want = f(1.0, 0.0, 0.0, 0.25, 0.0)
    for got in (NF.effective_lower(lb, 5, ints, bins, fidx), milp_dense.effective_lower(lb, ints, bins, fidx)):
        assert np.array_equal(words(got), words(want)), got  # (+0.0, not ceil(-1.5) and not -0.0)
    assert milp_dense.effective_lower(None, ints, bins, fidx) is None and NF.effective_lower(None, 5, ints, bins, fidx) is None
    # the product with +0.0 is still formed: an infinite coefficient at a free column makes the right-hand side NaN
    lp = (f(1.0, 1.0), np.array([[math.inf, 1.0]]), f(3.0), None, None)
    for tab in (NF.free_milp_tableau(lp, f(7.0, 0.5), None, True, [0], [0], (), True)[0],
                milp_dense.dense_tableau(*lp, maximize=True, integers=[0], lb=f(7.0, 0.5), free=[0])):
        assert math.isnan(tab.reshape(2, 4)[1, 0]) and tab.reshape(2, 4)[1, 3] == -math.inf
    # NaN in lb at the free columns: the words of the clean tableau
    lp, lb, ub = grid_lp(5, 3, 1, "both", 1)
    dirty = lb.copy()
    dirty[[0, 3]] = math.nan
    a = NF.free_milp_tableau(lp, lb, ub, True, [0, 3], [0, 1], [4], True)[0]
    b = NF.free_milp_tableau(lp, dirty, ub, True, [0, 3], [0, 1], [4], True)[0]
    assert np.array_equal(words(a), words(b)) and not np.isnan(b).any()


def test_rule_3_a_binary_variable_cannot_be_free():
    from yalps_amd import milp_dense
    assert milp_dense.free_set([0, 1, 2, 3, 4], [1, 3], True) == [0, 2, 4] and NF.free_set(5, True, [1, 3]) == (0, 2, 4)
    assert milp_dense.free_set([0, 4], [1, 3], False) == [0, 4] and milp_dense.free_set([], [1], False) == []
    with pytest.raises(ValueError, match="free names variable 3, which is binary"):
        milp_dense.free_set([0, 3], [1, 3], False)
    with pytest.raises(ValueError):
        NF.free_set(5, (0, 3), [1, 3])


def test_rule_4_integer_columns_and_the_largest_node():
    from yalps_amd import milp_dense
    assert milp_dense.integer_columns(6, [1, 3, 4], [0, 3, 4, 5]) == [2, 4, 5, 8, 9] == NF.integer_columns(6, [1, 3, 4], (0, 3, 4, 5))
    assert milp_dense.integer_columns(6, [1, 3], ()) == [2, 4]
    base = milp_dense.largest_node_bytes(6, 2, 1, 3, 1, 2)
    assert base == 8 * 7 * (1 + 2 + 2 + 2 + 1 + 6)
    assert milp_dense.largest_node_bytes(6, 2, 1, 3, 1, 2, 4, 2) == 8 * (7 + 4) * (1 + 2 + 2 + 2 + 1 + 2 * (3 + 2))
    c = MF.table_call("binary rows and twins")
    assert (c.w, c.hmax, c.n_int_eff) == (1 + c.n + c.f, c.h + 2 * (len(c.ints) + c.int_twins), len(c.ints) + c.int_twins) and c.int_twins == 2


def test_host_fallback_subtracts_the_halves():
    from yalps_amd import milp_dense
    # n = 2, x1 free: w = 4; x0 basic in row 0, the twin (column 3) basic in row 2, x1 itself not basic
    c, low = f(2.0, -1.0), f(0.5, 0.0)
    col0, pos, var = f(-5.0, 2.5, 1.25), np.array([0, 4, 1, 6, 2, 5, 3], np.int32), np.array([0, 2, 4, 6, 1, 5, 3], np.int32)
    for status, result in (("optimal", -5.0), ("timedout", -5.0), ("timedout", math.nan), ("unbounded", 6.0), ("unbounded", 2.0), ("infeasible", math.nan)):
        mapped = status if status != "timedout" else ("optimal" if result == result else "infeasible")
        for lo in (low, None):
            want = FD.free_solution(col0, pos, var, mapped, result, 1.0, 1e-8, c, lb=lo, free=[1])
            got = milp_dense.dense_solution(col0, pos, var, status, result, 1.0, 1e-8, 2, c=c, low=lo, free=[1])
            assert np.array_equal(NM.words(got[0]), NM.words(want[0])) and np.array_equal(NM.words(got[1]), NM.words(want[1])), (status, result)
    x, obj = milp_dense.dense_solution(col0, pos, var, "optimal", -5.0, 1.0, 1e-8, 2, c=c, low=low, free=[1])
    assert x.tolist() == [0.0 + 0.5, 0.0 - 1.25] and obj == 5.0 + BD.shift_sum(c, low), x  # (x0 basic in row 0: -5 is not above precision)
    x, _ = milp_dense.dense_solution(col0, pos, var, "unbounded", 6.0, 1.0, 1e-8, 2, free=[1])
    assert x.tolist() == [0.0, -math.inf]  # (var[6] = 3: the twin's column)


# --------------------------------------------------------------------------------------------------------- argument checks

def test_validate_free_refuses_by_name(nat):
    V = nat.milpdense_validate_free
    V(2, 3, 2, 1, OPS, [0, 2], [2], lb=VEC, ub=VEC, upper=(0, 1), free=(0, 1))
    V(2, 3, 2, 1, OPS, [0, 2], [2], free=(1,))                        # no bounds
    V(2, 3, 2, 1, OPS, [0, 2], [2], lb=VEC, ub=VEC, upper=(0, 1))     # no free variable: yalps_milpdense_validate_bounds
    for kw, reason in ((dict(free=(2,)), "free_idx[0]: variable 2 is binary (a binary variable cannot be free)"),
                       (dict(free=(0, 3)), "yalps_milpdense: free_idx: variable 3 out of range"), (dict(free=(-1,)), "free_idx: variable -1 out of range"),
                       (dict(free=(1, 1)), "free_idx is not strictly ascending at variable 1"), (dict(free=(1, 0)), "not strictly ascending"),
                       (dict(free=(0,), upper=(0,)), "n_upper > 0 without ub"), (dict(free=(0,), lb=(None, 3, 1, 0)), "yalps_milpdense: lb is NULL")):
        with pytest.raises(nat.NativeError, match=re.escape(reason)):
            V(2, 3, 2, 1, OPS, [0, 2], [2], **kw)
    L = nat.milpdense_lib()
    assert L.yalps_milpdense_validate_free(2, 3, 2, 1, *[None] * 5, None, None, 0, None, -1, None, 0, None, 0, None) == -1
    assert b"free_idx: negative length" in L.yalps_milpdense_last_error()
    rc = L.yalps_milpdense_solve_free(None, 1, 1, 1, 0, *([None] * 5), None, None, 0, None, 0, None, 0, None, 0, None, 0, 1e-8, 8192.0, 0, 0.0, 1.0, 0,
                                      *([None] * 7))
    assert rc == -1 and L.yalps_milpdense_last_error() == b"yalps_milpdense_solve_free: handle is NULL"


def test_largest_node_counts_the_twins_and_their_cuts(nat):
    """w = 1024 with one twin: 512 rows of the largest node are 4 MiB exactly.  n = 1022, one free integer variable: two integer
    columns, four cuts."""
    V = nat.milpdense_validate_free
    ops = lambda m: ((FAKE, 1022, 1, 0), (FAKE, m * 1022, 1022, 1), (FAKE, m, 1, 0), None, None)
    V(1, 1022, 507, 0, ops(507), [5], free=(5,))
    text = ("yalps_milpdense: largest node of 513 x 1024 doubles (1 twin columns of free variables, 509 rows and two cuts for each of 2 integer "
            "columns: 1 integer variables and the twins of the 1 free ones among them) is above the limit of 4194304 bytes")
    with pytest.raises(nat.NativeError, match=re.escape(text)):
        V(1, 1022, 508, 0, ops(508), [5], free=(5,))
    V(1, 1022, 509, 0, ops(509), [5], free=(6,))   # (a free continuous variable: its twin is no integer column)
    with pytest.raises(nat.NativeError, match=re.escape("513 x 1024 doubles (1 twin columns of free variables, 511 rows and two cuts for each of 1 integer "
                                                        "columns: 1 integer variables and the twins of the 0 free ones")):
        V(1, 1022, 510, 0, ops(510), [5], free=(6,))


def test_milp_batch_checks_free_before_the_library(nat, monkeypatch):
    torch = pytest.importorskip("torch")
    from yalps_amd import tensors
    monkeypatch.setattr(nat, "MilpDense", lambda *a, **k: pytest.fail("the library was touched"))
    monkeypatch.setattr(nat, "milpdense_lib", lambda *a, **k: pytest.fail("the library was touched"))
    mine, base = inspect.signature(tensors.milp_batch_free).parameters, inspect.signature(tensors.milp_batch).parameters
    assert mine["free"].kind is inspect.Parameter.KEYWORD_ONLY and mine["free"].default == () and "free" not in base
    # milp_batch keeps its argument list; the sibling has the same one plus free, behind upper
    assert [k for k in mine if k != "free"] == list(base) and list(mine)[list(mine).index("free") - 1] == "upper"
    assert all(mine[k].kind is base[k].kind and mine[k].default == base[k].default for k in base)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    call = lambda **kw: tensors.milp_batch_free(z(3), z(2, 3), z(2), integers=[0, 2], binaries=[2], **kw)
    for kw, exc, text in ((dict(free=(0, 2)), ValueError, "milp_batch: free names variable 2, which is binary: a binary variable cannot be free"),
                          (dict(free=(1, 1)), ValueError, "milp_batch: free names variable 1 twice"),
                          (dict(free=(3,)), ValueError, "milp_batch: free names variable 3, outside 0 .. 2"),
                          (dict(free=(-1,)), ValueError, "outside 0 .. 2"),
                          (dict(free=(1.5,)), TypeError, "milp_batch: free holds 1.5"), (dict(free="01"), TypeError, "milp_batch: free must be a sequence"),
                          (dict(free=7), TypeError, "milp_batch: free must be"), (dict(free=(True,)), TypeError, "milp_batch: free holds True"),
                          (dict(free=True), ValueError, "a CPU tensor was given"), (dict(free=(0, 1)), ValueError, "a CPU tensor was given"),
                          (dict(free=None), ValueError, "a CPU tensor was given"), (dict(free=np.array([1, 0])), ValueError, "a CPU tensor was given")):
        with pytest.raises(exc, match=re.escape(text)):
            call(**kw)
    # the 4 MiB bound counts the twin column and the twin's two cuts, on both sides, and says so
    wide = lambda m: (z(1022), z(m, 1022), z(m))
    with pytest.raises(ValueError, match="a CPU tensor was given"):
        tensors.milp_batch_free(*wide(507), integers=[5], free=[5])
    with pytest.raises(ValueError, match=re.escape("milp_batch: the largest possible node, 513 x 1024 doubles (4202496 bytes: 1 twin columns of free "
                                                   "variables, 509 rows and two cuts for each of 2 integer columns -- 1 integer variables and the twins "
                                                   "of the 1 free ones among them), is above the batch limit of 4194304 bytes; solve() is")):
        tensors.milp_batch_free(*wide(508), integers=[5], free=[5])
    with pytest.raises(ValueError, match="a CPU tensor was given"):
        tensors.milp_batch_free(*wide(509), integers=[5], free=[6])
    with pytest.raises(ValueError, match=re.escape("513 x 1024 doubles")):
        tensors.milp_batch_free(*wide(510), integers=[5], free=[6])
    # without free variables the message is what it was
    with pytest.raises(ValueError, match=re.escape("milp_batch: the largest possible node, 513 x 1024 doubles (4202496 bytes: 511 rows and two cuts for "
                                                   "each of 1 integer variables), is above the batch limit")):
        tensors.milp_batch_free(z(1023), z(510, 1023), z(510), integers=[5], free=())
    for word in ("x[j] = p[j] - q[j]", "with no ceil", "a binary variable cannot be free", "n_int_eff = n_int + |free & integers|",
                 "8 (1 + n + f) (height + 2 n_int_eff)", "v(p) - v(q)", "milp_dense_free_root_kernel", "Out of scope: per-MILP sets"):
        assert word in tensors.milp_batch_free.__doc__, word
    assert "milp_batch_free" in tensors.milp_batch.__doc__


# ------------------------------------------------------------------------------------------------- the expectation itself

CPU_CALLS = MF.names()
FINITE = [n for n in CPU_CALLS if n != "NaN in lb at free"]
EXTRA = ("mix", "views", "shared", "concat", "no integers", "clean at free")


def call_of(name):
    return {"mix": MF.mix_call, "views": lambda: MF.view_call()[0], "shared": lambda: MF.view_call()[1], "concat": MF.concat_call,
            "no integers": MF.lp_call, "clean at free": MF.clean_call}.get(name, lambda: MF.table_call(name))()


@pytest.fixture(scope="module")
def refs(nat, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = NF.expected(nat, oracle, call_of(name))
        return made[name]
    return get


@pytest.mark.parametrize("name", CPU_CALLS + list(EXTRA))
def test_trees_are_small(refs, name):
    """The condition on the tables: every tree ends within NODE_LIMIT consumed nodes and fits the first arena."""
    rows = refs(name)
    assert max(r["nodes"] for r in rows) <= NM.NODE_LIMIT, (name, max(r["nodes"] for r in rows))
    assert rows[0]["reruns"] == 0 and "overflow" not in [r["status"] for r in rows], name


def split_answer(sol, call):
    """model_answer for a model with twins: x<j> at j, q<j> at n + t."""
    named = {"%s%d" % (k, j): int(k == "q") * (call.n + t) + int(k == "x") * j for k in "xq" for t, j in enumerate(call.fidx if k == "q" else range(call.n))}
    renamed = dict(sol, variables=[("x%d" % named[key], value) for key, value in sol["variables"]])
    return model_answer(renamed, call.n + call.f)


@pytest.mark.parametrize("name", FINITE + ["mix", "views", "concat", "no integers"])
def test_oracle_search_moved_back_equals_solve_of_the_equivalent_model(oracle, refs, name):
    call = call_of(name)
    rows = refs(name)
    one = oracle_backend(oracle)
    opt = dict(call.options, includeZeroVariables=True)
    for i, (model, row, low) in enumerate(zip(call.models(), rows, call.lows())):
        assert list(model["variables"]) == ["x%d" % j for j in range(call.n)] + ["q%d" % j for j in call.fidx]
        status, x, objective = split_answer(S._solve_with(one, model, opt), call)
        assert status == row["status"], (name, i, status, row["status"])
        assert np.array_equal(NM.words(x), NM.words(row["x_split"])), (name, i, x, row["x_split"])
        assert np.array_equal(NM.words(objective), NM.words(row["objective_shifted"])), (name, i, objective, row["objective_shifted"])
        with np.errstate(all="ignore"):  # moved back: one subtraction, one addition each
            back = x[:call.n].copy()
            back[list(call.fidx)] = back[list(call.fidx)] - x[call.n:]
            if low is not None:
                back, objective = back + low, np.float64(objective) + BD.shift_sum(call.lps[i][0], low)
        assert np.array_equal(NM.words(row["x"]), NM.words(back)) and np.array_equal(NM.words(row["objective"]), NM.words(objective)), (name, i)
        if call.exact and (row["status"] == "optimal" or (row["status"] == "timedout" and not math.isnan(row["result"]))):
            assert all(float(row["x"][j]).is_integer() for j in call.ints), (name, i, row["x"])


def test_table_reaches_its_endings(refs):
    E = refs
    down, call = E("negative optimum by the twin"), MF.table_call("negative optimum by the twin")
    assert [r["status"] for r in down] == ["optimal"] * 4 and [r["x"][0] for r in down] == [-2.0, -1.0, -1.0, -1.0] and all(r["nodes"] > 1 for r in down)
    # ... reached by a cut on the twin's column, 1 + n, and on no other way: the root leaves q0 at a fraction, p0 at zero
    assert call.fidx[0] == 0 and all(any(v == 1 + call.n for t in r["trace"] for _, v, _ in t[1]) for r in down)
    assert all(r["trace"][0][1][0][1] != 1 for r in down)
    tie = E("tie between a p and a q")
    assert all(r["status"] == "timedout" and math.isnan(r["result"]) and r["nodes"] == 12 for r in tie)
    assert [v for _, v, _ in tie[0]["trace"][0][1]] == [1]  # the first cut: column 1, p0 -- not column 4, q1, which ties with it
    fall = E("unbounded through a twin")
    assert [r["status"] for r in fall] == ["unbounded"] * 2 and all(r["x"][0] == -math.inf and r["objective"] == math.inf for r in fall)
    assert fall[0]["x"][1] == fall[0]["low"][1] == 0.0 and fall[0]["low"][0] == 0.0  # (+0.0 + l_eff: ceil(-0.25) at x1, +0.0 at the free x0)
    assert [r["status"] for r in E("infeasible row")] == ["infeasible", "optimal"]
    timed = E("timedout with a solution")
    assert all(r["status"] == "timedout" for r in timed) and any(not math.isnan(r["result"]) for r in timed)
    for name in CPU_CALLS:
        if name not in ("unbounded through a twin", "w = 32, all free"):  # (the latter's roots are integral: it is there for the fill)
            assert any(r["nodes"] > 0 for r in E(name)), name
    # negative values at free variables all over the table, among them integer ones
    for name in ["n=%d" % n for n in MF.LANES] + [e for e in MF.EDGES if e != "w = 34, f = 1"] + ["binary rows and twins", "mix"]:
        call = call_of(name)
        assert any(r["status"] in ("optimal", "timedout") and not math.isnan(r["result"]) and (r["x"][list(call.fidx)] < 0.0).any() for r in E(name)), name
    # a free variable with a bound row, lb elsewhere
    c = MF.table_call("free with a bound row, lb elsewhere")
    assert set(c.idx) & set(c.fidx) and set(c.idx) - set(c.fidx) and c.has_lb and any(lb[j] != 0.0 for lb in c.lbs for j in range(c.n) if j not in c.fidx)


def test_rule_2_on_the_expectation(nat, oracle, refs):
    dirty, clean = MF.table_call("NaN in lb at free"), MF.clean_call()
    assert all(np.isnan(lb[list(dirty.fidx)]).all() for lb in dirty.lbs)
    for a, b in zip(refs("NaN in lb at free"), refs("clean at free")):
        assert a["status"] == b["status"] and np.array_equal(words(a["x"]), words(b["x"])) and a["objective"] == b["objective"]
        assert a["trace"] == b["trace"] and not np.isnan(a["x"]).any()


def test_mix_reruns_and_overflows(nat, oracle, refs):
    mix = MF.mix_call()
    rows = refs("mix")
    assert sum(r["nodes"] > 2 for r in rows) >= 4 and [r["status"] for r in rows[6:]] == ["optimal", "infeasible"]
    again = NF.expected(nat, oracle, mix, arena=2)
    assert again[0]["reruns"] >= 3
    over = {i for i, r in enumerate(NF.expected(nat, oracle, mix, arena=2, arena_max=2)) if r["status"] == "overflow"}
    assert 0 < len(over) < len(mix.lps)
    # the host has halves to subtract in a tree it answers
    assert any((rows[i]["x_split"][mix.n:] > 0.0).any() for i in over)


def test_concatenated_route_is_the_same_milp(refs):
    call = MF.concat_call()
    assert all(r["status"] == "optimal" and float(r["objective"]).is_integer() for r in refs("concat")) and any(r["nodes"] > 0 for r in refs("concat"))
    assert call.f == 2 and not call.has_lb and call.has_ub


# ------------------------------------------------------------------------------------------------- every flaw shows

# flaw -> the calls of the GPU table whose expected answer it changes
TELLS = {
    "twin not integer": ("negative optimum by the twin", "w = 33, all free", "no bounds"),
    "ceil at a free integer": ("binary rows and twins", "n=64"),
    "lb read at a free variable": ("free with a bound row, lb elsewhere", "n=63", "NaN in lb at free"),
    "twins first in the integer list": ("tie between a p and a q",),
    "binary row with a twin cell": ("binary rows and twins", "n=129"),
    "sum of halves": ("negative optimum by the twin", "n=129", "w = 33, all free"),
    "twin +inf": ("unbounded through a twin",),
}


def answer_words(row):
    return np.concatenate([NM.words(row["x"]), NM.words(row["objective"]), NM.words(row["col0"]), NM.words(row["result"]),
                           np.array([NM.STATUS.index(row["status"]), row["nodes"], row["node_pivots"], row["root_pivots"]], np.int64)])


def changed(a, b):
    return not np.array_equal(answer_words(a), answer_words(b)) or a["trace"] != b["trace"]


@pytest.mark.parametrize("flaw", [k for k in NF.FLAWS if k not in NF.SHAPE_ONLY])
def test_every_flaw_changes_a_named_call(nat, oracle, refs, flaw):
    """What the GPU comparison compares bit for bit -- status, counts, result, column 0 of the best tableau, x, the objective, the
    node trace -- changes under the flaw in at least one row of each call TELLS names."""
    for name in TELLS[flaw]:
        call, rows = MF.table_call(name), refs(name)
        bad = NF.expected(nat, oracle, call.flawed(flaw))
        n = sum(changed(a, b) for a, b in zip(rows, bad))
        print("%s, %s: %d of %d rows change" % (flaw, name, n, len(rows)))
        assert n >= 1, (flaw, name)
        if flaw in NF.READ_FLAWS:  # (the read-out leaves the search alone)
            assert all(a["trace"] == b["trace"] and np.array_equal(NM.words(a["col0"]), NM.words(b["col0"])) for a, b in zip(rows, bad))


def test_hmax_without_the_twins_cuts_shows_in_the_kernel_names(nat, oracle, refs):
    """The oracle-driven search has no slices: hmax changes none of its answers, which is asserted.  What it changes is the size
    class of the tree pass -- the kernel the GPU table names -- and the room of a node with a cut on every integer column."""
    name = "256 to 1024 lanes by the twins' cuts"
    call = MF.table_call(name)
    bad = call.flawed("hmax without the twins' cuts")
    assert all(not changed(a, b) for a, b in zip(refs(name), NF.expected(nat, oracle, bad)))
    assert (LB.size_class(call.w, bad.hmax), LB.size_class(call.w, call.hmax)) == (2, 3)
    from tests.test_milp_dense import tree_kernel
    assert tree_kernel(bad) == "milp_tree_kernel<256,lds>" and tree_kernel(call) == "milp_tree_kernel<1024,lds>"
    assert call.hmax - bad.hmax == 2 * call.int_twins == 2


# ------------------------------------------------------------------------------------------------------ header and build

def test_header_declares_the_new_entries(nat):
    text = open(os.path.join(ROOT, "include", "yalps_milpdense.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", code))
    assert declared == set(nat.SYMBOLS_MILPDENSE) and {"yalps_milpdense_validate_free", "yalps_milpdense_solve_free"} <= declared
    lib = nat.milpdense_lib()
    assert all(hasattr(lib, s) for s in declared)
    for word in ("x[j] = p[j] - q[j]", "with no ceil", "a binary variable cannot be free", "n_int_eff = n_integers + |free & integers|",
                 "8 * (1 + n + n_free) * (height + 2 * n_int_eff)", "v(p) - v(q)", "With n_free = 0"):
        assert word in text, word


def test_build_lists_the_free_library():
    from yalps_amd import build
    assert os.path.basename(build.LIB_MILPDENSE_FREE) == "libyalps_milpdense_free.so" and callable(build.build_milpdense_free)
    assert "libyalps_milpdense_free.so" in build.__doc__
    assert "milp_dense_free_kernel.cuh" not in [os.path.basename(p) for p in build.HIP_DEPS]
    assert "milp_dense_free_kernel.cuh" in [os.path.basename(p) for p in build.MILPDENSE_FREE_DEPS]
    assert "milp_dense_free_kernel.cuh" in [os.path.basename(p) for p in build.MILPDENSE_DEPS]  # (milp_dense.hip includes its structs)
    assert {"milp_dense_free_root_kernel", "milp_dense_free_solution_kernel"} <= set(build.NO_SCRATCH)
    assert "milp_dense_free_root_kernel" in inspect.getsource(build.check_register_budgets)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libyalps_milpdense_free.so" in entry


def test_free_kernels_pass_the_register_budget(nat):
    """The six free root forms and the free epilogue are a code object of their own, under the build gate of their siblings: no
    scratch, no accumulator registers, within 128 VGPRs, static LDS a multiple of 16; the other two hold what they held."""
    from yalps_amd import build
    ks = build.check_register_budgets(build.LIB_MILPDENSE_FREE, min_resident=0)
    roots = {k: v for k, v in ks.items() if "milp_dense_free_root_kernel" in k}
    epilogue = {k: v for k, v in ks.items() if "milp_dense_free_solution_kernel" in k}
    assert len(roots) == 6 and len(epilogue) == 1 and len(ks) == 7, sorted(ks)
    for k, md in ks.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0 and int(md["vgpr_count"]) <= 128, (k, md)
    for k, md in roots.items():
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (k, md)
    mine = build.kernel_metadata(build.LIB_MILPDENSE)
    count = lambda tag: sum(tag in k for k in mine)
    assert (count("milp_dense_root_kernel"), count("milp_tree_kernel"), count("milp_dense_solution_kernel"), len(mine)) == (6, 6, 1, 13), sorted(mine)
    assert not any("bounds" in k or "free" in k for k in mine)
    theirs = build.kernel_metadata(build.LIB_MILPDENSE_BOUNDS)
    assert len(theirs) == 7 and not any("free" in k for k in theirs)
    import subprocess
    needed = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", build.LIB_MILPDENSE], capture_output=True, text=True, check=True).stdout
    assert "libyalps_milpdense_free.so" in needed and "libyalps_milpdense_bounds.so" in needed and "$ORIGIN" in needed
