"""milp_batch(lb=, ub=, upper=) and yalps_milpdense_solve_bounds without a GPU: the bounded MILP tableau against three references,
the three rules that come from the variables being integer, the argument checks of the library and of milp_batch, the package's
host fallback, the build, and the expectation the GPU tests use -- tests/_np_milp_dense_bounds.py -- against solve() of the
equivalent models."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _milp_dense_bounds as MDB
from tests import _np_dense as ND
from tests import _np_dense_bounds as BD
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB
from tests.test_lp_batch import oracle_backend
from tests.test_milp_dense_model import model_answer
from yalps_amd import model as M
from yalps_amd import solve as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = lambda *v: np.array(v, np.float64)
MODES = ("lb", "ub", "both")


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native, build
    build.build_milpdense()
    build.build_milptree()
    build.build_lpdense()
    return _native


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------ the tableau

def grid_lp(n, m_ub, m_eq, mode, seed):
    from tests.test_lp_dense_model import random_lp
    rng = np.random.default_rng([20261305, n, m_ub, m_eq, MODES.index(mode), seed])
    lp = random_lp(rng, n, m_ub, m_eq)
    lb = rng.integers(-6, 5, n).astype(np.float64) * 0.25 if mode != "ub" else None  # (quarters: fractional at integer variables)
    ub = rng.integers(-4, 9, n).astype(np.float64) * 0.5 if mode != "lb" else None
    return lp, lb, ub


def sets(n):
    """(integers, binaries): integers only, binaries only, both, a variable in both, True."""
    return [([0], ()), ((), [n - 1]), ([0], [n - 1]), ([n - 1, 0], [0]), (True, ()), ((), True)]


def uppers(n, mode, bins):
    free = [j for j in range(n) if j not in bins]
    return (True,) if mode == "lb" else (True, (), tuple(free[:1]), tuple(free[-1:]), tuple(reversed(free)))


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m_eq", (0, 1, 2))
@pytest.mark.parametrize("m_ub", (0, 3))
@pytest.mark.parametrize("n", (1, 2, 5))
def test_bounded_milp_tableau_against_three_references(n, m_ub, m_eq, mode, maximize):
    from yalps_amd import milp_dense
    lp, lb, ub = grid_lp(n, m_ub, m_eq, mode, 0)
    for integers, binaries in sets(n):
        ints, bins = NM.sets_of(n, integers, binaries)
        for upper in uppers(n, mode, bins):
            who = (n, m_ub, m_eq, mode, maximize, integers, binaries, upper)
            idx = NB.bound_rows(n, upper, ub is not None, bins)
            got, w, h, int_cols = NB.bounded_milp_tableau(lp, lb, ub, upper, integers, binaries, maximize)
            assert (w, h, got.size) == (n + 1, 1 + m_ub + 2 * m_eq + len(idx) + len(bins), (n + 1) * h), who
            # tableauModel's matrix of the equivalent model in x'
            tm = M.tableau_model(NB.equivalent_model(lp, lb, ub, upper, integers, binaries, maximize))
            t = tm.tableau
            t.dense()
            assert (t.width, t.height) == (w, h) and np.array_equal(words(got), words(np.asarray(t.matrix[:w * h], np.float64))), who
            assert int_cols == list(tm.integers), who
            # the boundless tableau of the explicitly built operands, its unit rows moved to their place
            ops, rows = NB.explicit_milp_operands(lp, lb, ub, upper, integers, binaries)
            explicit = NM.dense_milp_tableau(ops, integers, binaries, maximize)[0].reshape(h, w)
            assert np.array_equal(words(got), words(explicit[rows].ravel())), who
            # the package: what the host fallback packs
            mine = milp_dense.dense_tableau(*lp, binaries=bins, maximize=maximize, integers=ints, lb=lb, ub=ub, upper=idx)
            assert np.array_equal(words(got), words(mine)), who
            packed = milp_dense.packed_milp(lp, ints, bins, maximize, dict(S.default_options), lb=lb, ub=ub, upper=idx)
            row, col, val = LB.cells_of(got, w, h)
            assert packed[:2] == (w, h) and np.array_equal(packed[2], row) and np.array_equal(packed[3], col) and LB.same_words(packed[4], val)
            assert list(packed[5]) == int_cols, who


# --------------------------------------------------------------------------------------------------------- the three rules

def test_rule_1_the_effective_lower_bound():
    from yalps_amd import milp_dense
    lb = f(0.5, -0.5, -1.5, 0.25, -0.0, math.nan, math.inf, -math.inf, 2.0, 1e300, 0.75)
    ints, bins = list(range(10)), [10]
    want = f(1.0, -0.0, -1.0, 1.0, -0.0, math.nan, math.inf, -math.inf, 2.0, 1e300, 0.0)
    for got in (NB.effective_lower(lb, 11, ints + bins, bins), milp_dense.effective_lower(lb, ints + bins, bins)):
        assert np.array_equal(NM.words(got), NM.words(want)), got
        assert words(got[1:2])[0] == words([-0.0])[0] and words(got[10:])[0] == 0  # ceil(-0.5) is -0.0; a binary is +0.0
    assert np.array_equal(words(NB.effective_lower(lb[:5], 5, [], [])), words(lb[:5]))  # continuous: as it lies
    assert NB.effective_lower(None, 3, [0], []) is None and milp_dense.effective_lower(None, [0], []) is None
    # in the tableau: the bound row holds ub - ceil(lb), the right-hand side moves by the row's sum with ceil(lb)
    lp = (f(1.0, 1.0, 1.0), np.array([[2.0, 3.0, 5.0]]), f(20.0), None, None)
    m = NB.bounded_milp_tableau(lp, f(0.5, -0.5, -1.5), f(4.0, 4.0, 4.0), True, [0, 1, 2], (), True)[0].reshape(5, 4)
    assert m[1, 0] == 20.0 - (2.0 * 1.0 + 3.0 * -0.0 + 5.0 * -1.0) and m[2:, 0].tolist() == [3.0, 4.0, 5.0]
    m = NB.bounded_milp_tableau(lp, f(0.5, -0.5, -1.5), f(4.0, 4.0, 4.0), True, (), (), True)[0].reshape(5, 4)
    assert m[1, 0] == 20.0 - (1.0 - 1.5 - 7.5) and m[2:, 0].tolist() == [3.5, 4.5, 5.5]
    # the product with +0.0 at a binary column is still formed: an infinite coefficient there gives NaN
    lp = (f(1.0, 1.0), np.array([[math.inf, 1.0]]), f(3.0), None, None)
    for tab in (NB.bounded_milp_tableau(lp, f(7.0, 0.5), None, True, (), [0], True)[0],
                milp_dense.dense_tableau(*lp, binaries=[0], maximize=True, integers=[0], lb=f(7.0, 0.5))):
        assert math.isnan(tab[3])


def test_rule_2_binaries_have_no_bound_row():
    from yalps_amd import milp_dense
    lp, lb, ub = grid_lp(5, 3, 1, "both", 1)
    clean = NB.bounded_milp_tableau(lp, lb, ub, True, [0], [1, 3], True)
    lbp, ubp = lb.copy(), ub.copy()
    lbp[[1, 3]], ubp[[1, 3]] = math.nan, math.nan
    poisoned = NB.bounded_milp_tableau(lp, lbp, ubp, True, [0], [1, 3], True)
    assert np.array_equal(words(clean[0]), words(poisoned[0])) and not np.isnan(poisoned[0]).any()
    mine = milp_dense.dense_tableau(*lp, binaries=[1, 3], maximize=True, integers=[0, 1, 3], lb=lbp, ub=ubp, upper=[0, 2, 4])
    assert np.array_equal(words(mine), words(clean[0]))
    # upper=True: every variable that is not binary
    assert NB.bound_rows(5, True, True, [1, 3]) == (0, 2, 4) and clean[2] == 1 + 3 + 2 + (5 - 2) + 2
    assert milp_dense.bound_rows([0, 1, 2, 3, 4], [1, 3], True) == [0, 2, 4] and milp_dense.bound_rows([], [1, 3], True) == []
    assert milp_dense.bound_rows([0, 4], [1, 3], False) == [0, 4]
    with pytest.raises(ValueError, match="variable 3, which is binary"):
        milp_dense.bound_rows([0, 3], [1, 3], False)
    with pytest.raises(ValueError):
        NB.bound_rows(5, (0, 3), True, [1, 3])


def test_rule_3_row_order():
    lp = (f(1.0, 2.0, 3.0), np.array([[1.0, 1.0, 1.0]]), f(9.0), np.array([[1.0, 0.0, 1.0]]), f(4.0))
    m = NB.bounded_milp_tableau(lp, f(1.0, 0.0, 0.5), f(3.0, 9.0, 2.5), (2, 0), [0], [1], True)[0].reshape(7, 4)
    assert m[4].tolist() == [2.0, 1.0, 0.0, 0.0] and m[5].tolist() == [2.0, 0.0, 0.0, 1.0]  # the bound rows, ascending: x0, x2
    assert m[6].tolist() == [1.0, 0.0, 1.0, 0.0]                                              # then the binary row of x1
    assert m[1, 0] == 9.0 - 1.5 and m[2, 0] == 4.0 - 1.5 and m[3, 0] == -(4.0 - 1.5)


def test_package_shift_sum_is_the_pinned_order():
    """yalps_amd.milp_dense.shift_sum against both statements of the order in tests/_np_dense_bounds.py, on the rows that pin it
    (tests/test_lp_dense_bounds_model.py::test_shift_sum_order_is_pinned) and on random rows of every lane count."""
    from yalps_amd.milp_dense import shift_sum
    one, e = np.ones(65), 1.0 + 2.0 ** -30
    rows = []
    a = np.zeros(65)
    a[0], a[64], a[1] = 1e16, 1.0, -1e16
    rows.append((a, one, 0.0))
    for v, want in (((1e16, -1e16, 1.0), 1.0), ((1e16, 1.0, -1e16), 0.0)):
        b = np.zeros(64)
        b[0], b[32], b[16] = v
        rows.append((b, np.ones(64), want))
    rows.append((f(e, 1.0), f(e, -(1.0 + 2.0 ** -29)), 0.0))
    a, l = np.zeros(65), np.ones(65)
    a[0], l[0], a[64], l[64] = 1.0, -(1.0 + 2.0 ** -29), e, e
    rows.append((a, l, 0.0))
    d = np.zeros(65)
    d[0], d[32], d[64] = 1e16, -1e16, 1.0
    rows.append((d, one, 0.0))
    rows += [(f(), f(), 0.0), (f(-0.0), f(1.0), 0.0)]
    for a, l, want in rows:
        got = shift_sum(a, l)
        assert words([got])[0] == words([BD.shift_sum(a, l)])[0] == words([BD.shift_sum_lanes(a, l)])[0] == words([want])[0], (a, l, got)
    rng = np.random.default_rng(20261306)
    for n in (1, 2, 63, 64, 65, 128, 129, 300):
        a, l = rng.standard_normal(n) * 1e3, rng.standard_normal(n)
        assert words([shift_sum(a, l)])[0] == words([BD.shift_sum(a, l)])[0] == words([BD.shift_sum_lanes(a, l)])[0], n
    assert math.isnan(shift_sum(f(math.inf, 1.0), f(0.0, 1.0))) and shift_sum(f(1.5e308, 1.5e308), f(1.0, 1.0)) == math.inf
    for flaw in BD.SUM_FLAWS:  # (and it is none of the wrong orders)
        assert any(words([shift_sum(a, l)])[0] != words([BD.flawed_shift_sum(a, l, flaw)])[0] for a, l, _ in rows), flaw


def test_host_fallback_moves_the_answer_back():
    from yalps_amd import milp_dense
    c, low = f(2.0, -1.0, 0.5), f(1.0, -0.0, 0.3)
    col0, pos, var = f(-5.0, 2.5, 1.0), np.array([0, 4, 2, 5, 1, 3], np.int32), np.array([0, 4, 2, 5, 1, 3], np.int32)
    for status, result in (("optimal", -5.0), ("timedout", -5.0), ("timedout", math.nan), ("unbounded", 4.0), ("infeasible", math.nan)):
        mapped = status if status != "timedout" else ("optimal" if result == result else "infeasible")
        want = BD.bounded_solution(col0, pos, var, mapped, result, 1.0, 1e-8, c, low)
        got = milp_dense.dense_solution(col0, pos, var, status, result, 1.0, 1e-8, 3, c=c, low=low)
        assert np.array_equal(NM.words(got[0]), NM.words(want[0])) and np.array_equal(NM.words(got[1]), NM.words(want[1])), status
    x, obj = milp_dense.dense_solution(col0, pos, var, "optimal", -5.0, 1.0, 1e-8, 3, c=c, low=low)
    assert x.tolist() == [0.0 + 1.0, 0.0, 2.5 + 0.3] and obj == 5.0 + BD.shift_sum(c, low)  # (w = 4: x0 is basic in row 0, x2 in row 1)
    x, _ = milp_dense.dense_solution(col0, pos, var, "unbounded", 4.0, 1.0, 1e-8, 3, c=c, low=low)
    assert x.tolist() == [math.inf, 0.0, 0.3]
    assert milp_dense.largest_node_bytes(3, 2, 1, 2, 1) + 8 * 4 * 5 == milp_dense.largest_node_bytes(3, 2, 1, 2, 1, 5)


# --------------------------------------------------------------------------------------------------------- argument checks

FAKE = 4096  # a pointer value no check dereferences
OPS = ((FAKE, 3, 1, 0), (FAKE, 6, 3, 1), (FAKE, 2, 1, 0), (FAKE, 3, 3, 1), (FAKE, 1, 1, 0))  # B = 2, n = 3, m_ub = 2, m_eq = 1
VEC = (FAKE, 3, 1, 0)


def test_validate_bounds_refuses_by_name(nat):
    V = nat.milpdense_validate_bounds
    V(2, 3, 2, 1, OPS, [0, 2], [2], lb=VEC, ub=VEC, upper=(0, 1))
    V(2, 3, 2, 1, OPS, [0, 2], [2])                                  # no bounds: yalps_milpdense_validate
    V(2, 3, 2, 1, OPS, [0], [], ub=(None, 0, 0, 0))                   # ub without a listed variable is never read
    for kw, reason in ((dict(lb=(FAKE, 3, -1, 0)), "yalps_milpdense: lb: negative stride"), (dict(ub=(FAKE, -3, 1, 0), upper=(0,)), "ub: negative stride"),
                       (dict(lb=(None, 3, 1, 0)), "yalps_milpdense: lb is NULL"), (dict(ub=(None, 3, 1, 0), upper=(1,)), "yalps_milpdense: ub is NULL"),
                       (dict(ub=VEC, upper=(0, 3)), "upper_idx[1] = 3 is outside 0 .. n-1"), (dict(ub=VEC, upper=(-1,)), "outside 0 .. n-1"),
                       (dict(ub=VEC, upper=(1, 1)), "upper_idx is not ascending at 1"), (dict(ub=VEC, upper=(1, 0)), "not ascending"),
                       (dict(upper=(0,)), "n_upper > 0 without ub"),
                       (dict(ub=VEC, upper=(0, 2)), "upper_idx[1]: variable 2 is binary")):
        with pytest.raises(nat.NativeError, match=re.escape(reason)):
            V(2, 3, 2, 1, OPS, [0, 2], [2], **kw)
    # what yalps_milpdense_validate refuses, through this entry too
    with pytest.raises(nat.NativeError, match="binary variable 1 is not in integers"):
        V(2, 3, 2, 1, OPS, [0, 2], [1], lb=VEC)
    L = nat.milpdense_lib()
    rc = L.yalps_milpdense_solve_bounds(None, 1, 1, 1, 0, *([None] * 5), None, None, 0, None, 0, None, 0, None, 0, 1e-8, 8192.0, 0, 0.0, 1.0, 0,
                                        *([None] * 7))
    assert rc == -1 and L.yalps_milpdense_last_error() == b"yalps_milpdense_solve_bounds: handle is NULL"


def test_largest_node_counts_the_bound_rows(nat):
    """w = 1024: 512 rows of the largest node are 4 MiB exactly.  One integer variable (two cuts) and k bound rows."""
    V = nat.milpdense_validate_bounds
    ops = lambda m: ((FAKE, 1023, 1, 0), (FAKE, m * 1023, 1023, 1), (FAKE, m, 1, 0), None, None)
    wide = (FAKE, 0, 1, 0)
    V(1, 1023, 409, 0, ops(409), [5], ub=wide, upper=range(100))
    with pytest.raises(nat.NativeError, match=re.escape("largest node of 513 x 1024 doubles (511 rows and two cuts for each of 1 integer")):
        V(1, 1023, 410, 0, ops(410), [5], ub=wide, upper=range(100))
    V(1, 1023, 509, 0, ops(509), [5], lb=wide)  # (lb adds no row)
    # the message of a call without bounds is what it was
    with pytest.raises(nat.NativeError) as e:
        nat.milpdense_validate(1, 1023, 510, 0, ops(510), [5])
    assert str(e.value).endswith("yalps_milpdense: largest node of 513 x 1024 doubles (511 rows and two cuts for each of 1 integer variables) "
                                 "is above the limit of 4194304 bytes")


def test_milp_batch_checks_bounds_before_the_library(nat, monkeypatch):
    torch = pytest.importorskip("torch")
    from yalps_amd import tensors
    monkeypatch.setattr(nat, "MilpDense", lambda *a, **k: pytest.fail("the library was touched"))
    monkeypatch.setattr(nat, "milpdense_lib", lambda *a, **k: pytest.fail("the library was touched"))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    call = lambda **kw: tensors.milp_batch(z(3), z(2, 3), z(2), integers=[0, 2], binaries=[2], **kw)
    for kw, exc, text in ((dict(ub=z(3), upper=(0, 2)), ValueError, "milp_batch: upper names variable 2, which is binary"),
                          (dict(ub=z(3), upper=(1, 1)), ValueError, "milp_batch: upper names variable 1 twice"),
                          (dict(ub=z(3), upper=(3,)), ValueError, "milp_batch: upper names variable 3, outside 0 .. 2"),
                          (dict(ub=z(3), upper=(-1,)), ValueError, "outside 0 .. 2"),
                          (dict(lb=z(3), upper=()), ValueError, "milp_batch: upper names the variables whose ub entry is read, and no ub was given"),
                          (dict(lb=z(3).float()), TypeError, "milp_batch: lb is torch.float32"),
                          (dict(ub=np.zeros(3)), TypeError, "milp_batch: ub must be a torch.Tensor"),
                          (dict(lb=z(4)), ValueError, "milp_batch: lb has 4 entries, c has 3 variables"),
                          (dict(ub=z(2, 2, 3)), ValueError, "dimensions"),
                          (dict(lb=z(3), ub=z(3), upper=[1, 0]), ValueError, "milp_batch: the operands are read on the GPU where they lie: a CPU tensor was given"),
                          (dict(lb=z(3)), ValueError, "a CPU tensor was given"), (dict(ub=z(3)), ValueError, "a CPU tensor was given")):
        with pytest.raises(exc, match=re.escape(text)):
            call(**kw)
    with pytest.raises(ValueError, match="disagree about B"):
        tensors.milp_batch(z(5, 3), z(2, 3), z(2), ub=z(4, 3))
    # the 4 MiB bound with the bound rows counted, on both sides (under it the call goes on to refuse the CPU tensors)
    wide = lambda m: (z(1023), z(m, 1023), z(m))
    with pytest.raises(ValueError, match="a CPU tensor was given"):
        tensors.milp_batch(*wide(409), integers=[5], ub=z(1023), upper=range(100))
    with pytest.raises(ValueError, match=re.escape("milp_batch: the largest possible node, 513 x 1024 doubles (4202496 bytes: 511 rows and two cuts for "
                                                   "each of 1 integer variables), is above the batch limit of 4194304 bytes; solve() is")):
        tensors.milp_batch(*wide(410), integers=[5], ub=z(1023), upper=range(100))
    with pytest.raises(ValueError, match="a CPU tensor was given"):
        tensors.milp_batch(*wide(509), integers=[5], lb=z(1023))
    # upper=True: 1023 - 1 bound rows and the binary row under row 0
    with pytest.raises(ValueError, match=re.escape("the largest possible node, 1026 x 1024 doubles (8404992 bytes: 1024 rows and two cuts")):
        tensors.milp_batch(z(1023), binaries=[5], ub=z(1023), integers=())
    # the boundless message has not changed (tests/test_milp_dense_model.py pins it too)
    with pytest.raises(ValueError, match=re.escape("milp_batch: the largest possible node, 513 x 1024 doubles (4202496 bytes: 511 rows and two cuts for "
                                                   "each of 1 integer variables), is above the batch limit of 4194304 bytes; solve() is the route for such models")):
        tensors.milp_batch(*wide(510), integers=[5])


def test_signature():
    pytest.importorskip("torch")
    from yalps_amd import tensors
    sig = inspect.signature(tensors.milp_batch).parameters
    names = list(sig)
    assert names[:5] == ["c", "A_ub", "b_ub", "A_eq", "b_eq"] and all(sig[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in names[:5])
    for name, default in (("lb", None), ("ub", None), ("upper", True)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is default
    before = dict(integers=(), binaries=(), maximize=False, precision=1e-8, max_pivots=8192, check_cycles=False, tolerance=0.0,
                  max_iterations=32768, stats=None)
    assert set(names[5:]) == set(before) | {"lb", "ub", "upper"}
    for name, default in before.items():
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    assert [k for k in names[5:] if k in before] == list(before)
    for word in ("ceil(lb[j])", "no bound row", "then the k = len(upper) bound rows", "Out of scope: free"):
        assert word in tensors.milp_batch.__doc__, word
    assert "bounds in milp_batch" not in tensors.linprog_batch.__doc__ + tensors.linprog_objective_bounds.__doc__


# ------------------------------------------------------------------------------------------------- the expectation itself

CPU_CALLS = MDB.names()
FINITE = [n for n in CPU_CALLS if n not in ("NaN at binaries", "inf in ub, NaN in lb")]
SOLVE_LIMIT = 32  # MILPs of a call that also go through solve() (the queue call: its first ones; they come from one generator)


def call_of(name):
    return {"mix": MDB.mix_call, "hist": MDB.hist_call, "views": lambda: MDB.view_call()[0], "shared": lambda: MDB.view_call()[1],
            "identity": MDB.identity_call, "partial": MDB.partial_call}.get(name, lambda: MDB.table_call(name))()


@pytest.fixture(scope="module")
def refs(nat, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = NB.expected(nat, oracle, call_of(name))
        return made[name]
    return get


@pytest.mark.parametrize("name", CPU_CALLS + ["mix", "hist", "views", "shared", "identity", "partial"])
def test_trees_are_small(refs, name):
    """The condition on the tables: every tree ends within NODE_LIMIT consumed nodes and fits the first arena."""
    rows = refs(name)
    assert max(r["nodes"] for r in rows) <= NM.NODE_LIMIT, (name, max(r["nodes"] for r in rows))
    assert rows[0]["reruns"] == 0 and "overflow" not in [r["status"] for r in rows], name


@pytest.mark.parametrize("name", FINITE + ["mix", "hist", "views", "identity"])
def test_oracle_search_moved_back_equals_solve_of_the_equivalent_model(oracle, refs, name):
    call = call_of(name)
    rows = refs(name)
    one = oracle_backend(oracle)
    opt = dict(call.options, includeZeroVariables=True)
    lb, ub = call.bounds_stacked()
    for i, (model, row, low) in enumerate(list(zip(call.models(), rows, call.lows()))[:SOLVE_LIMIT]):
        status, x, objective = model_answer(S._solve_with(one, model, opt), call.n)
        assert status == row["status"], (name, i, status, row["status"])
        assert np.array_equal(NM.words(x), NM.words(row["x_shifted"])), (name, i, x, row["x_shifted"])
        assert np.array_equal(NM.words(objective), NM.words(row["objective_shifted"])), (name, i, objective, row["objective_shifted"])
        if low is not None:  # moved back: one addition each
            with np.errstate(all="ignore"):
                assert np.array_equal(NM.words(row["x"]), NM.words(x + low)), (name, i)
                assert np.array_equal(NM.words(row["objective"]), NM.words(np.float64(objective) + BD.shift_sum(call.lps[i][0], low))), (name, i)
        if row["status"] == "optimal" or (row["status"] == "timedout" and not math.isnan(row["result"])):
            # exactly inside [l_eff, ub]: x' >= 0 is rounded to the precision before l_eff is added, and x' <= ub - l_eff
            x = row["x"]
            if low is not None:
                assert (x >= low).all(), (name, i, x, low)
            else:
                assert (x >= 0.0).all()
            if ub is not None:
                top = np.asarray(ub[i])[list(call.idx)]
                assert (x[list(call.idx)] <= top + (0.0 if call.flaw is None and exact_data(call) else 1e-8)).all(), (name, i, x, top)
            if exact_data(call):
                assert all(float(x[j]).is_integer() for j in call.ints), (name, i, x)
            assert all(x[j] in (0.0, 1.0) for j in call.bins if exact_data(call)), (name, i, x)


def exact_data(call):
    """Data in quarters, whose vertices the search reaches without rounding that shows: the hand-made calls and those of the
    table's generator with a grain."""
    return call.exact


def test_table_reaches_its_endings(refs):
    E = refs
    assert [r["status"] for r in E("lb > ub")] == ["infeasible", "optimal", "infeasible"] and E("lb > ub")[0]["nodes"] == 0
    r = E("unbounded through an unlisted variable")[0]
    assert r["status"] == "unbounded" and r["x"].tolist() == [1.0, -1.0, math.inf] and r["objective"] == math.inf  # (inf + lb)
    with_sol, without = E("timedout with a solution"), E("timedout without a solution")
    assert all(r["status"] == "timedout" for r in with_sol + without)
    assert any(not math.isnan(r["result"]) for r in with_sol) and all(math.isnan(r["result"]) and r["nodes"] == 1 for r in without)
    q = E("queue")
    ends = {(r["status"], r["status"] == "timedout" and not math.isnan(r["result"])) for r in q}
    assert ends == {("optimal", False), ("infeasible", False), ("unbounded", False), ("cycled", False), ("timedout", False), ("timedout", True)}, ends
    for name in ["bound rows and binary rows", "no operand rows", "equalities only"] + ["n=%d" % n for n in MDB.LANES] + \
            [s + c for s in MDB.SHAPES for c in ("", " check")]:
        assert any(r["nodes"] > 0 for r in E(name)), name
    # rule 1 shows: the answers with lb rounded up differ from those of the continuous relaxation's lb
    frac = E("fractional lb at integers")
    assert frac[0]["x"].tolist()[:3] == [2.0, 1.0, 0.0] and [r["status"] for r in frac] == ["optimal"] * 3
    lies = E("inf in ub, NaN in lb")
    assert [r["status"] for r in lies] == ["optimal", "unbounded", "unbounded"]
    # the history rerun: roots, and in every tree a node, of more pivots than a history of HIST holds
    hist = E("hist")
    assert all(r["root_pivots"] > MDB.HIST and max(t[4] for t in r["trace"]) > MDB.HIST for r in hist)


def test_rule_2_on_the_expectation(nat, oracle, refs):
    clean = NB.expected(nat, oracle, MDB.rule_calls()[1])
    for a, b in zip(refs("NaN at binaries"), clean):
        assert a["status"] == b["status"] == "optimal" and np.array_equal(words(a["x"]), words(b["x"])) and a["objective"] == b["objective"]
        assert a["trace"] == b["trace"]


def test_mix_reruns_and_overflows(nat, oracle):
    mix = MDB.mix_call()
    rows = NB.expected(nat, oracle, mix)
    assert [r["nodes"] for r in rows[6:]] == [0, 0] and [r["status"] for r in rows[6:]] == ["optimal", "infeasible"]
    assert all(r["nodes"] > 2 for r in rows[:6])
    again = NB.expected(nat, oracle, mix, arena=2)
    assert again[0]["reruns"] >= 6  # (the six trees, some of them twice; the two roots without a tree never)
    over = [r["status"] for r in NB.expected(nat, oracle, mix, arena=2, arena_max=2)]
    assert 0 < over.count("overflow") < len(mix.lps)


def test_identity_route_is_the_same_milp(nat, oracle, refs):
    call = MDB.identity_call()
    rows = NM.expected(nat, oracle, NM.Call("identity rows", MDB.identity_operands(call), integers=True, maximize=True))
    for a, b in zip(refs("identity"), rows):
        assert a["status"] == b["status"] == "optimal" and a["objective"] == b["objective"] and float(a["objective"]).is_integer()
    assert any(r["nodes"] > 0 for r in rows)


# ------------------------------------------------------------------------------------------------- rounding that shows

# rows of a call (of 8) whose expected answer changes under a flaw, in BD.FLAWS' order: what the oracle alone gives, held as a floor
FLOORS = {"hard n=65": dict(zip(BD.FLAWS, (5, 2, 2, 2, 8, 8, 8))), "hard n=129": dict(zip(BD.FLAWS, (4, 2, 1, 1, 8, 8, 8)))}


def answer_words(row):
    return np.concatenate([NM.words(row["x"]), NM.words(row["objective"]), NM.words(row["col0"]), NM.words(row["result"]),
                           np.array([NM.STATUS.index(row["status"]), row["nodes"], row["node_pivots"], row["root_pivots"]], np.int64)])


@pytest.mark.parametrize("name", MDB.HARD)
def test_hard_calls_tell_every_flaw(nat, oracle, refs, name):
    """Non-integer lb at continuous variables, data whose rounding shows: under each of BD.SUM_FLAWS and BD.READ_FLAWS the expected
    answer of at least FLOORS rows changes -- status, counts, result, column 0 of the best tableau, x or the objective, all of
    which the GPU test compares bit for bit.  Without this the GPU comparison could pass with another order of summation."""
    call, rows = call_of(name), refs(name)
    kinds = [j for j in range(call.n) if j not in call.ints]
    assert any(not float(lb[j]).is_integer() for lb in call.lbs for j in kinds)
    assert sum(r["status"] in ("optimal", "timedout") and not math.isnan(r["result"]) for r in rows) >= 2, [r["status"] for r in rows]
    for flaw in BD.FLAWS:
        bad = NB.expected(nat, oracle, call.flawed(flaw))
        changed = sum(not np.array_equal(answer_words(a), answer_words(b)) for a, b in zip(rows, bad))
        print("%s, %s: %d of %d rows change" % (name, flaw, changed, len(rows)))
        assert changed >= FLOORS[name][flaw], (name, flaw, changed)
        if flaw in BD.READ_FLAWS:  # (the read-out leaves the search alone)
            assert all(a["trace"] == b["trace"] and np.array_equal(NM.words(a["col0"]), NM.words(b["col0"])) for a, b in zip(rows, bad))


# ------------------------------------------------------------------------------------------------------ header and build

def test_header_declares_the_new_entries(nat):
    text = open(os.path.join(ROOT, "include", "yalps_milpdense.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(yalps_[a-z0-9_]+)\s*\(", code))
    assert declared == set(nat.SYMBOLS_MILPDENSE), declared ^ set(nat.SYMBOLS_MILPDENSE)
    assert {"yalps_milpdense_validate_bounds", "yalps_milpdense_solve_bounds"} <= declared
    lib = nat.milpdense_lib()
    assert all(hasattr(lib, s) for s in declared)
    for word in ("ceil(lb[j])", "has no bound row", "then the n_upper bound rows in ascending index, then the binary rows", "libyalps_milpdense_bounds.so"):
        assert word in text, word


def test_build_lists_the_bounds_library():
    from yalps_amd import build
    assert os.path.basename(build.LIB_MILPDENSE_BOUNDS) == "libyalps_milpdense_bounds.so" and callable(build.build_milpdense_bounds)
    assert "libyalps_milpdense_bounds.so" in build.__doc__ and "libyalps_lpdense_bounds.so" in build.__doc__
    names = [os.path.basename(p) for p in build.HIP_DEPS]
    assert "milp_dense_bounds_kernel.cuh" not in names
    assert "milp_dense_bounds_kernel.cuh" in [os.path.basename(p) for p in build.MILPDENSE_BOUNDS_DEPS]
    assert "milp_dense_bounds_kernel.cuh" in [os.path.basename(p) for p in build.MILPDENSE_DEPS]  # (milp_dense.hip includes its structs)
    assert {"milp_dense_bounds_root_kernel", "milp_dense_bounds_solution_kernel"} <= set(build.NO_SCRATCH)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "libyalps_milpdense_bounds.so" in entry


def test_bounds_kernels_pass_the_register_budget(nat):
    """The six bounded root forms and the bounded epilogue are a code object of their own, under the build gate of their boundless
    siblings: no scratch, no accumulator registers, within 128 VGPRs, static LDS a multiple of 16."""
    from yalps_amd import build
    ks = build.check_register_budgets(build.LIB_MILPDENSE_BOUNDS, min_resident=0)
    roots = {k: v for k, v in ks.items() if "milp_dense_bounds_root_kernel" in k}
    epilogue = {k: v for k, v in ks.items() if "milp_dense_bounds_solution_kernel" in k}
    assert len(roots) == 6 and len(epilogue) == 1 and len(ks) == 7, sorted(ks)
    for k, md in ks.items():
        assert int(md["private_segment_fixed_size"]) == 0 and int(md["agpr_count"]) == 0 and int(md["vgpr_count"]) <= 128, (k, md)
    for k, md in roots.items():
        assert int(md["group_segment_fixed_size"]) % 16 == 0, (k, md)
    # the boundless library holds exactly the kernels it held
    mine = build.kernel_metadata(build.LIB_MILPDENSE)
    count = lambda tag: sum(tag in k for k in mine)
    assert (count("milp_dense_root_kernel"), count("milp_tree_kernel"), count("milp_dense_solution_kernel"), len(mine)) == (6, 6, 1, 13), sorted(mine)
    assert not any("bounds" in k for k in mine)
    # and it links the new one
    import subprocess
    needed = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", build.LIB_MILPDENSE], capture_output=True, text=True, check=True).stdout
    assert "libyalps_milpdense_bounds.so" in needed and "$ORIGIN" in needed
