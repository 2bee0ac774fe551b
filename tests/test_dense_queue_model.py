"""The calls of tests/test_dense_queue.py, with the oracle alone (no GPU): that every call is admitted and selects the kernel form
it is meant for, that its seven items end as tests/_dense_queue.py says, and that the DATA can tell a workgroup that leaves
something of item k behind when it takes item k + 1 (Q.STALE) from a right one.  Also the refusals of the four grid hooks, which
both libraries check in front of the device."""
from collections import Counter

import numpy as np
import pytest

from tests import _dense_queue as Q
from tests import _lp_batch as LB
from tests import _lp_dense_free as LF


@pytest.fixture(scope="module")
def calls(oracle):
    return Q.lp_calls(oracle)


@pytest.fixture(scope="module")
def refs(oracle, calls):
    return {c.name: [c.oracle_answer(oracle, i) for i in range(Q.ITEMS)] for c in calls}


def test_every_call_passes_the_validator(calls):
    from yalps_amd import _native as nat
    for call in calls:
        fake = lambda rows, cols: (8, rows * cols, cols, 1)  # (a pointer that is not NULL: nothing is dereferenced)
        ops = (fake(call.n, 1), fake(call.m_ub, call.n), fake(call.m_ub, 1), fake(call.m_eq, call.n), fake(call.m_eq, 1))
        bound = None if call.family == "plain" else fake(call.n, 1)
        nat.lpdense_validate_free(Q.ITEMS, call.n, call.m_ub, call.m_eq, ops, lb=bound, ub=bound, upper=call.idx, free=call.fidx)
        assert len(call.lps) == Q.ITEMS and call.m_eq >= 1, call.name


def test_what_the_calls_cover(calls):
    """One call per (family, form): the 30 LP forms above class 0 by (kernel, class, aux), 18 spellings."""
    forms = Counter((c.kernel, LB.size_class(c.w, c.h), int(Q.BS.aux_hbm(c.w, c.h)) if LB.size_class(c.w, c.h) == 4 else 0) for c in calls)
    for call in calls:
        assert (LB.size_class(call.w, call.h), call.kernel) == LF.kernel_of(call), call.name
        assert (call.cls, call.aux) == Q.forms()[call.form][2:] and call.cls >= 1
    spellings = {c.kernel for c in calls}
    print("dense queue calls: %d, (kernel, class, aux) forms: %d, kernel spellings: %d" % (len(calls), len(forms), len(spellings)))
    assert len(calls) == len(forms) == 30 and set(forms.values()) == {1}
    assert spellings == Q.lp_spellings() and len(spellings) == 18
    assert Counter(cls for _, cls, _ in forms) == {1: 6, 2: 6, 3: 6, 4: 12} and Counter(aux for _, _, aux in forms) == {0: 24, 1: 6}
    for family in Q.FAMILIES:
        assert {"%s<256,check,lds>" % Q.LP_KERNEL[family], "%s<1024,check>" % Q.LP_KERNEL[family]} <= spellings
    by_family = {f: next(c for c in calls if c.family == f) for f in Q.FAMILIES}
    assert not by_family["plain"].has_lb and not by_family["plain"].k and not by_family["plain"].f
    b, f = by_family["bounded"], by_family["free"]
    assert b.has_lb and b.has_ub and 0 < b.k < b.n and not b.f           # `upper` a strict subset
    assert f.f >= 2 and len(set(f.fidx) & set(f.idx)) == 1 and f.has_lb  # two free variables, one of them with an upper bound


@pytest.mark.parametrize("name", Q.lp_names())
def test_the_items_end_as_meant(calls, refs, oracle, name):
    call = next(c for c in calls if c.name == name)
    R = refs[name]
    statuses = [r["status"] for r in R]
    print(name, "budget", call.max_pivots, [(r["status"], r["n_pivots"]) for r in R])
    assert [statuses[i] for i in Q.OPTIMAL] == ["optimal"] * 3 and statuses[Q.INFEASIBLE] == "infeasible", statuses
    assert statuses[Q.UNBOUNDED] == "unbounded" and statuses[Q.CYCLED] == "cycled", statuses
    assert {"optimal", "infeasible", "unbounded", "cycled"} <= set(statuses)
    # the budget: 3 pivots less than item CYCLED needs (alone, unlimited), reached by it in the call
    import copy
    alone = copy.copy(call)
    alone.max_pivots, alone._refs = 3000.0, {}
    full = alone.oracle_answer(oracle, Q.CYCLED)
    assert full["status"] == "optimal" and full["n_pivots"] == call.max_pivots + Q.BUDGET_SHORT and R[Q.CYCLED]["n_pivots"] == call.max_pivots
    assert all(r["n_pivots"] >= 1 for r in R), "an item without a pivot leaves the identity behind: the next one could not tell"
    # the non-finite item: a NaN right-hand side; with bounds a shift sum of +inf and one of -inf (rows 2 and 3)
    start = R[Q.NONFINITE]["start"].reshape(call.h, call.w)
    assert np.isnan(start[2, 0])
    if call.family != "plain":
        from tests import _np_dense_bounds as BD
        lp, low = call.lps[Q.NONFINITE], call.low(Q.NONFINITE)
        assert [BD.shift_sum(lp[1][r], low) for r in (2, 3)] == [np.inf, -np.inf] and np.isnan(start[3, 0]) and start[4, 0] == np.inf
    if call.family == "free":  # unbounded through a twin
        r = R[Q.UNBOUNDED]
        assert call.n < int(r["var"][int(r["result"])]) < call.w and (r["x"] == -np.inf).sum() == 1
    for k in range(Q.ITEMS - 1):
        assert LF.differing(R[k]["x"], R[k + 1]["x"]) > 0, (name, k, "adjacent items with the same x")


@pytest.mark.parametrize("name", [n for n in Q.lp_names() if not n.endswith("check")])
def test_the_data_tells_stale_state(calls, refs, oracle, name):
    """For every adjacent pair and every flaw of Q.STALE the oracle's answer for item k + 1 changes in a compared word.  (The fill
    does not depend on checkCycles: a call and its `check` twin hold the same data, and the twin's answers are asserted equal.)"""
    call = next(c for c in calls if c.name == name)
    R = refs[name]
    for k in range(Q.ITEMS - 1):
        for flaw in Q.STALE:
            start, pos, var = Q.stale_start(call, R[k], R[k + 1], flaw)
            assert Q.words_differ(Q.answer_from(oracle, call, k + 1, start, pos, var), R[k + 1]) > 0, (name, k, flaw)
    twin = refs[name + " check"]
    assert all(Q.words_differ(a, b) == 0 for a, b in zip(R, twin)), "checkCycles changes an answer: the twin needs its own look"


def test_answer_from_the_canonical_start_is_the_canonical_answer(calls, refs, oracle):
    call = calls[0]
    identity = np.arange(call.w + call.h, dtype=np.int32)
    for i, ref in enumerate(refs[call.name]):
        assert Q.words_differ(Q.answer_from(oracle, call, i, ref["start"], identity, identity), ref) == 0, i


@pytest.mark.parametrize("var,value,word", [("YALPS_LPDENSE_PER_CU", "9", "outside 0..8"), ("YALPS_LPDENSE_PER_CU", "-1", "outside 0..8"),
                                            ("YALPS_LPDENSE_CUS", "-2", "negative"), ("YALPS_MILPDENSE_PER_CU", "9", "outside 0..8"),
                                            ("YALPS_MILPDENSE_PER_CU", "-1", "outside 0..8"), ("YALPS_MILPDENSE_CUS", "-2", "negative")])
def test_a_bad_grid_hook_is_refused_at_create(monkeypatch, var, value, word):
    """Both libraries read their two grid hooks in front of the device: the refusal needs no GPU."""
    from yalps_amd import _native as nat
    monkeypatch.setenv(var, value)
    with pytest.raises(nat.NativeError) as e:
        (nat.LpDense if var.startswith("YALPS_LPDENSE") else nat.MilpDense)(0)
    assert var in str(e.value) and word in str(e.value) and " error -1: " in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------- the MILP calls

@pytest.fixture(scope="module")
def milp_calls():
    return Q.milp_calls()


def test_what_the_milp_calls_cover(milp_calls):
    """One call per (family, form): all 18 root spellings and all 6 tree spellings, the classes 1 .. 3, HBM and aux."""
    roots, trees = Q.milp_spellings()
    print("dense queue MILP calls: %d, root spellings: %d, tree spellings: %d" % (len(milp_calls), len(roots), len(trees)))
    assert len(milp_calls) == 30 and len(roots) == 18 and len(trees) == 6
    assert {c.root_kernel for c in milp_calls} == roots and {c.tree_kernel for c in milp_calls} == trees
    assert Counter((c.family, c.cls, c.aux, c.check) for c in milp_calls) == Counter(
        (f, cls, aux, check) for f in Q.FAMILIES for _, _, cls, aux in Q.forms().values() for check in (False, True))
    for c in milp_calls:
        assert LB.size_class(c.w, c.h) == c.cls >= 1 and LB.size_class(c.w, c.hmax) == c.tree_cls and len(c.lps) == Q.ITEMS, c.name
        assert bool(Q.BS.aux_hbm(c.w, c.h)) == bool(c.aux) and bool(Q.BS.aux_hbm(c.w, c.hmax)) == bool(c.aux), c.name
        assert 6.0 <= c.max_iterations <= 12.0
    free = next(c for c in milp_calls if c.family == "free")
    assert free.f == 2 and free.int_twins == 1 and len(set(free.fidx) & set(free.idx)) == 1
    bounded = next(c for c in milp_calls if c.family == "bounded")
    assert bounded.has_lb and bounded.has_ub and 0 < bounded.k < bounded.n


@pytest.mark.parametrize("name", Q.milp_names())
def test_the_milp_items_end_as_meant(milp_calls, oracle, name):
    """By the oracle-driven search: four roots that branch, an integral root, an infeasible root, a root cycled by the budget."""
    from yalps_amd import _native as nat
    call = next(c for c in milp_calls if c.name == name)
    rows = Q.milp_rows(nat, oracle, call)
    print(name, "budget", call.max_pivots, [(r["status"], r["root_pivots"], r["nodes"]) for r in rows])
    for i in Q.BRANCH:
        assert rows[i]["nodes"] > 0 and 0 < rows[i]["root_pivots"] <= call.max_pivots, (name, i)
    assert rows[Q.INTEGRAL]["status"] == "optimal" and rows[Q.INTEGRAL]["nodes"] == 0 and rows[Q.INTEGRAL]["root_pivots"] > 0
    assert rows[Q.M_INFEASIBLE]["status"] == "infeasible" and rows[Q.M_INFEASIBLE]["nodes"] == 0
    assert rows[Q.M_CYCLED]["status"] == "cycled" and rows[Q.M_CYCLED]["root_pivots"] == call.max_pivots and rows[Q.M_CYCLED]["nodes"] == 0
    for k in range(Q.ITEMS - 1):
        assert LF.differing(rows[k]["x"], rows[k + 1]["x"]) > 0, (name, k, "adjacent items with the same x")
