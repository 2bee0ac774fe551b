"""What defines sensitivity_many's numbers and lp_sens_kernel's five arrays, independently of the product:

A. the exact reference (tests/_exact_sensitivity.py): duals, reduced costs and every range end from the textbook definitions
   in rational arithmetic, at the basis the solve ended on, from the model's own terms.  The mapping of
   yalps_amd/sensitivity.py is compared with it on the golden LP cases, the two models of tests/test_lp_sensitivity.py, four
   dense models and hand models for what those lack -- on the CPU through the C oracle, on the GPU through sensitivity_many.
B. the loop reference (tests/_sens_table.py): the ranging epilogue on LPs that end optimal after 0 pivots, so that the test
   writes its input entry by entry -- every kernel form, pass, group size and tail, planted winners in every lane position,
   the IEEE rules -- against a plain double loop over Python floats.

Comparisons.  A: |got - exact| <= 1e-9 * max(1, |got|, |exact|), infinite ends equal as infinities, keys and their order
exactly.  B: row0 bit for bit, the ratio arrays bit for bit wherever the reference is not a zero, zeros equal as numbers."""
import math

import numpy as np
import pytest

from tests import _exact_sensitivity as X
from tests import _lp_batch as LB
from tests import _lp_variants as LV
from tests import _np_sensitivity as NS
from tests import _sens_table as ST
from tests.test_lp_sensitivity import KERNELS, MINIMISE, TEXTBOOK, lp_cases

INF = math.inf
TOL = 1e-9  # 50 x the worst disagreement measured (1.8e-11, below), 100 x tighter than the finite-difference property
SMALL = 1e-6

# ---------------------------------------------------------------------------------------------- A: hand models
# Each says what it is for; test_hand_models_show_what_they_are_for asserts that the oracle's solve shows it.

DUPLICATES = {  # an iterable model: constraint "a" is given three times (merged to [2, 6]), variable key "x" twice (two columns),
    "direction": "maximize", "objective": "p",  # and y's coefficient of "p" twice (the later one counts)
    "constraints": [("a", {"max": 10}), ("b", {"max": 8}), ("a", {"min": 2}), ("a", {"max": 6})],
    "variables": [("x", {"p": 3, "a": 1, "b": 1}), ("y", [("p", 1), ("a", 1), ("b", 2), ("p", 2)]), ("x", {"p": 2.5, "a": 2, "b": 0.5})],
}
TWO_SIDED = {  # maximize: "c1" is two-sided and binds at its upper side, "c2" is two-sided and binds at its lower side
    "direction": "maximize", "objective": "p",
    "constraints": {"c1": {"min": 2, "max": 6}, "c2": {"min": 3, "max": 9}, "c3": {"max": 1}},
    "variables": {"x": {"p": 3, "c1": 1}, "y": {"p": 2.5, "c1": 1, "c2": 1, "c3": 1}, "z": {"p": -1, "c2": 1}},
}
EQUAL_MAX = {  # `equal` constraints: "e1" has a positive dual, "e2" a negative one -- here under "maximize" ...
    "direction": "maximize", "objective": "p",
    "constraints": {"e1": {"equal": 4}, "e2": {"equal": 2}, "lim": {"max": 3}},
    "variables": {"x": {"p": 2, "e1": 1, "lim": 1}, "y": {"p": 1, "e1": 1}, "z": {"p": -3, "e2": 1}},
}
EQUAL_MIN = dict(EQUAL_MAX, direction="minimize")  # ... and under "minimize"
ABSENT = {  # variable "u" has no coefficient of the objective, and is basic
    "direction": "maximize", "objective": "p",
    "constraints": {"a": {"max": 4}, "b": {"min": 1}},
    "variables": {"x": {"p": 2, "a": 1}, "u": {"a": 1, "b": 1}},
}
NO_OBJECTIVE = {  # no "objective" key: every cost is 0
    "constraints": {"a": {"min": 2}, "b": {"max": 5}},
    "variables": {"x": {"a": 1, "b": 1}, "y": {"a": 1}},
}
DEGENERATE = {  # three constraints meet in the optimum (2, 2): a basic variable is 0
    "direction": "maximize", "objective": "p",
    "constraints": {"c1": {"max": 2}, "c2": {"max": 2}, "c3": {"max": 4}},
    "variables": {"x": {"p": 1, "c1": 1, "c3": 1}, "y": {"p": 1, "c2": 1, "c3": 1}},
}
DUAL_DEGENERATE = {  # the objective is parallel to "c1": a whole edge is optimal, a non-basic reduced cost is 0
    "direction": "maximize", "objective": "p",
    "constraints": {"c1": {"max": 4}, "c2": {"max": 3}},
    "variables": {"x": {"p": 1, "c1": 1, "c2": 1}, "y": {"p": 1, "c1": 1}},
}
FALLING = {  # an upper side that may fall without limit (x only grows): the one infinite end no other model has
    "direction": "maximize", "objective": "p",
    "constraints": {"d": {"max": -2}},
    "variables": {"x": {"p": -1, "d": -1}},
}
HAND = [("falling upper side", FALLING), ("duplicates", DUPLICATES), ("two-sided", TWO_SIDED), ("equal, maximize", EQUAL_MAX), ("equal, minimize", EQUAL_MIN),
        ("absent from the objective", ABSENT), ("no objective", NO_OBJECTIVE), ("degenerate", DEGENERATE),
        ("dual degenerate", DUAL_DEGENERATE)]
DENSE = ((12, 10), (30, 30), (30, 29), (60, 50))
# golden cases whose B^-1 or B^-1 N has a nonzero entry below SMALL (test_small_entries_have_no_say)
GOLDEN_WITH_SMALL_ENTRIES = {"Steepest Edge Column Selection", "Stigler Diet"}

_exact = {}


def all_models(oracle):
    """[(name, kind, model, options)] of every model of tier A."""
    out = [(name, "golden", model, options) for name, model, options in lp_cases()]
    out += [("TEXTBOOK", "hand", TEXTBOOK, None), ("MINIMISE", "hand", MINIMISE, None)]
    out += [("dense %d x %d" % (M, N), "dense", LV.dense_model(oracle, M, N, 3), None) for M, N in DENSE]
    out += [(name, "hand", model, None) for name, model in HAND]
    return out


@pytest.fixture(scope="module")
def exact(oracle):
    """[(name, kind, model, options, Exact)], computed once for the module (a few seconds) and never changed."""
    if "all" not in _exact:
        _exact["all"] = [(name, kind, model, options, X.Exact(oracle, model, options)) for name, kind, model, options in all_models(oracle)]
    return _exact["all"]


def optimal(exact):
    return [row for row in exact if row[4].status == "optimal"]


def test_the_exact_reference_checks_itself(exact):
    """Without a solver: both ends and the midpoint of every finite range are primal and dual feasible for the basis, a
    point (1 + |end|) / 1024 beyond a finite end is not, an infinite end stays feasible 1, 2^10 and 2^20 away."""
    assert len(exact) == 43 + 2 + len(DENSE) + len(HAND)
    assert sum(1 for row in exact if row[1] == "golden" and row[4].status == "optimal") == 34
    assert all(row[4].status == "optimal" for row in exact if row[1] != "golden")
    points = sum(e.self_check() for *_, e in optimal(exact))
    print("points", points)
    assert points > 4500, points
    # the ends the goldens lack are there: finite and infinite ends of upper_range, lower_range and objective_range, both ends
    ends = set()
    for *_, e in optimal(exact):
        for part in ("constraints", "variables"):
            for _, entry in e.sensitivity[part]:
                for field, value in entry.items():
                    if field.endswith("_range"):
                        ends |= {(field, 0, value[0] == -INF), (field, 1, value[1] == INF)}
    assert ends == {(f, side, infinite) for f in ("upper_range", "lower_range", "objective_range") for side in (0, 1)
                    for infinite in (False, True)}


def test_small_entries_have_no_say(exact):
    """The kernel ignores entries with |M[r,c]| <= precision, the exact reference does not: the models must not depend on the
    difference.  No nonzero entry of B^-1 or B^-1 N of a hand model or a dense model is below 1e-6 in magnitude.  Of the 34
    optimal golden cases two have one -- "Steepest Edge Column Selection" 4.0e-18 (the residue of 0.1-like coefficients that
    cancel in the reals, not in doubles) and "Stigler Diet" 9.3e-7 -- and for every model, those two included, the exact
    answer is the same, Fraction for Fraction, with every entry below 1e-6 taken as 0: no such entry decides a range end."""
    small = set()
    for name, kind, _, _, e in optimal(exact):
        least = e.smallest_entry()
        print(name, float(least))
        if least < X.Fraction(SMALL):
            small.add(name)
            assert kind == "golden", (name, float(least))  # (a hand model with a small pivot is the wrong hand model)
        assert e.sensitivity_ignoring(SMALL) == e.sensitivity, name
    assert small == GOLDEN_WITH_SMALL_ENTRIES, small


def test_hand_models_show_what_they_are_for(exact):
    by_name = {name: e for name, _, _, _, e in exact}
    sens = lambda name: (dict(by_name[name].sensitivity["constraints"]), by_name[name].sensitivity["variables"])
    nonbasic_side = lambda e, key, kind: any(e.n + i not in e.position for i, s in enumerate(e.sides) if s[:2] == (key, kind))
    cons, vars_ = sens("duplicates")
    assert list(cons) == ["a", "b"] and [k for k, _ in vars_] == ["x", "y", "x"]
    assert set(cons["a"]) == {"dual", "upper_range", "lower_range"} and by_name["duplicates"].columns[1][2] == 2  # (y's p is the later 2)
    assert [s[:3] for s in by_name["duplicates"].sides] == [("a", "upper", 6), ("a", "lower", 2), ("b", "upper", 8)]
    e = by_name["two-sided"]
    cons, _ = sens("two-sided")
    assert nonbasic_side(e, "c1", "upper") and not nonbasic_side(e, "c1", "lower") and cons["c1"]["dual"] > 0
    assert nonbasic_side(e, "c2", "lower") and not nonbasic_side(e, "c2", "upper") and cons["c2"]["dual"] < 0
    for name in ("equal, maximize", "equal, minimize"):
        cons, _ = sens(name)
        assert cons["e1"]["dual"] > 0 > cons["e2"]["dual"], name
        assert all(set(cons[k]) == {"dual", "upper_range", "lower_range"} for k in ("e1", "e2"))
    e = by_name["absent from the objective"]
    assert "p" not in ABSENT["variables"]["u"] and e.columns[1][0] == "u" and 1 in e.position and e.xB[e.position[1]] > 0
    e = by_name["no objective"]
    assert "objective" not in NO_OBJECTIVE and all(c[2] == 0 for c in e.columns) and all(d == 0 for d in e.d.values())
    e = by_name["degenerate"]
    assert any(x == 0 for x in e.xB) and all(d > 0 for d in e.d.values())
    e = by_name["dual degenerate"]
    assert any(d == 0 for d in e.d.values()) and all(x > 0 for x in e.xB)
    assert sens("falling upper side")[0]["d"]["upper_range"] == (-INF, 0) and sens("falling upper side")[0]["d"]["dual"] == 1
    # what the goldens lack and these bring: a binding lower side of a two-sided constraint under "maximize"
    assert sens("two-sided")[0]["c2"]["lower_range"] == (1, 9)


def worst_of(results, exact_rows):
    """(worst finite disagreement, [(model, key, field, disagreement)] above TOL) of solved models against their exact rows."""
    worst, bad = (0.0, None), []
    for (name, _, _, _, e), r in zip(exact_rows, results):
        assert r["status"] == e.status, (name, r["status"], e.status)
        if e.status != "optimal":
            assert r["sensitivity"] is None, name
            continue
        for dis, key, field in X.compare(r["sensitivity"], e.sensitivity):
            if dis > TOL:
                bad.append((name, key, field, dis))
            elif dis > worst[0]:
                worst = (dis, (name, key, field))
    return worst, bad


def test_the_mapping_against_the_exact_reference(oracle, exact):
    """Every dual, reduced cost and range end the product's mapping gives, driven by the C oracle and the numpy restatement,
    against the exact reference.  Worst disagreement measured: 1.75e-11, a reduced cost of "Large Farm MIP" (the oracle's own
    rounding over its pivots); every other figure agrees to 1.5e-14 or better; no infinite end disagrees.  TOL is 1e-9."""
    results = NS.oracle_sensitivity(oracle, [row[2] for row in exact], [row[3] for row in exact])
    worst, bad = worst_of(results, exact)
    print("worst disagreement", worst)
    assert not bad, bad[:10]


def wrong_mapping(factor, lower_only):
    """sensitivity_of behind a wrong reading of the ratio arrays: all of them times `factor`, or (lower_only) only the
    entries that belong to the rows that stand for lower sides."""
    from yalps_amd import sensitivity as SE
    real = SE.sensitivity_of

    def wrapped(tabmod, bounds_info, ranges):
        row0, *ratios = (np.array(a, np.float64) for a in ranges)
        if not lower_only:
            ratios = [a * factor for a in ratios]
        else:
            t = tabmod.tableau
            for b in bounds_info["bounds"].values():
                if math.isfinite(b["lower"]):
                    r = b["row"] + (1 if math.isfinite(b["upper"]) else 0)
                    p = int(t.position_of_variable[t.width + r])
                    for a in (ratios[:2] if p < t.width else ratios[2:]):
                        a[p if p < t.width else p - t.width] *= factor
        return real(tabmod, bounds_info, (row0, *ratios))
    return wrapped


@pytest.mark.parametrize("factor,lower_only", [(1.5, False), (0.5, False), (1.5, True), (0.5, True)])
def test_wrong_mappings_are_rejected(oracle, exact, monkeypatch, factor, lower_only):
    """Ranges 1.5 x too wide pass the finite-difference property (it steps halfway), ranges 0.5 x as wide pass it by
    construction, and nothing else looks at a lower_range end: the exact reference rejects all four."""
    from yalps_amd import sensitivity as SE
    monkeypatch.setattr(SE, "sensitivity_of", wrong_mapping(factor, lower_only))
    results = NS.oracle_sensitivity(oracle, [row[2] for row in exact], [row[3] for row in exact])
    _, bad = worst_of(results, exact)
    models = {name for name, _, _, _ in bad}
    print(factor, lower_only, len(bad), sorted(models))
    assert bad
    if lower_only:
        assert {field.split()[0] for _, _, field, _ in bad} == {"lower_range"}
        assert {"MINIMISE", "two-sided", "equal, maximize"} <= models
    else:
        assert {field.split()[0] for _, _, field, _ in bad} == {"upper_range", "lower_range", "objective_range"}
        assert len(models) >= 30  # (nearly every optimal model has a finite, nonzero range end)


# ---------------------------------------------------------------------------------------------- B: the epilogue's table

# (form, pass, G): the tail kinds the table reaches.  A 1024-lane form needs a tableau above 79 KiB (LDS) or 150 KiB (HBM);
# with fewer than NG = 1024 / G lines of at most G entries a tableau has fewer than 1024 + NG entries, so "fewer" exists
# there only for G = 64, whose lines may be longer than 64.
ALL3 = ("multiple", "plus one", "fewer")
REACHED = {(form, which, g): ALL3 if form == "256,lds" or g == 64 else ALL3[:2]
           for form in ST.FORMS for which in (1, 2) for g in ST.GROUPS}

_table = {}


@pytest.fixture(scope="module")
def table(oracle):
    """(rows, references, winners): the table and the loop reference of every row, computed once and never changed."""
    if "rows" not in _table:
        rows = ST.table(oracle)
        refs = [ST.loop_reference(lp) for _, lp in rows]
        _table["rows"], _table["refs"], _table["wins"] = rows, [r for r, _ in refs], [w for _, w in refs]
    return _table["rows"], _table["refs"], _table["wins"]


def test_the_table_reaches_every_form_pass_group_size_and_tail(table):
    rows, refs, wins = table
    print(len(rows), "LPs,", sum(lp[0] * lp[1] for _, lp in rows), "entries")
    got = {}
    for form, which, g, tail in ST.reached(rows):
        if tail != "other":
            got.setdefault((form, which, g), set()).add(tail)
    assert {k: tuple(t for t in ALL3 if t in v) for k, v in got.items()} == REACHED
    # line lengths on both sides of every power of two, per form and pass
    lengths = {}
    for _, lp in rows:
        for which, g, length, _ in ST.passes(lp[0], lp[1]):
            lengths.setdefault((ST.form_of(lp[0], lp[1]), which), set()).add(length)
    every = {n for ls in ST.LENGTHS.values() for n in ls}
    assert all(every <= lengths[(form, which)] for form in ST.FORMS for which in (1, 2))
    names = [name for name, _ in rows]
    shapes = {(lp[0], lp[1]) for _, lp in rows}
    assert {(8200, 2), (2, 8200), (1, 5), (6, 1), (1, 1), (2, 7), (7, 2)} <= shapes and len(set(names)) == len(names)
    # planted winners: every lane position of every G has carried the winner of each of the four arrays
    carried = {}
    for (_, lp), win in zip(rows, wins):
        for which, g, _, _ in ST.passes(lp[0], lp[1]):
            for name in (("col_up", "col_dn") if which == 1 else ("row_lo", "row_hi")):
                carried.setdefault((name, g), set()).update(at % g for at in win[name][1:] if at is not None)
    for name in ST.NAMES[1:]:
        for g in ST.GROUPS:
            assert carried[(name, g)] == set(range(g)), (name, g, sorted(set(range(g)) - carried[(name, g)]))


def test_the_ieee_rules_by_hand(table):
    """The loop reference itself, on the IEEE block, against values worked out by hand -- alone and embedded."""
    rows, refs, _ = table
    n = ST.IEEE_ROWS
    seen = 0
    for (name, lp), ref in zip(rows, refs):
        if not name.startswith("IEEE"):
            continue
        seen += 1
        w, h = lp[0], lp[1]
        for k, array in enumerate(ST.NAMES[1:], start=1):
            shift = (w if k <= 2 else h) - 1 - n
            for index, value in ST.IEEE_BY_HAND[array].items():
                assert ref[k][shift + index] == value, (name, array, index, ref[k][shift + index], value)
        assert 0 < ref[1][w - 1 - n + 15] < 2.3e-308 and 0 < ref[4][h - 1 - n + 16] < 2.3e-308  # (subnormal)
        if w > n + 1:  # embedded: the lines outside the block have no entry beyond the precision
            assert np.isinf(ref[1][1:w - n]).all() and np.isinf(ref[2][1:w - n]).all()
            assert (ref[3][1:h - n] == -INF).all() and (ref[4][1:h - n] == INF).all()
    assert seen == 3
    m = LB.scatter(rows[0][1])
    assert np.isnan(m).sum() == 1 and np.isinf(m).sum() == 7 and (m == ST.P).sum() == 2 and (m == -ST.P).sum() == 3


def test_restatement_and_host_ranging_against_the_loop_reference(table):
    """tests/_np_sensitivity.restate (the reference of the existing GPU tests) and sensitivity.ranges_from_tableau (the host
    ranging of the LPs above 4 MiB) on every matrix of the table."""
    from yalps_amd.sensitivity import ranges_from_tableau
    rows, refs, _ = table
    for (name, lp), ref in zip(rows, refs):
        m = LB.scatter(lp)
        for what, f in (("restate", NS.restate), ("ranges_from_tableau", ranges_from_tableau)):
            diff = ST.differences(f(m, lp[0], lp[1], lp[5]), ref)
            assert not diff, (what, name, diff[:5])


def test_the_lane_model_and_four_wrong_evaluators(table):
    """The lane model walks a matrix as the kernel's lanes do; right, it agrees with the loop reference on every 256-lane LP
    of the table, and each of its four flaws is visible somewhere in the table."""
    rows, refs, _ = table
    small = [(name, lp, ref) for (name, lp), ref in zip(rows, refs) if lp[0] * lp[1] <= 4000]
    assert len(small) > 100
    for name, lp, ref in small:
        diff = ST.differences(ST.lane_model(lp), ref)
        assert not diff, (name, diff[:5])
    for flaw in ST.FLAWS:
        caught = next((name for name, lp, ref in small if ST.differences(ST.lane_model(lp, flaw), ref)), None)
        print(flaw, "->", caught)
        assert caught is not None, flaw
    # ... and where: the thresholds and the NaN rule by the IEEE block, the lost lane by the first planted LP with G >= 2
    ieee = small[0]
    assert ieee[0] == "IEEE rules, small"
    for flaw in ("inclusive thresholds", "NaN propagates"):
        assert ST.differences(ST.lane_model(ieee[1], flaw), ieee[2]), flaw
    for name, lp, ref in small:
        if name.startswith("planted") and not name.endswith("G 1"):
            lost = {d[0] for d in ST.differences(ST.lane_model(lp, "skips the last lane"), ref)}
            assert lost >= ({"col_up", "col_dn"} if "pass 1" in name else {"row_lo", "row_hi"}), (name, lost)


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    from yalps_amd import build, _native
    build.build_lpsens()
    build.build_hip()
    assert _native.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return _native


@pytest.mark.gpu
def test_sensitivity_many_against_the_exact_reference(gpu, oracle, exact):
    """The same models through the real sensitivity_many in one call, against the same exact answers by the same rule.
    Worst disagreement measured on an MI355X: 1.75e-11, the same figure as through the oracle (the solve is bit for bit its)."""
    from yalps_amd import solve as S
    from tests.test_lp_batch import same_solution
    stats = {}
    results = S.sensitivity_many([row[2] for row in exact], [row[3] for row in exact], stats)
    assert stats["batched"] == len(exact) and stats["large"] == 0 and all(k["kernel"] in KERNELS for k in stats["kernels"])
    worst, bad = worst_of(results, exact)
    print("worst disagreement", worst)
    assert not bad, bad[:10]
    for (name, _, model, options, _), r in zip(exact, results):
        assert same_solution(r, S.solve(model, options)), name


def launches(lps):
    """[(kernel, class, LPs)] a batch must be launched as."""
    count = {}
    for lp in lps:
        cls = LB.size_class(lp[0], lp[1])
        kernel = next(k for k, (c, check) in KERNELS.items() if check == lp[7] and (c == cls or (c == 0 and cls < 3)))
        count[(kernel, cls)] = count.get((kernel, cls), 0) + 1
    return sorted((k, c, n) for (k, c), n in count.items())


@pytest.mark.gpu
def test_the_epilogue_on_the_table(gpu, oracle, table):
    """The table as one shuffled batch, checkCycles off and on: 0 pivots and the matrix bit for bit the input, the five arrays
    against the loop reference; then once more on the same handle in another order."""
    from tests.test_lp_sensitivity import launches_of
    rows, refs, _ = table
    lps = [(*lp[:7], check) for check in (False, True) for _, lp in rows]
    names = [name for _ in (0, 1) for name, _ in rows]
    want = refs + refs
    answers = {}

    def answer(k):
        j = k % len(rows)  # (checkCycles does not change the oracle's answer of an LP that takes 0 pivots)
        if j not in answers:
            answers[j] = LB.oracle_answer(oracle, rows[j][1])
            assert answers[j]["n_pivots"] == 0 and answers[j]["status"] == "optimal"
        return answers[j]

    s = gpu.LpSens(0)
    try:
        for seed in (5, 6):
            order = [int(k) for k in np.random.default_rng(seed).permutation(len(lps))]
            out = s.solve([lps[k] for k in order], keep_tableaux=True)
            bad = []
            for i, k in enumerate(order):
                LB.check_lp(s, i, out, answer(k), lps[k], label=names[k])
                assert int(out[2][i]) == 0 and LB.same_words(s.tableau(i), LB.scatter(lps[k])), names[k]
                diff = ST.differences(s.ranges(i), want[k])
                if diff:
                    got = s.ranges(i)
                    bad.append((names[k], lps[k][7], [(a, j, got[ST.NAMES.index(a)][j], want[k][ST.NAMES.index(a)][j]) for a, j in diff[:4]]))
            assert not bad, (len(bad), bad[:6])
            info = s.info()
            assert info["reruns"] == 0 and launches_of(info) == launches(lps)
            assert {k for k, _, _ in launches_of(info)} == set(KERNELS)
    finally:
        s.close()
