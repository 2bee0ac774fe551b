"""The host models of linprog_batch, milp_batch and milp_batch_free -- the call objects whose oracle_answer / expected the GPU tests
compare the device with, bit for bit -- against HiGHS on the problem as the caller stated it (tests/_independent.py, which shares
no code with the product or with its numpy restatement).  No GPU: a convention that kernel and restatement got wrong together
shows here.  The recorded answers are tests/golden/independent_{lp,milp}.json.gz; where scipy imports they are checked against a
fresh run."""
import numpy as np
import pytest

from tests import _independent as I
from tests import _independent_models as IM

LP_FAMILIES = ("LP plain", "LP bounded", "LP free")
MILP_FAMILIES = ("MILP plain", "MILP bounded", "MILP free")
MIN_WITH_NODES = 24           # optimal cases whose trees consumed nodes, per MILP family
MIN_NEGATIVE = 8              # of milp_batch_free's: an optimum with a negative integer


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native
    return _native


@pytest.fixture(scope="module")
def lps():
    return I.load("lp")


@pytest.fixture(scope="module")
def milps():
    return I.load("milp")


@pytest.fixture(scope="module")
def lp_models(oracle, lps):
    """{group name: the host model's answers}, computed once."""
    return {g["name"]: IM.lp_answers(oracle, g) for g in lps}


@pytest.fixture(scope="module")
def milp_models(nat, oracle, milps):
    return {g["name"]: IM.milp_rows(g, nat=nat, oracle=oracle) for g in milps}


def same_operands(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in I.OPERANDS)


def header(g):
    return {k: v for k, v in g.items() if k not in ("cases", "dropped")}


def test_the_lp_fixture_is_what_scipy_gives_now(lps):
    pytest.importorskip("scipy")
    fresh = [I.solved_lp(I.generate(g)) for g in I.lp_groups()] + [I.solved_lp(g) for g in I.ending_groups("lp")]
    assert [g["name"] for g in fresh] == [g["name"] for g in lps]
    for new, old in zip(fresh, lps):
        assert header(new) == header(old) and new["dropped"] == old["dropped"], new["name"]
        assert len(new["cases"]) == len(old["cases"]), new["name"]
        for a, b in zip(new["cases"], old["cases"]):
            assert same_operands(a, b), new["name"]
            d = I.lp_differences(new, a, a["answer"], b["answer"])
            assert I.within({k: v for k, v in d.items() if not k.startswith("own ")}, I.tolerance(new)), (new["name"], d)


def test_the_milp_fixture_is_what_scipy_gives_now(milps):
    """The recorded MILPs are generated ones, in order, and HiGHS answers them now as recorded.  (Which of the generated ones are
    recorded is the oracle-driven search's decision: test_our_milp_model_against_highs runs it on every recorded case.)"""
    pytest.importorskip("scipy")
    made = {g["name"]: g for g in [I.generate(g) for g in I.milp_groups()] + I.ending_groups("milp")}
    assert list(made) == [g["name"] for g in milps]
    for old in milps:
        new = made[old["name"]]
        assert header(new) == header(old), old["name"]
        rest = iter(new["cases"])
        for b in old["cases"]:
            a = next((a for a in rest if same_operands(a, b)), None)
            assert a is not None, old["name"]
            now, want = I.scipy_milp(old, a), b["answer"]
            assert now["status"] == want["status"], old["name"]
            if now["status"] == "optimal":
                assert abs(now["objective"] - want["objective"]) <= I.tolerance(old)["objective"], old["name"]


def test_every_recorded_lp_is_unique_and_few_were_dropped(lps):
    for family in LP_FAMILIES:
        groups = [g for g in lps if g["family"] == family]
        generated, kept = sum(g["generated"] for g in groups), sum(len(g["cases"]) for g in groups)
        assert all(g["dropped"] == g["generated"] - len(g["cases"]) for g in groups)
        print("%s: generated %d, dropped %d, kept %d" % (family, generated, generated - kept, kept))
        assert generated - kept <= I.MAX_DROPPED * generated, family
        assert all(len(g["cases"]) >= 1 for g in groups), family  # (no shape is lost)
        for g in groups:
            for case in g["cases"]:
                assert I.unique(g, case, case["answer"]), g["name"]
                cert = I.certificate(g, case, case["answer"]["x"], case["answer"]["objective"], [case["answer"][k] for k in I.MARGINALS])
                assert max(cert.values()) <= I.MARGIN, (g["name"], cert)  # (HiGHS's own answer is an optimal one, in the caller's terms)


def test_the_lp_table_reaches_what_it_is_for(lps):
    names = {g["name"]: g for g in lps}
    assert {I.bucket(g) for g in lps if g["family"] == "LP plain"} == {"small", "large"}
    for family in LP_FAMILIES:
        groups = [g for g in lps if g["family"] == family]
        assert {g["maximize"] for g in groups} == {True, False} and {g["m_eq"] > 0 for g in groups} == {True, False}, family
        assert {"%s %s" % (family.split()[1], shape) for shape in ("100x99", "160x152", "8170x31")} <= set(names), family
    assert {g["n"] for g in lps if g["n"] in I.LANES} == set(I.LANES)
    bounded = [g for g in lps if g["family"] == "LP bounded"]
    assert any(g["has_lb"] and g["upper"] is None for g in bounded) and any(not g["has_lb"] and g["upper"] is True for g in bounded)
    assert any(g["has_lb"] and isinstance(g["upper"], list) and any(c["lb"].min() < 0.0 for c in g["cases"]) for g in bounded)
    free = [g for g in lps if g["family"] == "LP free"]
    assert any(g["free"] is True for g in free) and any(not g["has_lb"] and g["upper"] is None for g in free)
    assert any(set(I.free_idx(g)) & set(I.upper_idx(g)) for g in free)
    assert any((c["answer"]["x"][I.free_idx(g)] < -0.5).any() for g in free for c in g["cases"])
    ends = [c["answer"]["status"] for g in lps if g["family"] == "endings" for c in g["cases"]]
    assert ends == ["optimal", "infeasible", "infeasible", "optimal", "unbounded", "optimal", "unbounded"]


def test_the_milp_table_keeps_its_floors(milps):
    for family in MILP_FAMILIES:
        groups = [g for g in milps if g["family"] == family]
        cases = [(g, c) for g in groups for c in g["cases"]]
        generated = sum(g["generated"] for g in groups)
        print("%s: generated %d, dropped %d, kept %d" % (family, generated, generated - len(cases), len(cases)))
        assert all(c["answer"]["status"] == "optimal" for _, c in cases)
        assert sum(c["answer"]["nodes"] > 0 for _, c in cases) >= MIN_WITH_NODES, family
        assert any(g["binaries"] for g in groups) and any(I.bucket(g) == "large" and g["cases"] for g in groups), family
        if family != "MILP plain":  # a fractional lb at an integer variable that the optimum rests on: ceil(lb), above lb
            assert any(abs(c["answer"]["x"][j] - np.ceil(c["lb"][j])) < 0.5 and c["lb"][j] != np.ceil(c["lb"][j])
                       for g, c in cases if g["has_lb"] for j in g["integers"] if j not in I.free_idx(g)), family
    free = [(g, c) for g in milps if g["family"] == "MILP free" for c in g["cases"]]
    negative = [any(c["answer"]["x"][j] < -0.5 for j in g["integers"]) for g, c in free]
    assert sum(negative) >= MIN_NEGATIVE
    ends = [c["answer"]["status"] for g in milps if g["family"] == "endings" for c in g["cases"]]
    assert ends.count("infeasible") == 2 and "unbounded" in ends and ends.count("optimal") == 3, ends


def report(measured):
    for key, row in measured.items():
        print("%-22s %s" % (" / ".join(key), "  ".join("%s %.2g" % kv for kv in row.items())))


def test_our_lp_model_against_highs(lps, lp_models):
    """Status, x, objective and the four marginals of the host model against the fixture, and the certificate of the model's own
    answer.  Prints the maxima behind I.MEASURED."""
    measured, bad = {}, []
    for g in lps:
        for i, (case, ans) in enumerate(zip(g["cases"], lp_models[g["name"]])):
            d = I.lp_differences(g, case, ans, case["answer"])
            I.merged(measured.setdefault((g["family"], I.bucket(g)), {}), d)
            if not I.within(d, I.tolerance(g)):
                bad.append((g["name"], i, d))
    report(measured)
    assert not bad, bad[:5]
    assert set(measured) == {k for k in I.MEASURED if not k[0].startswith("MILP")}


def test_our_milp_model_against_highs(milps, milp_models):
    """Every recorded MILP ends in the host search as HiGHS says -- "optimal" within the budget for the generated ones -- with
    HiGHS's objective, at an x that is feasible and integral in the caller's terms and gives that objective."""
    measured, bad = {}, []
    for g in milps:
        for i, (case, row) in enumerate(zip(g["cases"], milp_models[g["name"]])):
            d = I.milp_differences(g, case, row, case["answer"])
            I.merged(measured.setdefault((g["family"], I.bucket(g)), {}), d)
            if not I.within(d, I.tolerance(g)) or int(row["nodes"]) != case["answer"]["nodes"]:
                bad.append((g["name"], i, d))
    report(measured)
    assert not bad, bad[:5]


def rejecting(groups, answers_of, differences, mutant):
    """The (group, case) pairs whose recorded answer rejects the mutant."""
    out = []
    for g in groups:
        for i, (case, ans) in enumerate(zip(g["cases"], answers_of(g, mutant))):
            if not I.within(differences(g, case, ans, case["answer"]), I.tolerance(g)):
                out.append((g["name"], i))
    return out


@pytest.mark.parametrize("mutant", sorted(IM.LP_MUTANTS))
def test_the_lp_fixture_rejects_each_wrong_convention(oracle, lps, mutant):
    small = [g for g in lps if I.bucket(g) == "small" and g["family"] != "LP plain"]
    told = rejecting(small, lambda g, m: IM.lp_answers(oracle, g, m), I.lp_differences, mutant)
    print(mutant, len(told), told[:4])
    assert bool(told) == (mutant not in IM.UNTELLABLE), mutant


@pytest.mark.parametrize("mutant", sorted(IM.MILP_MUTANTS))
def test_the_milp_fixture_rejects_each_wrong_convention(nat, oracle, milps, mutant):
    small = [g for g in milps if I.bucket(g) == "small" and g["family"] != "MILP plain"]
    told = rejecting(small, lambda g, m: IM.milp_rows(g, m, nat=nat, oracle=oracle), I.milp_differences, mutant)
    print(mutant, len(told), told[:4])
    assert bool(told) == (mutant not in IM.UNTELLABLE), mutant
