"""Helpers of tests/test_independent_model.py and tests/test_independent.py (TEST INFRASTRUCTURE): the host model of every group of
tests/_independent.py -- the call objects the GPU tests of each function use (LD.Call, LBD.BCall, LF.FCall with oracle_answer;
NM.Call, NB.BCall, NF.FCall with expected) -- answered in _independent's vocabulary, and the mutants: the same models with one
convention deliberately WRONG, to show that the comparison with HiGHS can fail.
"""
import numpy as np

from tests import _lp_dense as LD
from tests import _lp_dense_bounds as LBD
from tests import _lp_dense_free as LF
from tests import _np_dense_duals as DD
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB
from tests import _np_milp_dense_free as NF

# mutant -> what it gets wrong (the list of the conventions kernel and restatement could get wrong together)
LP_MUTANTS = {
    "shift by -lb": "the sign of the shift by lb: the model is built and read back with -lb",
    "bound row without -1": "FD's flaw: +0.0 in the twin's cell of the bound row of a free variable",
    "upper negated under maximize": "the sign of `upper` under maximize=True",
    "reduced without twin": "FD's flaw: the reduced cost of a free variable without its twin's term",
    "objective not moved back": "the objective left in x': c . l_eff missing",
    "lb read": "FD's flaw: lb read at a free variable, which stays split",
    "free ignored": "a free variable held by x >= lb (x >= 0 without lb)",
    "lb added twice": "x moved back by 2 l_eff",
}
MILP_MUTANTS = {
    "floor at an integer": "floor(lb) in place of ceil(lb) at the integer variables",
    "lb read at a free variable": "NF's flaw: l_eff = lb, ceil(lb) at an integer one, at a free variable, which stays split",
    "ceil at a free integer": "NF's flaw: l_eff = ceil(lb) at a free integer variable, which stays split",
    "free ignored": "a free variable held by x >= lb (x >= 0 without lb)",
    "twin not integer": "NF's flaw: the twins of the free integer variables are never branched on",
    "objective not moved back": "the objective left in x'",
}
# A free variable that stays split, x = l + p - q with p, q >= 0, is as free with one l as with another, and p - q is whole where x - l
# is: these three flaws move words (the other tests of each function tell them bit by bit, and by NaN in lb), not the problem
# solved.  And at an optimum that is unique() one of p, q is basic, the other column is its negation, so both reduced costs are zero
# and "reduced without twin" reports the same zero (it shows where both halves are nonbasic: an optimum that is not a vertex of the
# caller's problem, which tests/test_lp_dense_free_model.py reaches with precision = 0.25).  No recorded case can reject these four; the
# model test asserts exactly that, so that the list does not claim more than it shows.
UNTELLABLE = ("lb read", "reduced without twin", "lb read at a free variable", "ceil at a free integer")
FD_FLAWS = ("bound row without -1", "reduced without twin", "lb read")
NF_FLAWS = ("lb read at a free variable", "ceil at a free integer", "twin not integer")


def kind_of(group, mutant=None):
    fr = (group["free"] is True or len(group["free"]) > 0) and mutant != "free ignored"
    return "free" if fr else "bounded" if group["has_lb"] or group["upper"] is not None else "plain"


def _lps(group, lb_of=lambda lb: lb):
    rows = []
    for case in group["cases"]:
        rows.append((case["c"], case["A_ub"], case["b_ub"], case["A_eq"], case["b_eq"], None if case["lb"] is None else lb_of(case["lb"]), case["ub"]))
    return rows


def lp_call(group, lb_of=lambda lb: lb, mutant=None):
    kind, rows = kind_of(group, mutant), _lps(group, lb_of)
    upper = True if group["upper"] is None else group["upper"]
    if kind == "plain":
        return LD.Call(group["name"], [r[:5] for r in rows], maximize=group["maximize"])
    if kind == "bounded":
        return LBD.BCall(group["name"], rows, upper, maximize=group["maximize"])
    return LF.FCall(group["name"], rows, upper, group["free"], maximize=group["maximize"])


def lp_answers(oracle, group, mutant=None):
    """[dict(status, x, objective, ineqlin, eqlin, lower, upper)] of the group's host model; mutant: None or one of LP_MUTANTS."""
    assert mutant is None or mutant in LP_MUTANTS, mutant
    kind = kind_of(group, mutant)
    call = lp_call(group, (lambda lb: -lb) if mutant == "shift by -lb" else (lambda lb: lb), mutant)
    sign = 1.0 if group["maximize"] else -1.0
    out = []
    for i, case in enumerate(group["cases"]):
        if kind == "free":
            ref = call.oracle_answer(oracle, i, flaw=mutant if mutant in FD_FLAWS else None)
        else:
            ref = call.oracle_answer(oracle, i)
        if kind == "plain":
            ineqlin, eqlin, reduced = DD.marginals_of(ref, call.n, call.m_ub, call.m_eq, sign)
            upper = np.zeros(0)
        else:
            ineqlin, eqlin, reduced, upper = (ref[k] for k in LBD.OUTPUTS)
        ans = dict(status=ref["status"], x=np.array(ref["x"], np.float64), objective=float(ref["objective"]), ineqlin=ineqlin, eqlin=eqlin,
                   lower=reduced, upper=upper)
        low = np.zeros(call.n) if case["lb"] is None else np.array(case["lb"], np.float64)
        if kind == "free":
            low[list(call.fidx)] = 0.0
        if mutant == "upper negated under maximize" and group["maximize"]:
            ans["upper"] = -ans["upper"]
        if mutant == "objective not moved back":
            ans["objective"] -= float(case["c"] @ low)
        if mutant == "lb added twice":
            ans["x"] = ans["x"] + low
        out.append(ans)
    return out


def milp_call(group, mutant=None):
    lb_of = lambda lb: lb
    if mutant == "floor at an integer":
        ints = list(group["integers"])

        def lb_of(lb):
            lb = lb.copy()
            lb[ints] = np.floor(lb[ints])
            return lb
    kind, rows = kind_of(group, mutant), _lps(group, lb_of)
    upper = True if group["upper"] is None else group["upper"]
    kw = dict(integers=group["integers"], binaries=group["binaries"], maximize=group["maximize"], max_iterations=group["max_iterations"])
    if kind == "plain":
        return NM.Call(group["name"], [r[:5] for r in rows], **kw)
    if kind == "bounded":
        return NB.BCall(group["name"], rows, upper, **kw)
    call = NF.FCall(group["name"], rows, upper, group["free"], **kw)
    return call.flawed(mutant) if mutant in NF_FLAWS else call


def milp_rows(group, mutant=None, nat=None, oracle=None):
    """NM / NB / NF.expected's rows of the group's host model; mutant: None or one of MILP_MUTANTS."""
    assert mutant is None or mutant in MILP_MUTANTS, mutant
    if nat is None:
        from yalps_amd import _native as nat
    if oracle is None:
        from tests import _oracle
        oracle = _oracle.load()
    call = milp_call(group, mutant)
    rows = {"plain": NM, "bounded": NB, "free": NF}[kind_of(group, mutant)].expected(nat, oracle, call)
    if mutant == "objective not moved back":
        for row in rows:
            if "objective_shifted" in row:
                row["objective"] = row["objective_shifted"]
    return rows
