"""linprog_batch(duals=True), linprog_objective_bounds, milp_batch and milp_batch_free on the GPU against HiGHS's recorded answers to
the problems as the caller states them (tests/golden/independent_{lp,milp}.json.gz, made by tests/_independent.py, which shares no
code with the product or with its numpy restatement; tests/test_independent_model.py holds the host models to the same answers
without a GPU).  The work runs in two child processes that import torch first (tests/_lp_dense.py says why) and call only the
public functions, one batched call per group of cases.  The bounds are I.TOL: twice what the host models, which the device equals
bit for bit in the other tests, were measured to differ from HiGHS by."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _independent as I
from tests import _independent_child as IC
from tests import _independent_models as IM
from tests import _batch_shapes as BS
from tests import _lp_batch as LB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("YALPS_MILPDENSE_ARENA", "YALPS_MILPDENSE_ARENA_MAX", "YALPS_MILPDENSE_HIST", "YALPS_MILPDENSE_GRID", "YALPS_LPDENSE_HIST",
         "YALPS_MILPDENSE_CUS", "YALPS_MILPDENSE_PER_CU", "YALPS_LPDENSE_CUS", "YALPS_LPDENSE_PER_CU")
LP_GROUPS = [g["name"] for g in I.lp_groups()] + [g["name"] for g in I.ending_groups("lp")]
MILP_GROUPS = [g["name"] for g in I.milp_groups()] + [g["name"] for g in I.ending_groups("milp")]
LP_KERNEL = {"plain": "lp_dense_kernel", "bounded": "lp_dense_bounds_kernel", "free": "lp_dense_free_kernel"}
MILP_KERNELS = {"plain": ("milp_dense_root_kernel", "milp_dense_solution_kernel<256>"),
                "bounded": ("milp_dense_bounds_root_kernel", "milp_dense_bounds_solution_kernel<256>"),
                "free": ("milp_dense_free_root_kernel", "milp_dense_free_solution_kernel<256>")}


def run_child(tmp_path_factory, which):
    from yalps_amd import build
    for make in (build.build_milpdense, build.build_milptree, build.build_milpbatch, build.build_lpdense, build.build_hip):
        make()
    path = str(tmp_path_factory.mktemp("independent") / (which + ".npz"))
    clean = {k: v for k, v in os.environ.items() if k not in HOOKS}
    child = subprocess.run([sys.executable, "-m", "tests._independent_child", which, path], cwd=ROOT, capture_output=True, text=True, timeout=600,
                           env=clean)
    assert child.returncode == 0, child.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def lps():
    return {g["name"]: g for g in I.load("lp")}


@pytest.fixture(scope="module")
def milps():
    return {g["name"]: g for g in I.load("milp")}


@pytest.fixture(scope="module")
def ran_lp(tmp_path_factory):
    return run_child(tmp_path_factory, "lp")


@pytest.fixture(scope="module")
def ran_milp(tmp_path_factory):
    return run_child(tmp_path_factory, "milp")


def of(ran, name):
    return {k[len(name) + 1:]: v for k, v in ran.items() if k.startswith(name + "/")}


def form(w, h):
    cls = LB.size_class(w, h)
    return "<%d%s>" % (1024 if cls >= 3 else 256, ",lds" if cls < 4 else "")


def lp_answer(got, names, i, k):
    return dict(status=names[i], x=got["x"][i], objective=got["objective"][i], ineqlin=got["ineqlin"][i], eqlin=got["eqlin"][i],
                lower=got["lower"][i], upper=got["upper"][i] if "upper" in got else np.zeros(k))


@pytest.mark.parametrize("name", LP_GROUPS)
def test_linprog_batch_against_highs(ran_lp, lps, name):
    """Status, x, objective and the four marginals within I.TOL of the recorded answer, the certificate's residuals of the device's
    own outputs within I.TOL too, and the kernel by name."""
    g, got = lps[name], of(ran_lp, name)
    names, tol, worst = str(got["names"]).split(), I.tolerance(g), {}
    assert len(names) == len(g["cases"]) > 0
    for i, case in enumerate(g["cases"]):
        d = I.lp_differences(g, case, lp_answer(got, names, i, len(I.upper_idx(g))), case["answer"])
        I.merged(worst, d)
        assert I.within(d, tol), (name, i, d)
    print(name, {k: float("%.2g" % v) for k, v in worst.items()})
    call = IM.lp_call(g)
    assert str(got["kernels"]).split() == [LP_KERNEL[IM.kind_of(g)] + form(call.w, call.h)], (name, got["kernels"])
    assert got["aux"].tolist() == [int(BS.aux_hbm(call.w, call.h))]


def test_the_lp_calls_reach_every_form_of_the_three_kernels(ran_lp, lps):
    seen = {str(of(ran_lp, name)["kernels"]) for name in lps}
    want = {kernel + f for kernel in LP_KERNEL.values() for f in ("<256,lds>", "<1024,lds>", "<1024>")}
    assert want <= seen, want - seen
    for kind in ("plain", "bounded", "free"):
        assert int(of(ran_lp, kind + " 8170x31")["aux"][0]) == 1 and int(of(ran_lp, kind + " 160x152")["aux"][0]) == 0


@pytest.mark.parametrize("name", IC.GRADIENT_GROUPS)
def test_gradients_of_the_objective_are_highs_marginals(ran_lp, lps, name):
    """objective.sum().backward() with every operand requiring grad: c.grad = x, b_ub.grad = ineqlin, b_eq.grad = eqlin, lb.grad =
    lower with exactly +0.0 at the free variables, ub.grad = upper scattered over zeros."""
    g, got = lps[name], of(ran_lp, name)
    tol, idx, fr = I.tolerance(g), I.upper_idx(g), I.free_idx(g)
    assert (got["grad status"] == 0).all() and len(g["cases"]) >= 14
    for i, case in enumerate(g["cases"]):
        a = case["answer"]
        scattered = np.zeros(g["n"])
        scattered[idx] = a["upper"]
        for k, want, bound in (("c", a["x"], tol["x"]), ("b_ub", a["ineqlin"], tol["ineqlin"]), ("b_eq", a["eqlin"], tol["eqlin"]),
                               ("lb", a["lower"], tol["lower"]), ("ub", scattered, tol["upper"])):
            if case[k] is None:
                assert "grad_" + k not in got
                continue
            grad = got["grad_" + k][i]
            assert np.abs(grad - want).max() <= bound, (name, i, k, np.abs(grad - want).max())
        if case["lb"] is not None:
            assert got["grad_lb"][i][fr].tobytes() == np.zeros(len(fr)).tobytes(), (name, i)
        if case["ub"] is not None:
            rest = [j for j in range(g["n"]) if j not in idx]
            assert got["grad_ub"][i][rest].tobytes() == np.zeros(len(rest)).tobytes(), (name, i)
    assert IM.kind_of(g) != "free" or (fr and g["has_lb"])


@pytest.mark.parametrize("name", MILP_GROUPS)
def test_milp_batch_against_highs(ran_milp, milps, name):
    """Status and objective within I.TOL of the recorded answer; x feasible and integral in the caller's terms with c . x the
    objective; the root, tree and epilogue kernels by name."""
    g, got = milps[name], of(ran_milp, name)
    names, tol, worst = str(got["names"]).split(), I.tolerance(g), {}
    assert len(names) == len(g["cases"]) > 0 and int(got["overflows"]) == 0
    for i, case in enumerate(g["cases"]):
        d = I.milp_differences(g, case, dict(status=names[i], x=got["x"][i], objective=got["objective"][i]), case["answer"])
        I.merged(worst, d)
        assert I.within(d, tol), (name, i, d)
        assert int(got["nodes"][i]) == case["answer"]["nodes"], (name, i)
    print(name, {k: float("%.2g" % v) for k, v in worst.items()})
    call = IM.milp_call(g)
    root, epilogue = MILP_KERNELS[IM.kind_of(g)]
    kernels = str(got["kernels"]).split()
    assert kernels[0] == root + form(call.w, call.h) and kernels[-1] == epilogue, (name, kernels)
    assert set(kernels[1:-1]) == {"milp_tree_kernel" + form(call.w, call.hmax)}, (name, kernels)


def test_the_milp_calls_reach_the_large_forms(ran_milp, milps):
    roots = {str(of(ran_milp, name)["kernels"]).split()[0] for name in milps}
    assert {"milp_dense_root_kernel<256,lds>", "milp_dense_root_kernel<1024,lds>", "milp_dense_bounds_root_kernel<256,lds>",
            "milp_dense_bounds_root_kernel<1024>", "milp_dense_free_root_kernel<256,lds>", "milp_dense_free_root_kernel<1024>"} <= roots, roots
    g = milps["free milp 8170x31"]
    call = IM.milp_call(g)
    assert BS.aux_hbm(call.w, call.h)


def test_the_endings_keep_the_documented_conventions(ran_lp, ran_milp, lps, milps):
    """"infeasible": NaN everywhere.  "unbounded": +-inf as the objective in the call's direction, +inf at the unbounded variable --
    -inf where that is the twin of a free variable -- the effective lower bound at the others, NaN marginals."""
    nan_row = lambda a: bool(np.isnan(a).all())
    crossed = of(ran_lp, "endings bounded")
    assert str(crossed["names"]).split() == ["optimal", "infeasible", "infeasible"]
    for i in (1, 2):
        assert all(nan_row(crossed[k][i]) for k in ("x", "objective") + I.MARGINALS)
    free, lb = of(ran_lp, "endings free"), lps["endings free"]["cases"][1]["lb"]
    assert str(free["names"]).split() == ["optimal", "unbounded"]
    assert free["x"][1].tolist() == [-np.inf, lb[1]] and free["objective"][1] == np.inf and all(nan_row(free[k][1]) for k in I.MARGINALS)
    assert free["x"][0][0] < 0.0
    unlisted = of(ran_lp, "endings unlisted")
    assert str(unlisted["names"]).split() == ["optimal", "unbounded"]
    assert unlisted["x"][1].tolist() == [lb[0], np.inf] and unlisted["objective"][1] == np.inf and all(nan_row(unlisted[k][1]) for k in I.MARGINALS)
    assert unlisted["x"][0][1] > lps["endings unlisted"]["cases"][0]["ub"][1]  # (the ub entry of a variable `upper` does not list is not read)
    crossed = of(ran_milp, "endings bounded")
    assert str(crossed["names"]).split() == ["optimal", "infeasible", "infeasible"]
    assert nan_row(crossed["x"][1:]) and nan_row(crossed["objective"][1:]) and not crossed["nodes"][1:].any()
    unlisted = of(ran_milp, "endings unlisted")
    assert str(unlisted["names"]).split() == ["optimal", "unbounded"]
    # (x1 is integer there: its effective lower bound is ceil(lb); the column found unbounded is a row's slack, so no variable shows +inf)
    assert unlisted["x"][1].tolist() == [lb[0], np.ceil(lb[1])] and unlisted["objective"][1] == np.inf
    assert str(of(ran_milp, "endings free")["names"]).split() == [c["answer"]["status"] for c in milps["endings free"]["cases"]]
