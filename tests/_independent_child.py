"""The child processes of tests/test_independent.py (TEST INFRASTRUCTURE; tests/_lp_dense.py says why children: torch first).  They
read the recorded groups of tests/_independent.py -- numpy and the files only, no scipy -- call nothing but the public functions,
one batched call per group, and write everything to one .npz each:

  child "lp"    linprog_batch(duals=True) on every LP group; then one linprog_objective_bounds with every operand requiring grad
                per family (GRADIENT_GROUPS) and objective.sum().backward()
  child "milp"  milp_batch / milp_batch_free on every MILP group
"""
import sys

import numpy as np

from tests import _independent as I

GRADIENT_GROUPS = ("plain n=8 eq", "bounded n=7 subset eq", "free n=6 in upper eq max")
GRADIENTS = ("c", "b_ub", "b_eq", "lb", "ub")


def _torch_first():
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    return torch


def arguments(torch, group, leaf=False):
    """(the five operands, the keywords the caller would write) of the group's one call."""
    def dev(a):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t.requires_grad_() if leaf else t
    c, A_ub, b_ub, A_eq, b_eq, lb, ub = (dev(a) for a in I.stacked(group))
    kw = dict(maximize=group["maximize"])
    if lb is not None:
        kw["lb"] = lb
    if ub is not None:
        kw.update(ub=ub, upper=True if group["upper"] is True else list(group["upper"]))
    if group["free"] is True or group["free"]:
        kw["free"] = True if group["free"] is True else list(group["free"])
    return (c, A_ub, b_ub, A_eq, b_eq), kw


def kernels_of(stats):
    return np.array(" ".join(k["kernel"] for k in stats["kernels"]))


def child_lp(path):
    torch = _torch_first()
    from yalps_amd import tensors
    out = {}
    groups = I.load("lp")
    for g in groups:
        ops, kw = arguments(torch, g)
        stats = {}
        got = tensors.linprog_batch(*ops, duals=True, stats=stats, **kw)
        put = {"x": got.x, "objective": got.objective, "status": got.status, "ineqlin": got.ineqlin, "eqlin": got.eqlin, "lower": got.reduced_costs}
        if "ub" in kw:
            put["upper"] = got.upper
        out.update({"%s/%s" % (g["name"], k): t.cpu().numpy() for k, t in put.items()})
        out["%s/names" % g["name"]] = np.array(" ".join(tensors.status_names(got.status)))
        out["%s/kernels" % g["name"]] = kernels_of(stats)
        out["%s/aux" % g["name"]] = np.array([k["aux"] for k in stats["kernels"]], np.int64)
    for g in groups:
        if g["name"] in GRADIENT_GROUPS:
            ops, kw = arguments(torch, g, leaf=True)
            objective, duals = tensors.linprog_objective_bounds(*ops, **kw)
            assert objective.grad_fn is not None
            objective.sum().backward()
            given = dict(zip(("c", "A_ub", "b_ub", "A_eq", "b_eq"), ops), lb=kw.get("lb"), ub=kw.get("ub"))
            for k in GRADIENTS:
                if given[k] is not None:
                    out["%s/grad_%s" % (g["name"], k)] = given[k].grad.cpu().numpy()
            out["%s/grad status" % g["name"]] = duals.status.cpu().numpy()
    np.savez(path, **out)


def child_milp(path):
    torch = _torch_first()
    from yalps_amd import tensors
    out = {}
    for g in I.load("milp"):
        ops, kw = arguments(torch, g)
        stats = {}
        solve = {"milp_batch": tensors.milp_batch, "milp_batch_free": tensors.milp_batch_free}[g["fn"]]
        got = solve(*ops, integers=list(g["integers"]), binaries=list(g["binaries"]), max_iterations=g["max_iterations"], stats=stats, **kw)
        out.update({"%s/%s" % (g["name"], k): getattr(got, k).cpu().numpy() for k in ("x", "objective", "status", "nodes")})
        out["%s/names" % g["name"]] = np.array(" ".join(tensors.status_names(got.status)))
        out["%s/kernels" % g["name"]] = kernels_of(stats)
        out["%s/overflows" % g["name"]] = np.int64(stats["overflows"])
    np.savez(path, **out)


if __name__ == "__main__":
    {"lp": child_lp, "milp": child_milp}[sys.argv[1]](sys.argv[2])
