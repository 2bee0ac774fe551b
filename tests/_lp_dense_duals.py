"""Helpers of tests/test_lp_dense_duals.py (TEST INFRASTRUCTURE): the calls the GPU tests of yalps_lpdense_solve_duals /
linprog_batch(duals=True) / linprog_objective make, and the two child processes that make them (tests/_lp_dense.py says why
children: torch first).  Each child writes everything its calls left behind to one .npz; the tests compare those files with
tests/_np_dense_duals.py::dense_marginals of the C oracle's answer.

  table(oracle)   [Call]: every call of the child "table" through _native.LpDense with kept tableaux and all seven outputs
  child "table"   the table; the same LPs with none or some of the three new pointers; then linprog_batch(duals=True) on
                  views, on a side stream, with B = 0, with a host pointer; next to sensitivity_many; then linprog_objective
  child "hist"    under YALPS_LPDENSE_HIST=4: the rerun writes the marginals
"""
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _lp_dense as LD
from tests import _nonfinite as NF
from tests import _np_dense as ND
from tests import _np_dense_duals as DD

INF = float("inf")
SENTINEL = -7.0
MARGINALS = ("ineqlin", "eqlin", "reduced")
STATUS_LPS = 2100             # more than class 0's grid of 8 x 256 workgroups
STATUS_BUDGET = 2.0           # max_pivots of the call "statuses": an LP of more pivots ends "cycled"
INEQ_SHAPE = (2, 1025)        # (n, m_ub): ineqlin's lanes go round
EQ_SHAPE = (2, 513)           # (n, m_eq)
NONFINITE = ("N1", "N2")      # the non-finite families that end optimal with a NaN in row 0 (asserted by the test)


def ineq_stride_lp():
    """maximize x0 + 2 x1 under 1025 rows of which only rows 511 and 1024 bind (x1 <= 2, x0 <= 3): the duals that are not zero sit
    at the last lane of a round of 256 and at the first lane of the second round of 1024."""
    n, m = INEQ_SHAPE
    rng = np.random.default_rng(20261027)
    A = rng.integers(1, 4, (m, n)).astype(np.float64)
    b = 1000.0 + rng.integers(0, 9, m).astype(np.float64)
    A[511], b[511] = (0.0, 1.0), 2.0
    A[1024], b[1024] = (1.0, 0.0), 3.0
    return np.array([1.0, 2.0]), A, b, None, None


def eq_stride_lp():
    """513 equalities through the one point (3, 2), small integers: feasible, and all but two of them redundant."""
    n, m = EQ_SHAPE
    rng = np.random.default_rng(20261028)
    A = rng.integers(0, 4, (m, n)).astype(np.float64)
    A[0], A[512] = (1.0, 0.0), (0.0, 1.0)
    return np.array([1.0, 3.0]), None, None, A, A @ np.array([3.0, 2.0])


def bound_calls(oracle):
    """The first and the last LDS class bound from below (256 and 1024 lanes), the last one with checkCycles too."""
    shapes = [s for j, s in enumerate(LD.bound_shapes()) if j % 2 == 0]
    out = []
    for (k, w, h), check in ((shapes[0], False), (shapes[-1], False), (shapes[-1], True)):
        assert LB.size_class(w, h) == k
        out.append(LD.tableau_call("class %d bound under%s" % (k, " check" if check else ""), [oracle.dense_lp(h - 1, w - 1, 3)], w, h, check=check))
    return out


def names():
    shapes = [s for j, s in enumerate(LD.bound_shapes()) if j % 2 == 0]
    out = ["n=0", "n=1 m=1", "n=2 m=1", "n=1, both kinds", "equalities only", "inequalities only", "both kinds, minimize",
           "both kinds, maximize", "both kinds, minimize, check"]
    out += ["precision 1e-08 n=%d" % n for n, _ in LD.PRECISION_SHAPES] + ["ineqlin strides", "eqlin strides"]
    out += ["class %d bound under" % shapes[0][0], "class %d bound under" % shapes[-1][0], "class %d bound under check" % shapes[-1][0]]
    out += ["HBM odd n 301x280", "aux", "aux check", "statuses", "both slacks", "Degenerate Max", "Degenerate Min", "hist clean"]
    out += ["nonfinite %s" % f for f in NONFINITE]
    return out


def table(oracle):
    R, D = LD.random_call, oracle.dense_lp
    T = [R("n=0", 4, 0, 3, 0), R("n=1 m=1", 6, 1, 1, 0), R("n=2 m=1", 6, 2, 1, 0), R("n=1, both kinds", 8, 1, 2, 1),
         R("equalities only", 6, 9, 0, 4), R("inequalities only", 6, 8, 3, 0), R("both kinds, minimize", 8, 5, 4, 3),
         R("both kinds, maximize", 8, 5, 4, 3, maximize=True), R("both kinds, minimize, check", 8, 5, 4, 3, check=True)]
    T += [LD.precision_call(n, m, 1e-8) for n, m in LD.PRECISION_SHAPES]
    T += [LD.Call("ineqlin strides", [ineq_stride_lp()], maximize=True), LD.Call("eqlin strides", [eq_stride_lp()])]
    T += bound_calls(oracle)
    T.append(LD.tableau_call("HBM odd n 301x280", [D(300, 279, 3)], 280, 301))
    m_ub, n = LD.AUX_SHAPE
    assert BS.aux_hbm(n + 1, m_ub + 1)
    T += [LD.tableau_call("aux" + (" check" if check else ""), [D(m_ub, n, 3)], n + 1, m_ub + 1, max_pivots=INF, check=check) for check in (False, True)]
    T.append(R("statuses", STATUS_LPS, 4, 4, 0, maximize=True, max_pivots=STATUS_BUDGET))
    lp, maximize, precision = DD.both_slacks_lp()
    T.append(LD.Call("both slacks", [lp], maximize=maximize, precision=precision))
    for name in ("Degenerate Max", "Degenerate Min"):
        lp, maximize = DD.dense_from_case(name)
        T.append(LD.Call(name, [lp], maximize=maximize))
    T.append(LD.hist_call(oracle))
    M, N = LD.NONFINITE_SHAPE
    nf = {f: (seed, m) for f, seed, m in LD.nonfinite_families(oracle)}
    for f in NONFINITE:
        o = NF.options(f, M, N, nf[f][0])
        T.append(LD.tableau_call("nonfinite %s" % f, [nf[f][1]], N + 1, M + 1, precision=o["precision"], max_pivots=o["max_pivots"], check=o["check_cycles"]))
    assert [c.name for c in T] == names()
    return T


def partial_call():
    """The LPs of the calls with none / some of the three new pointers."""
    return LD.random_call("partial", 8, 5, 4, 3)


PARTIAL = ((), ("eqlin",), ("ineqlin", "reduced"), MARGINALS)


def gradient_call():
    """The LPs of the first linprog_objective test: the two minimised gradient LPs, and the first again with b_eq = -1 (A_eq > 0:
    infeasible)."""
    lps = [lp for lp, maximize in DD.gradient_lps() if not maximize]
    bad = list(lps[0])
    bad[4] = np.array([-1.0])
    return LD.Call("gradient rows", lps + [tuple(bad)], precision=DD.GRAD_PRECISION_A)


GRADIENT_WEIGHTS = (2.0, -0.5, 3.0)
SHARED_STEPS = (0.0, 0.125, 0.25)  # b_ub of the shared-operand test: the first gradient LP's, moved by these


def shared_call():
    lp = DD.gradient_lps()[0][0]
    return LD.Call("shared", [(lp[0], lp[1], lp[2] + d, lp[3], lp[4]) for d in SHARED_STEPS], precision=DD.GRAD_PRECISION_A)


def difference_calls(k):
    """Gradient LP k: (the call over c / b_ub / b_eq moved by GRAD_H, the call over A_ub / A_eq moved by GRAD_H_A)."""
    lp, maximize = DD.gradient_lps()[k]
    return (LD.Call("differences %d" % k, DD.gradient_batch(lp, DD.GRAD_H, (0, 2, 4)), maximize=maximize, precision=DD.GRAD_PRECISION),
            LD.Call("differences %d A" % k, DD.gradient_batch(lp, DD.GRAD_H_A, (1, 3)), maximize=maximize, precision=DD.GRAD_PRECISION_A))


# ------------------------------------------------------------------------------------------------ the children

def run_call(torch, handle, call, want=MARGINALS):
    """One Call through LpDense.solve with kept tableaux, all outputs pre-filled with SENTINEL, the new pointers of `want` passed."""
    B, n = len(call.lps), call.n
    ops, operands = LD._device_operands(torch, call)
    full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    x, objective = full((B, n), torch.float64), full((B,), torch.float64)
    status, pivots = full((B,), torch.int32), full((B,), torch.int64)
    marg = dict(ineqlin=full((B, call.m_ub), torch.float64), eqlin=full((B, call.m_eq), torch.float64), reduced=full((B, n), torch.float64))
    ptr = lambda t: t.data_ptr() if t.numel() else None
    handle.solve(B, n, call.m_ub, call.m_eq, operands, maximize=call.maximize, precision=call.precision, max_pivots=call.max_pivots,
                 check_cycles=call.check, keep_tableaux=True, x=ptr(x), objective=ptr(objective), status=ptr(status), pivots=ptr(pivots),
                 **{k: ptr(marg[k]) for k in want})
    sols = [handle.solution(i) for i in range(B)]
    info = handle.info()
    out = dict(x=x.cpu().numpy(), objective=objective.cpu().numpy(), status=status.cpu().numpy(), pivots=pivots.cpu().numpy(),
               col0=np.stack([s[0] for s in sols]), pos=np.stack([s[1] for s in sols]), var=np.stack([s[2] for s in sols]),
               tableau=np.stack([handle.tableau(i) for i in range(B)]), launches=np.int64(info["launches"]),
               kernels=np.array(" ".join(k["kernel"] for k in info["kernels"])), grids=np.array([k["grid"] for k in info["kernels"]], np.int64))
    out.update({k: t.cpu().numpy() for k, t in marg.items()})
    return out


def answer(out):
    """A LinprogDuals as numpy arrays."""
    return {k: t.detach().cpu().numpy() for k, t in zip(("x", "objective", "status", "pivots") + MARGINALS, out)}


def plumbing(torch, out):
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    from yalps_amd.sensitivity import sensitivity_many
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def put(tag, d):
        out.update({"%s/%s" % (tag, k): v for k, v in d.items()})

    # duals=True next to duals=False: the four old outputs are the same bits
    call = partial_call()
    ops = [dev(a) for a in call.stacked()]
    put("flag off", LD.answer(tensors.linprog_batch(*ops)))
    put("flag on", answer(tensors.linprog_batch(*ops, duals=True)))

    # views: LD.plumbing's two constructions, with duals
    inp = LD.strided_inputs()
    B, n = inp["c"].shape
    c_wide, b_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda"), torch.full((B, 8), -9.0, dtype=torch.float64, device="cuda")
    c_wide[:, ::2], b_wide[:, ::2] = dev(inp["c"]), dev(inp["b_ub"])
    A_ub_t, A_eq_t = dev(inp["A_ub"].T), dev(inp["A_eq"].transpose(0, 2, 1))
    views = (c_wide[:, ::2], A_ub_t.t(), b_wide[:, ::2], A_eq_t.transpose(1, 2), dev(inp["b_eq"]))
    assert not views[0].is_contiguous() and views[1].stride() == (1, 4) and views[4].dim() == 1
    put("views", answer(tensors.linprog_batch(*views, duals=True)))
    put("contiguous", answer(tensors.linprog_batch(*[dev(a) for a in LD.strided_call(inp).stacked()], duals=True)))
    inp = LD.offset_inputs()
    B, m, n = inp["A_ub"].shape
    A_wide = torch.full((B, m + 1, n + 2), -9.0, dtype=torch.float64, device="cuda")
    A_wide[:, 1:, 2:] = dev(inp["A_ub"])
    views = (dev(inp["c"]).expand(B, n), A_wide[:, 1:, 2:], dev(inp["b_ub"]).expand(B, m))
    assert views[0].stride() == (0, 1) and views[1].storage_offset() == (n + 2) + 2
    put("offset views", answer(tensors.linprog_batch(*views, maximize=True, duals=True)))
    put("offset contiguous", answer(tensors.linprog_batch(*[dev(a) for a in LD.offset_call(inp).stacked()[:3]], maximize=True, duals=True)))

    # the producer of A_ub on a side stream, directly before the call on that stream
    inp = LD.stream_inputs()
    side = torch.cuda.Stream()
    half, c, b = dev(inp["A_half"]), dev(inp["c"]), dev(inp["b_ub"])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big @ big * 2.0 ** -11  # (work in front of the producer: every entry stays 1.0)
        A = half * 2.0 + big[:6, :7] - 1.0
        put("stream", answer(tensors.linprog_batch(c, A, b, maximize=True, duals=True)))
    out["stream/A"] = A.cpu().numpy()
    del side

    # B = 0, and sides without rows
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    empty = tensors.linprog_batch(z(0, 3), z(0, 2, 3), z(0, 2), z(0, 1, 3), z(0, 1), duals=True)
    out["empty/shapes"] = np.array([d for t in empty for d in t.shape], np.int64)
    none = tensors.linprog_batch(torch.ones(2, 3, dtype=torch.float64, device="cuda"), duals=True)
    out["no rows/shapes"] = np.array([d for t in none[4:] for d in t.shape], np.int64)
    out["no rows/types"] = np.array(" ".join("%s %s %s" % (type(t).__name__, t.dtype, t.device.type) for t in none[4:]))
    put("no rows", answer(none))

    # a host pointer for a new output: refused by name, nothing launched, nothing written
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    call = LD.random_call("refusal", 3, 2, 2, 1)
    ops, operands = LD._device_operands(torch, call)
    good = {k: torch.full((3, s), SENTINEL, dtype=torch.float64, device="cuda") for k, s in zip(MARGINALS, (2, 1, 2))}
    host = np.zeros((3, 2))
    messages = []
    for name in MARGINALS:
        try:
            handle.solve(3, 2, 2, 1, operands, **{k: (host.ctypes.data if k == name else t.data_ptr()) for k, t in good.items()})
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    out["refusal/messages"] = np.array(messages)
    out["refusal/untouched"] = np.bool_(all(bool((t == SENTINEL).all().item()) for t in good.values()) and not host.any())
    put("refusal/after", run_call(torch, handle, call))
    handle.close()

    # sensitivity_many on the equivalent models
    for call in (LD.public_calls()[0], LD.public_calls()[2]):
        put("public " + call.name, answer(tensors.linprog_batch(*[None if a is None else dev(a) for a in call.stacked()], maximize=call.maximize, duals=True)))
        sols = sensitivity_many([ND.equivalent_model(*lp, maximize=call.maximize) for lp in call.lps])
        out["public %s/sens_status" % call.name] = np.array([LD.STATUS.index(s["status"]) for s in sols], np.int32)
        nan = [np.full(k, np.nan) for k in (call.m_ub, call.m_eq, call.n)]
        rows = [DD.model_marginals(s, call.n, call.m_ub, call.m_eq) if s["status"] == "optimal" else nan for s in sols]
        for j, key in enumerate(MARGINALS):
            out["public %s/sens_%s" % (call.name, key)] = np.stack([r[j] for r in rows])


def objective_runs(torch, out):
    """linprog_objective: every operand batched and requiring grad, one row infeasible; all operands but b_ub shared; and the
    batches whose objectives give the central differences."""
    from yalps_amd import tensors
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_()

    def run(tag, ops, weights, **options):
        objective, duals = tensors.linprog_objective(*ops, **options)
        assert objective.grad_fn is not None and not any(t.requires_grad for t in duals)
        assert torch.equal(objective.detach().nan_to_num(7.0), duals.objective.nan_to_num(7.0))
        objective.backward(torch.tensor(weights, dtype=torch.float64, device="cuda"))
        out.update({"%s/%s" % (tag, k): v for k, v in answer(duals).items()})
        for name, t in zip(("c", "A_ub", "b_ub", "A_eq", "b_eq"), ops):
            out["%s/grad_%s" % (tag, name)] = t.grad.cpu().numpy()

    call = gradient_call()
    run("gradient rows", [leaf(a) for a in call.stacked()], GRADIENT_WEIGHTS, precision=call.precision)
    call = shared_call()
    lp = call.lps[0]
    run("shared", [leaf(lp[0]), leaf(lp[1]), leaf(call.stacked()[2]), leaf(lp[3]), leaf(lp[4])], (1.0, 2.0, -3.0), precision=call.precision)
    for k, (lp, maximize) in enumerate(DD.gradient_lps()):
        run("base %d" % k, [leaf(a) for a in lp], (1.0,), maximize=maximize, precision=DD.GRAD_PRECISION_A)
        for call in difference_calls(k):
            got = tensors.linprog_batch(*[torch.from_numpy(a).cuda() for a in call.stacked()], maximize=maximize, precision=call.precision)
            out.update({"%s/%s" % (call.name, k2): v for k2, v in LD.answer(got).items()})
    no_grad = tensors.linprog_objective(*[torch.from_numpy(a).cuda() for a in DD.gradient_lps()[0][0]])[0]
    out["no grad/grad_fn"] = np.bool_(no_grad.grad_fn is not None or no_grad.requires_grad)


def child_table(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import _native as nat
    out = {}
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in table(_oracle.load()):
            out.update({"%s/%s" % (call.name, k): v for k, v in run_call(torch, handle, call).items()})
        for want in PARTIAL:
            out.update({"partial %s/%s" % ("+".join(want) or "none", k): v for k, v in run_call(torch, handle, partial_call(), want).items()})
    finally:
        handle.close()
    plumbing(torch, out)
    objective_runs(torch, out)
    np.savez(path, **out)


def child_hist(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import os
    assert os.environ.get("YALPS_LPDENSE_HIST") == str(LD.HIST)
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import tensors
    call = LD.hist_call(_oracle.load())
    stats = {}
    ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
    out = answer(tensors.linprog_batch(*ops, maximize=call.maximize, check_cycles=True, stats=stats, duals=True))
    out.update(reruns=np.int64(stats["reruns"]), passes=np.int64(1 + max(k["pass"] for k in stats["kernels"])))
    np.savez(path, **out)


if __name__ == "__main__":
    {"table": child_table, "hist": child_hist}[sys.argv[1]](sys.argv[2])
