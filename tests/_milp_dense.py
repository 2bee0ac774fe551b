"""Helpers of tests/test_milp_dense_model.py and tests/test_milp_dense.py (TEST INFRASTRUCTURE): the table of dense MILP calls,
and the child processes that run them on the GPU.

torch brings a HIP runtime along, and a pointer or a stream is only good in the runtime that made it, so torch has to be
loaded before any of the package's libraries (tests/_lp_dense.py says more).  Each child imports torch first, runs its calls
and writes everything they left behind to one .npz; the tests compare those files with the oracle-driven search of
tests/_np_milp_dense.py.

  table()         [Call]: every call of the child "table" -- through _native.MilpDense with a trace, so that the tree's status,
                  result, best tableau and node sequence can be compared besides the six output tensors
  child "table"   the table, then the plumbing calls through milp_batch (views, a side stream, B = 0, refusals), the equality
                  with linprog_batch, and _native.MilpTree on the same MILPs pre-packed
  child "mix"     mix_call() through milp_batch under the environment the test sets: YALPS_MILPDENSE_GRID=1 (one workgroup
                  walks all trees), _ARENA=2 (reruns, of some trees only), _ARENA=2 with _ARENA_MAX=2 (overflows, answered by
                  the host fallback)
  child "hist"    hist_call() under YALPS_MILPDENSE_HIST=4: the history rerun of root LPs and of nodes
"""
import json
import math
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _np_milp_dense as NM

INF = math.inf
QUEUE_MILPS = 2100            # more than class 0's grid of 8 x 256 workgroups
TRACE_CAP = 24                # nodes of a tree the table's calls record
HIST = 4
f = lambda *v: np.array(v, np.float64)


def packing_call(name, specs, **options):
    """specs: (m, n, n_int, seed) of MILPs of one shape; they share the first one's integer variables."""
    made = [NM.packing_dense(*s) for s in specs]
    return NM.Call(name, [lp for lp, _ in made], integers=made[0][1], maximize=True, **options)


def model_call(name, model, **options):
    lp, ints = NM.of_model(model)
    return NM.Call(name, [lp], integers=ints, maximize=True, **options)


def knapsacks(B, n, seed):
    """B 0/1 knapsacks over n binary variables: weights 2 .. 9, values close to the weights, capacity a third of the total."""
    rng = np.random.default_rng([20261020, B, n, seed])
    out = []
    for _ in range(B):
        wgt = rng.integers(2, 10, n).astype(np.float64)
        out.append((wgt + rng.integers(0, 3, n), wgt.reshape(1, n), np.array([np.floor(wgt.sum() / 3.0) + 0.5]), None, None))
    return out


def mostly_continuous(n, seed):
    """maximize over n variables of which only the LAST is integer: two knapsack rows, the last variable's value fractional."""
    rng = np.random.default_rng([20261020, n, seed])
    c = rng.integers(1, 6, n).astype(np.float64)
    c[-1] = 50.0
    A = rng.integers(1, 5, (2, n)).astype(np.float64)
    A[:, -1] = (2.0, 3.0)
    return c, A, f(7.0, 11.5), None, None


def queue_lps():
    rng = np.random.default_rng(20261024)
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    return [(ints(1, 9, 3), ints(0, 5, 2, 3), ints(1, 9, 2) + 0.5, None, None) for _ in range(QUEUE_MILPS)]


def both_ways():
    """One MILP that is bounded in both directions: 1.5 <= x0 + x1 + x2 <= 4.5, 2 x0 - x1 <= 2.5."""
    return f(3.0, 2.0, 4.0), np.array([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [2.0, -1.0, 0.0]]), f(4.5, -1.5, 2.5), None, None


def mix_call():
    """Eight MILPs of one shape whose trees differ: packing trees of a few to a few dozen nodes, one whose root is integral (no
    tree pass work, nothing to rerun) and one whose root is infeasible."""
    made = [NM.packing_dense(8, 8, 6, seed) for seed in (1, 2, 3, 4, 5, 6)]
    lps = [lp for lp, _ in made]
    c, A, b = lps[0][:3]
    lps.append((c, np.eye(8), np.arange(1.0, 9.0), None, None))      # integral root
    lps.append((c, A, np.concatenate([[-1.0], b[1:]]), None, None))  # 0 <= A[0] x <= -1: infeasible
    return NM.Call("mix", lps, integers=made[0][1], maximize=True)


def hist_call():
    """Trees whose root LPs, and a node of each, take more pivots than a history of HIST holds; checkCycles on."""
    return packing_call("hist", [(12, 12, 6, s) for s in (1, 2, 3)], check=True)


def nonfinite_call():
    """A NaN in b_ub of some rows and an infinity in c: the reference as the CPU search gives it."""
    made = [NM.packing_dense(6, 6, 4, seed) for seed in (1, 2, 3, 4)]
    lps = []
    for k, (lp, _) in enumerate(made):
        c, A, b = lp[0].copy(), lp[1].copy(), lp[2].copy()
        if k % 2 == 0:
            b[k] = math.nan
        if k >= 2:
            c[1] = math.inf
        lps.append((c, A, b, None, None))
    return NM.Call("nonfinite", lps, integers=made[0][1], maximize=True, max_iterations=40.0)


def names():
    out = ["n=1", "n=2", "binaries all n=65", "binaries only", "both sets, one variable in both", "one integer n=257",
           "one integer n=1025", "equalities and binaries", "no integers"]
    out += ["under bound %d" % k for k in range(4)] + ["over bound 2", "over bound 3", "under bound 2 check", "HBM odd n",
                                                         "HBM odd n check", "aux form", "packing check"]
    out += ["root infeasible", "root unbounded at the last variable", "root cycled", "root integral", "several nodes",
            "no integer point", "timedout with a solution", "timedout without a solution", "tolerance", "maximize", "minimize"]
    out += ["nonfinite", "queue"]
    return out


def table():
    P = packing_call
    T = [NM.Call("n=1", [(f(1.0), f(2.0).reshape(1, 1), f(b), None, None) for b in (3.0, 4.0, 0.5, 7.0)], integers=[0], maximize=True),
         NM.Call("n=2", [(f(3.0, 2.0), np.array([[2.0, 2.0], [1.0, 3.0]]), f(b0, b1), None, None) for b0, b1 in ((3.0, 4.5), (7.0, 2.5), (5.0, 5.0))],
                 integers=[1, 0], maximize=True),
         NM.Call("binaries all n=65", knapsacks(2, 65, 1), binaries=True, maximize=True, max_iterations=60.0),
         NM.Call("binaries only", knapsacks(3, 7, 2), binaries=[6, 5, 4, 3, 2, 1, 0], maximize=True),
         NM.Call("both sets, one variable in both", knapsacks(3, 7, 3), integers=[1, 3, 5], binaries=[3, 6, 0, 2, 4], maximize=True),
         NM.Call("one integer n=257", [mostly_continuous(257, s) for s in (1, 2)], integers=[256], maximize=True),
         NM.Call("one integer n=1025", [mostly_continuous(1025, s) for s in (1, 2)], integers=[1024], maximize=True),
         NM.Call("equalities and binaries", [(f(2.0, 3.0, 1.0, 4.0), np.array([[1.0, 2.0, 1.0, 3.0]]), f(b), np.array([[1.0, 1.0, 1.0, 1.0]]), f(2.0))
                                             for b in (3.5, 4.5, 2.0)], integers=[2], binaries=[0, 1, 3], maximize=True),
         NM.Call("no integers", [NM.packing_dense(8, 8, 6, s)[0] for s in (1, 2, 3)], maximize=True)]
    for k in range(4):
        T.append(model_call("under bound %d" % k, BS.bound_model(k), max_iterations=12.0))
    for k in (2, 3):
        w = BS.BOUND_WIDTHS[k]
        T.append(model_call("over bound %d" % k, BS.packing(BS.rows_under(LB.BOUNDS[k], w), w - 1, 8, 2, 0.6), max_iterations=8.0))
    T.append(model_call("under bound 2 check", BS.bound_model(2), max_iterations=8.0, check=True))
    odd = BS.packing(150, 151, 8, 7, 0.3)
    T += [model_call("HBM odd n", odd, max_iterations=8.0), model_call("HBM odd n check", odd, max_iterations=6.0, check=True),
          model_call("aux form", BS.packing(8160, 30, 6, 1, 0.3), max_iterations=6.0),
          P("packing check", [(8, 8, 6, s) for s in (1, 2, 3)], check=True)]
    T += [NM.Call("root infeasible", [(f(1.0, 1.0), np.array([[1.0, 1.0]]), f(-1.0), None, None)], integers=[0], maximize=True),
          NM.Call("root unbounded at the last variable", [(f(0.0, 0.0, 1.0), np.array([[1.0, 1.0, 0.0]]), f(1.5), None, None)], integers=[0, 2],
                  maximize=True),
          P("root cycled", [(8, 8, 6, 1), (8, 8, 6, 2)], max_pivots=2.0),
          NM.Call("root integral", [(f(1.0, 1.0), np.eye(2), f(2.0, 3.0), None, None)], integers=True, maximize=True),
          P("several nodes", [(8, 8, 6, s) for s in (1, 2, 3, 4)]),
          NM.Call("no integer point", [(f(1.0, 1.0), None, None, np.array([[2.0, 0.0]]), f(1.0))], integers=[0], maximize=False),
          P("timedout with a solution", [(10, 10, 8, s) for s in (1, 2, 3)], max_iterations=6.0),
          P("timedout without a solution", [(10, 10, 8, s) for s in (1, 2, 3)], max_iterations=1.0),
          P("tolerance", [(10, 10, 8, s) for s in (1, 2, 3)], tolerance=0.2),
          NM.Call("maximize", [both_ways()], integers=True, maximize=True), NM.Call("minimize", [both_ways()], integers=True, maximize=False)]
    T += [nonfinite_call(), NM.Call("queue", queue_lps(), integers=True, maximize=True)]
    assert [c.name for c in T] == names()
    return T


# ------------------------------------------------------------------------------------------------ the children

def _device_operands(torch, call):
    from yalps_amd import tensors
    ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
    return ops, tuple(tensors._strides(t, True, k in (1, 3)) for k, t in enumerate(ops))


def run_call(torch, handle, call, trace_cap=TRACE_CAP):
    """One Call through MilpDense.solve: the six sentinel-filled output tensors, every tree's status, result and best tableau,
    its trace, and the launches."""
    B, n = len(call.lps), call.n
    ops, operands = _device_operands(torch, call)
    full = lambda shape, dtype: torch.full(shape, -7, dtype=dtype, device="cuda")
    x, objective, status = full((B, n), torch.float64), full((B,), torch.float64), full((B,), torch.int32)
    nodes, node_pivots, root_pivots = (full((B,), torch.int64) for _ in range(3))
    ptr = lambda t: t.data_ptr() if t.numel() else None
    stats = handle.solve(B, n, call.m_ub, call.m_eq, operands, integers=call.ints, binaries=call.bins, maximize=call.maximize,
                         precision=call.precision, max_pivots=call.max_pivots, check_cycles=call.check, tolerance=call.tolerance,
                         max_iterations=call.max_iterations, trace_cap=trace_cap, x=ptr(x), objective=ptr(objective), status=ptr(status),
                         nodes=ptr(nodes), node_pivots=ptr(node_pivots), root_pivots=ptr(root_pivots))
    keep = min(B, 16)  # (the queue call: the first trees' tableaux and traces stand for all; the tensors are compared whole)
    sols = [handle.solution(i) for i in range(keep)]
    pad = lambda a, size: np.concatenate([a, np.zeros(size - a.size, a.dtype)])
    traces = [[(LB_hex(t["eval"]), [(s, v, LB_hex(c)) for s, v, c in t["cuts"]], t["status"], LB_hex(t["result"]), t["n_pivots"], t["height"])
               for t in handle.trace(i)] for i in range(keep)]
    info = handle.info()
    after = [None if t is None else t.cpu().numpy() for t in ops]
    unchanged = all(a is None or a.tobytes() == b.tobytes() for a, b in zip(after, call.stacked()))
    return dict(x=x.cpu().numpy(), objective=objective.cpu().numpy(), status=status.cpu().numpy(), nodes=nodes.cpu().numpy(),
                node_pivots=node_pivots.cpu().numpy(), root_pivots=root_pivots.cpu().numpy(),
                tree_status=np.array([NM.STATUS.index(s[0]) for s in sols], np.int32), tree_result=np.array([s[1] for s in sols], np.float64),
                height=np.array([s[2] for s in sols], np.int32), col0=np.stack([pad(s[3], call.hmax) for s in sols]),
                pos=np.stack([pad(s[4], call.w + call.hmax) for s in sols]), var=np.stack([pad(s[5], call.w + call.hmax) for s in sols]),
                traces=np.array(json.dumps(traces)), launches=np.int64(info["launches"]), reruns=np.int64(info["reruns"]),
                overflows=np.int64(stats["overflows"]), kernels=np.array(" ".join(k["kernel"] for k in info["kernels"])),
                classes=np.array([k["class"] for k in info["kernels"]], np.int64), grids=np.array([k["grid"] for k in info["kernels"]], np.int64),
                unchanged=np.bool_(unchanged))


def LB_hex(x):
    from tests import _bnc
    return "nan" if math.isnan(x) else _bnc.hexd(x)


def answer(out):
    """A MilpBatchResult as numpy arrays."""
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


def view_inputs():
    """The MILPs of the views test: B = 5, n = 6, m_ub = 3, m_eq = 1; A_ub shared by the batch, b_eq shared."""
    rng = np.random.default_rng(20261025)
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    return dict(c=ints(1, 9, 5, 6), A_ub=ints(0, 5, 3, 6), b_ub=ints(3, 12, 5, 3) + 0.5, A_eq=ints(0, 2, 5, 1, 6), b_eq=f(2.0))


def view_call(inp):
    B = inp["c"].shape[0]
    return NM.Call("views", [(inp["c"][i], inp["A_ub"], inp["b_ub"][i], inp["A_eq"][i], inp["b_eq"]) for i in range(B)],
                   integers=[0, 2, 4], binaries=[4, 5], maximize=True)


def stream_inputs():
    rng = np.random.default_rng(20261026)
    return dict(c=rng.integers(1, 9, (4, 5)).astype(np.float64), A_half=rng.integers(0, 4, (4, 3, 5)).astype(np.float64),
                b_ub=rng.integers(3, 9, (4, 3)).astype(np.float64) + 0.5)


def plumbing(torch, out):
    """The calls through milp_batch; what each left behind goes into `out` under "<test>/<key>"."""
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    dev = lambda a: torch.from_numpy(a).cuda()

    def put(tag, d):
        out.update({"%s/%s" % (tag, k): v for k, v in d.items()})

    # views: A_ub shared and transposed, A_eq batched and transposed, c every other element of a wider tensor, b_ub behind a
    # storage offset inside a wider tensor, b_eq shared
    inp = view_inputs()
    call = view_call(inp)
    B, n = inp["c"].shape
    c_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda")
    b_wide = torch.full((B + 1, 5), -9.0, dtype=torch.float64, device="cuda")
    c_wide[:, ::2], b_wide[1:, 2:] = dev(inp["c"]), dev(inp["b_ub"])
    A_ub_t = dev(np.ascontiguousarray(inp["A_ub"].T))
    A_eq_t = dev(np.ascontiguousarray(inp["A_eq"].transpose(0, 2, 1)))
    b_eq = dev(inp["b_eq"])
    held = [c_wide, b_wide, A_ub_t, A_eq_t, b_eq]
    before = [t.cpu().numpy().copy() for t in held]
    views = (c_wide[:, ::2], A_ub_t.t(), b_wide[1:, 2:], A_eq_t.transpose(1, 2), b_eq)
    assert not views[0].is_contiguous() and not views[1].is_contiguous() and views[2].storage_offset() == 7
    kw = dict(integers=call.integers, binaries=call.binaries, maximize=True)
    put("views", answer(tensors.milp_batch(*views, **kw)))
    out["views/unchanged"] = np.bool_(all(a.tobytes() == t.cpu().numpy().tobytes() for a, t in zip(before, held)))
    put("contiguous", answer(tensors.milp_batch(*[dev(a) for a in call.stacked()], **kw)))

    # the producer of A_ub on a side stream, directly before the call on that stream
    inp = stream_inputs()
    side = torch.cuda.Stream()
    half, c, b = dev(inp["A_half"]), dev(inp["c"]), dev(inp["b_ub"])
    torch.cuda.synchronize()
    stats = {}
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big @ big * 2.0 ** -11  # (work in front of the producer: every entry stays 1.0)
        A = half * 2.0 + big[:3, :5] - 1.0
        first = tensors.milp_batch(c, A, b, integers=True, maximize=True, stats=stats)
    put("stream", answer(first))
    out["stream/A"] = A.cpu().numpy()
    out["stream/handles"] = np.int64(len(tensors._milp_handles))
    out["stream/kernels"] = np.array(" ".join(k["kernel"] for k in stats["kernels"]))
    del side

    # B = 0
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    stats = {}
    empty = tensors.milp_batch(z(0, 3), z(0, 2, 3), z(0, 2), integers=[1], stats=stats)
    out["empty/shapes"] = np.array([d for t in empty for d in t.shape], np.int64)
    out["empty/dtypes"] = np.array(" ".join(str(t.dtype) for t in empty))
    out["empty/launches"] = np.int64(stats["launches"])

    # no integer variable: linprog_batch's answer
    call = table_call("no integers")
    ops = [None if a is None else dev(a) for a in call.stacked()]
    put("no integers/milp", answer(tensors.milp_batch(*ops, maximize=True)))
    lp = tensors.linprog_batch(*ops, maximize=True)
    put("no integers/lp", dict(x=lp.x.cpu().numpy(), objective=lp.objective.cpu().numpy(), status=lp.status.cpu().numpy(), pivots=lp.pivots.cpu().numpy()))

    # refusals: a host pointer for an operand and for an output; nothing is launched, and the handle still works afterwards
    handle = nat.MilpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    call = table_call("n=2")
    ops, operands = _device_operands(torch, call)
    B = len(call.lps)
    x = torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda")
    host = np.zeros((B, 2))
    pinned = torch.zeros((B, 2), dtype=torch.float64).pin_memory()
    messages = []
    for name, p in (("c", host.ctypes.data), ("b_ub", pinned.data_ptr()), ("x_out", host.ctypes.data), ("nodes_out", host.ctypes.data)):
        bad, outs = list(operands), dict(x=x.data_ptr())
        if name == "c":
            bad[0] = (p, 2, 1, 0)
        elif name == "b_ub":
            bad[2] = (p, 2, 1, 0)
        elif name == "x_out":
            outs["x"] = p
        else:
            outs["nodes"] = p
        try:
            handle.solve(B, 2, 2, 0, bad, integers=[0, 1], **outs)
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    out["refusal/messages"] = np.array(messages)
    out["refusal/x_untouched"] = np.bool_(bool((x == -7.0).all().item()))
    put("refusal/after", run_call(torch, handle, call))
    handle.close()

    # the same MILPs pre-packed through MilpTree
    from yalps_amd import milp_dense
    tree = nat.MilpTree(0)
    for name in ("several nodes", "under bound 2", "tolerance"):
        call = table_call(name)
        milps = [milp_dense.packed_milp(lp, call.ints, call.bins, call.maximize, dict(call.options, timeout=INF)) for lp in call.lps]
        statuses, results, used, pivots, _ = tree.solve(milps)
        sols = [tree.solution(i) for i in range(len(milps))]
        pad = lambda a, size: np.concatenate([a, np.zeros(size - a.size, a.dtype)])
        put("tree/" + name, dict(status=np.array([NM.STATUS.index(s) for s in statuses], np.int32), result=np.asarray(results), nodes=np.asarray(used),
                                 node_pivots=np.asarray(pivots), height=np.array([s[0] for s in sols], np.int32),
                                 col0=np.stack([pad(s[1], call.hmax) for s in sols]), pos=np.stack([pad(s[2], call.w + call.hmax) for s in sols]),
                                 var=np.stack([pad(s[3], call.w + call.hmax) for s in sols])))
    tree.close()


_TABLE = {}


def table_call(name):
    if not _TABLE:
        _TABLE.update({c.name: c for c in table()})
    return _TABLE[name]


def _torch_first():
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    return torch


def child_table(path):
    torch = _torch_first()
    from yalps_amd import _native as nat
    out = {}
    handle = nat.MilpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in table():
            out.update({"%s/%s" % (call.name, k): v for k, v in run_call(torch, handle, call).items()})
    finally:
        handle.close()
    plumbing(torch, out)
    np.savez(path, **out)


def _public(torch, call, path):
    from yalps_amd import tensors
    stats = {}
    ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
    got = tensors.milp_batch(*ops, integers=call.integers, binaries=call.binaries, maximize=call.maximize, precision=call.precision,
                             max_pivots=call.max_pivots, check_cycles=call.check, tolerance=call.tolerance, max_iterations=call.max_iterations,
                             stats=stats)
    out = answer(got)
    out.update(reruns=np.int64(stats["reruns"]), launches=np.int64(stats["launches"]), overflows=np.int64(stats["overflows"]),
               passes=np.int64(1 + max(k["pass"] for k in stats["kernels"])), grids=np.array([k["grid"] for k in stats["kernels"]], np.int64),
               kernels=np.array(" ".join(k["kernel"] for k in stats["kernels"])),
               rerun_trees=np.array(tensors._milp_handles[next(iter(tensors._milp_handles))].info()["rerun_trees"], np.int64))
    np.savez(path, **out)


def child_mix(path):
    _public(_torch_first(), mix_call(), path)


def child_hist(path):
    import os
    assert os.environ.get("YALPS_MILPDENSE_HIST") == str(HIST)
    _public(_torch_first(), hist_call(), path)


if __name__ == "__main__":
    {"table": child_table, "mix": child_mix, "hist": child_hist}[sys.argv[1]](sys.argv[2])
