"""Helpers of tests/test_milp_dense_bounds_model.py and tests/test_milp_dense_bounds.py (TEST INFRASTRUCTURE): the table of
bounded dense MILP calls -- milp_batch(lb=, ub=, upper=) -- and the child processes that run them on the GPU (tests/_milp_dense.py
says why children: torch first).  Each child writes everything its calls left behind to one .npz; the tests compare those files
with tests/_np_milp_dense_bounds.py: the oracle-driven search on the bounded tableau, moved back.

  table()         [BCall]: every call of the child "table", through _native.MilpDense with a trace
  child "table"   the table, then the plumbing through milp_batch and the equalities with the other calls
  child "mix"     mix_call() through milp_batch under the environment the test sets (YALPS_MILPDENSE_GRID / _ARENA / _ARENA_MAX)
  child "hist"    hist_call() under YALPS_MILPDENSE_HIST=4
"""
import math
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _milp_dense as MD
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB

INF, NAN = math.inf, math.nan
QUEUE_MILPS = 2100            # more than class 0's grid of 8 x 256 workgroups
TRACE_CAP = MD.TRACE_CAP
HIST = MD.HIST
f = MD.f


def bounded_milp(rng, n, m_ub, m_eq, ints, bins, mode="both", grain=0.25, slack=1.0, heavy=()):
    """One MILP around a point x0 of its box that is integral where it has to be, so most are feasible.  grain: lb, the widths
    and the coefficients are multiples of it (lb is fractional at integer variables too: rule 1 rounds it up); None: data whose
    rounding shows -- lb ~ N(0, 1), coefficients uniform, no product a[j] * lb[j] exact.  The first A_ub row is positive: with
    x >= lb it bounds every variable.  Maximised objectives are positive.  heavy: columns whose coefficients are 16 times the
    others', so that the lanes that hold them decide the last bits of every shift_sum."""
    ints, bins = sorted(set(ints) | set(bins)), sorted(bins)
    if grain is None:
        lb, width = rng.standard_normal(n), 1.25 + 3.0 * rng.random(n)
        A_ub, A_eq = rng.random((m_ub, n)) * 6.0 - 2.0, rng.random((m_eq, n)) * 6.0 - 2.0
        if m_ub:
            A_ub[0] = 0.5 + rng.random(n)
        c = (0.5 + rng.random(n)) * (1.0 + rng.standard_normal(n) / 8.0)
        for j in heavy:
            A_ub[:, j], A_eq[:, j], c[j] = A_ub[:, j] * 16.0, A_eq[:, j] * 16.0, c[j] * 16.0
    else:
        q = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
        lb, width = q(-6, 7, n) * grain, 1.5 + q(0, 9, n) * grain
        A_ub, A_eq = q(-1, 5, m_ub, n), q(-1, 4, m_eq, n)
        if m_ub:
            A_ub[0] = q(1, 4, n)
        c = q(1, 9, n)
    if mode == "ub":
        lb = np.zeros(n)
    low = NB.effective_lower(lb, n, ints, bins)
    ub = low + width if mode != "ub" else width
    x0 = low + width * rng.random(n)
    for j in ints:
        x0[j] = low[j] + float(rng.integers(0, 2))
    for j in bins:
        x0[j] = float(rng.integers(0, 2))
    b_ub = A_ub @ x0 + slack * (rng.random(m_ub) if grain is None else np.ceil(rng.random(m_ub) * 4.0) * grain)
    return (c, A_ub if m_ub else None, b_ub if m_ub else None, A_eq if m_eq else None, A_eq @ x0 if m_eq else None,
            lb if mode != "ub" else None, ub if mode != "lb" else None)


def call(name, B, n, m_ub, m_eq, ints=(), bins=(), mode="both", upper=True, grain=0.25, seed=0, slack=1.0, heavy=(), **options):
    rng = np.random.default_rng([20261301, n, m_ub, m_eq, seed])
    options.setdefault("maximize", True)
    if not options["maximize"]:
        raise AssertionError("the generator's objectives are bounded above only")
    out = NB.BCall(name, [bounded_milp(rng, n, m_ub, m_eq, ints, bins, mode, grain, slack, heavy) for _ in range(B)], upper, integers=list(ints),
                   binaries=list(bins), **options)
    out.exact = grain is not None  # (data in quarters: the search reaches its vertices without rounding that shows)
    return out


def minimised(c):
    """The same MILPs with -c, minimised: the other sign in row 0, the same vertices."""
    out = NB.BCall(c.name, [(-lp[0], *lp[1:], lb, ub) for lp, lb, ub in zip(c.lps, c.lbs, c.ubs)], c.upper, integers=c.integers,
                   binaries=c.binaries, maximize=False, precision=c.precision, max_pivots=c.max_pivots, check=c.check, tolerance=c.tolerance,
                   max_iterations=c.max_iterations)
    out.exact = c.exact
    return out


def class_call(name, w, h, k, n_int, seed=0, **options):
    """A root of h x w with k bound rows on the first k variables and n_int integer variables (the last ones), no binary, data
    whose rounding shows."""
    n = w - 1
    return call(name, 1, n, h - 1 - k, 0, ints=range(n - n_int, n), upper=tuple(range(k)), grain=None, seed=seed, **options)


def rule_calls():
    """The three rules on hand-made data."""
    A, b = np.array([[1.0, 1.0, 1.0, 1.0]]), f(7.25)
    c = f(3.0, 2.0, 4.0, 1.0)
    # fractional lb at integer variables: 0.5 -> 1.0, -0.5 -> -0.0, -1.5 -> -1.0; the last variable is continuous and keeps 0.25
    lb, ub = f(0.5, -0.5, -1.5, 0.25), f(2.5, 1.5, 0.75, 3.0)
    frac = NB.BCall("fractional lb at integers", [(c, A, f(b0), None, None, lb, ub) for b0 in (7.25, 3.5, 1.0)], integers=[0, 1, 2], maximize=True)
    # NaN poison at the binary columns of lb and ub: neither is read there
    lbp, ubp = f(NAN, 0.5, NAN, -0.75), f(NAN, 2.5, NAN, 1.5)
    poison = NB.BCall("NaN at binaries", [(c, A, f(b0), None, None, lbp, ubp) for b0 in (3.25, 1.5)], integers=[1], binaries=[0, 2], maximize=True)
    clean = NB.BCall("clean at binaries", [(c, A, f(b0), None, None, f(0.0, 0.5, 0.0, -0.75), f(1.0, 2.5, 1.0, 1.5)) for b0 in (3.25, 1.5)],
                     integers=[1], binaries=[0, 2], maximize=True)
    # as it lies: +inf in ub (that bound row never binds) and NaN in lb at a continuous variable (every right-hand side is NaN)
    lies = NB.BCall("inf in ub, NaN in lb", [(c, A, b, None, None, f(0.5, 0.0, 0.0, 0.25), f(2.0, INF, 2.0, INF)),
                                             (c, A, b, None, None, f(0.5, 0.0, 0.0, NAN), f(2.0, 3.0, 2.0, 3.0)),
                                             (c, A, b, None, None, f(0.5, 0.0, 0.0, -INF), f(2.0, 3.0, 2.0, 3.0))], integers=[0, 1], maximize=True,
                    max_iterations=40.0)
    return [frac, poison, lies], clean


def endings_calls():
    c, A = f(2.0, 3.0, 1.0), np.array([[1.0, 2.0, 1.0]])
    infeasible = NB.BCall("lb > ub", [(c, A, f(9.5), None, None, f(0.5, 1.0, 0.25), f(3.0, ub1, 2.0)) for ub1 in (0.5, 3.5, -1.0)], integers=[0, 1],
                          maximize=True)
    # variable 2 has no coefficient in A and is not listed: the LP is unbounded through it
    free = NB.BCall("unbounded through an unlisted variable", [(c, np.array([[1.0, 2.0, 0.0]]), f(6.5), None, None, f(0.5, -1.5, 0.25), f(3.0, 2.0, 1.0))],
                    upper=(0, 1), integers=[0, 1], maximize=True)
    return [infeasible, free]


def queue_call():
    """2100 MILPs of three variables, two of them integer, variable 2 unlisted: every ending in one call.  The budget of three
    nodes leaves some trees "timedout", with and without a solution; a box with lb > ub is infeasible; a third column without
    coefficients is unbounded; two pivots are not enough for some roots ("cycled")."""
    rng = np.random.default_rng(20261302)
    q = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    lps = []
    for i in range(QUEUE_MILPS):
        A = q(0, 5, 2, 3)
        A[0] = np.maximum(A[0], 1.0)
        lb = q(-4, 5, 3) * 0.25
        ub = lb + q(2, 12, 3) * 0.25
        if i % 9 == 0:
            ub[int(q(0, 2))] = lb[0] - 1.0
        if i % 7 == 0:
            A[:, 2] = 0.0
        lps.append((q(1, 9, 3), A, A @ (lb + 1.0) + q(1, 9, 2) + 0.5, None, None, lb, ub))
    return NB.BCall("queue", lps, upper=(0, 1), integers=[0, 1], maximize=True, max_iterations=3.0, max_pivots=3.0)


R2, R3 = BS.rows_under(LB.BOUNDS[2], 99), BS.rows_under(LB.BOUNDS[3], 137)
# name: (w, root height, bound rows, integer variables, the classes of the root without its bound rows, of the root, and of the
# largest node, the seed: the first whose tree consumes nodes)
SHAPES = {
    "256 to 1024 lanes by the bound rows": (99, R2 + 2, 4, 2, (2, 3, 3), 4),
    "256 to 1024 lanes by the cuts": (99, R2 - 1, 4, 2, (2, 2, 3), 1),
    "LDS to HBM by the bound rows": (137, R3 + 2, 4, 2, (3, 4, 4), 0),
    "LDS to HBM by the cuts": (137, R3 - 1, 4, 2, (3, 3, 4), 2),
    "HBM odd n": (152, 160, 8, 2, (4, 4, 4), 2),
    "aux form": (31, 8170, 30, 2, (4, 4, 4), 3),
}
LANES = (1, 2, 63, 64, 65, 129)


def names():
    out = ["n=%d" % n for n in LANES]
    out += ["k=0", "k=1", "bound rows and binary rows", "no operand rows", "equalities only", "lb only", "ub only", "minimize", "check"]
    for name in SHAPES:
        out += [name, name + " check"]
    out += ["fractional lb at integers", "NaN at binaries", "inf in ub, NaN in lb", "lb > ub", "unbounded through an unlisted variable",
            "timedout with a solution", "timedout without a solution", "hard n=65", "hard n=129", "queue"]
    return out


HARD = ("hard n=65", "hard n=129")  # non-integer lb at continuous variables, data whose rounding shows: the flaws' floors hold here


def table():
    T = [call("n=1", 3, 1, 1, 0, ints=[0]), call("n=2", 3, 2, 2, 0, ints=[1])]
    T += [call("n=%d" % n, 2, n, 3, 1, ints=[0, n - 1], bins=[1], grain=None, max_iterations=24.0) for n in LANES[2:]]
    T += [call("k=0", 3, 5, 3, 1, ints=[0, 3], upper=()), call("k=1", 3, 5, 3, 1, ints=[0, 3], upper=(3,)),
          call("bound rows and binary rows", 3, 6, 3, 1, ints=[0, 3], bins=[1, 4]),
          call("no operand rows", 3, 5, 0, 0, ints=[0, 2], bins=[4]), call("equalities only", 3, 6, 0, 2, ints=[1, 4], bins=[2]),
          call("lb only", 3, 5, 3, 1, ints=[0, 3], bins=[2], mode="lb", seed=1), call("ub only", 3, 5, 3, 1, ints=[0, 3], bins=[2], mode="ub", seed=2),
          minimised(call("minimize", 3, 5, 3, 1, ints=[0, 3], bins=[2], seed=3)), call("check", 3, 5, 3, 1, ints=[0, 3], bins=[2], check=True, seed=4)]
    for name, (w, h, k, n_int, classes, seed) in SHAPES.items():
        for check in (False, True):
            c = class_call(name + (" check" if check else ""), w, h, k, n_int, seed=seed, max_iterations=5.0, check=check, **({"max_pivots": INF} if w == 31 else {}))
            assert (LB.size_class(c.w, c.h - c.k), LB.size_class(c.w, c.h), LB.size_class(c.w, c.hmax)) == classes, (name, c.w, c.h, c.hmax)
            assert BS.aux_hbm(c.w, c.h) == (name == "aux form") and (name != "HBM odd n" or c.n % 2 == 1)
            T.append(c)
    T += rule_calls()[0] + endings_calls()
    T += [call("timedout with a solution", 3, 10, 10, 0, ints=range(8), max_iterations=6.0, seed=2),
          call("timedout without a solution", 3, 10, 10, 0, ints=range(8), max_iterations=1.0, seed=2)]
    # (n = 65: lane 0 alone holds two columns, 0 and 64, and the first fold adds lane 32 to it: those three columns are heavy, and
    # continuous, so that what lane 0 does shows in the last bits of a sum; the seeds: the first whose answers tell every flaw)
    T += [call("hard n=65", 8, 65, 9, 3, ints=[5, 40], bins=[7], grain=None, seed=1, heavy=(0, 32, 64), max_iterations=24.0),
          call("hard n=129", 8, 129, 9, 3, ints=[5, 100], bins=[70], grain=None, seed=8, max_iterations=24.0)]
    T.append(queue_call())
    assert [c.name for c in T] == names(), [c.name for c in T]
    return T


_TABLE = {}


def table_call(name):
    if not _TABLE:
        _TABLE.update({c.name: c for c in table()})
    return _TABLE[name]


def boxed(base, name, seed):
    """The MILPs of a boundless packing call (A >= 0, maximised) with a box on every variable: lb in sixteenths of 0 .. 3/16 at
    a continuous variable and in quarters of -1.75 .. 0 at an integer one (rule 1 makes -1.0, -0.0 or +0.0 of it), so that the
    shifted right-hand sides stay positive; ub three or more above lb."""
    rng = np.random.default_rng([20261303, seed])
    lps = []
    for lp in base.lps:
        lb = rng.integers(0, 4, base.n).astype(np.float64) / 16.0
        lb[base.ints] = rng.integers(-7, 1, len(base.ints)).astype(np.float64) * 0.25
        lps.append((*lp, lb, lb + 3.0 + rng.integers(0, 8, base.n) * 0.25))
    return NB.BCall(name, lps, integers=base.integers, binaries=base.binaries, maximize=base.maximize, check=base.check)


def mix_call():
    """MD.mix_call's eight MILPs, whose trees differ in size, with a box on every variable.  The last two keep what they were
    made for: a root that is integral (lb = -1 at the integer variables and 0 at the others moves the right-hand sides 1 .. 8 by
    whole numbers) and a root that is infeasible (a right-hand side far below zero): neither has a tree to run again."""
    mix = boxed(MD.mix_call(), "mix", 0)
    low = np.zeros(mix.n)
    low[mix.ints] = -1.0
    mix.lbs[6], mix.ubs[6] = low, low + 16.0
    c, A, b = mix.lps[7][:3]
    mix.lps[7] = (c, A, np.concatenate([[-100.0], b[1:]]), None, None)
    return mix


def hist_call():
    """MD.hist_call's MILPs (root LPs and nodes of more pivots than a history of HIST holds, checkCycles on) in a box."""
    return boxed(MD.hist_call(), "hist", 1)


def lp_call():
    """No integer and no binary variable: linprog_batch's problem."""
    return call("no integers", 4, 6, 4, 2, grain=None, seed=2)


def identity_call():
    """Integral lb >= 0, every variable integer, integer data: the caller's other route -- -x <= -lb and x <= ub as rows under A_ub
    -- is the same MILP with an integer optimal value."""
    rng = np.random.default_rng(20261304)
    q = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    lps = []
    for _ in range(4):
        A = q(0, 5, 3, 4)
        A[0] = np.maximum(A[0], 1.0)
        lb = q(0, 3, 4)
        lps.append((q(1, 9, 4), A, A @ (lb + 1.0) + q(0, 4, 3) + 0.5, None, None, lb, lb + q(1, 4, 4)))
    return NB.BCall("identity", lps, integers=True, maximize=True)


def identity_operands(c):
    """(c, A_ub, b_ub) with the identity blocks under A_ub: -x <= -lb, x <= ub."""
    n = c.n
    eye = np.eye(n)
    return [(lp[0], np.concatenate([lp[1], -eye, eye]), np.concatenate([lp[2], -lb, ub]), None, None) for lp, lb, ub in zip(c.lps, c.lbs, c.ubs)]


def view_call():
    """B = 5, n = 6: per-MILP bounds (given as views) -- and, as "shared", one lb / ub for the batch ([n] tensors, batch stride 0)."""
    per = call("views", 5, 6, 3, 1, ints=[0, 2, 4], bins=[4, 5], upper=(0, 2, 3), seed=3)
    shared = NB.BCall("shared", [(*lp, per.lbs[0], per.ubs[0]) for lp in per.lps], upper=(0, 2, 3), integers=per.integers, binaries=per.binaries,
                      maximize=True)
    return per, shared


def partial_call():
    return call("partial", 3, 5, 3, 1, ints=[0, 3], bins=[2], seed=4)


PARTIAL = ((), ("x",), ("objective", "nodes"), ("status", "node_pivots", "root_pivots"))


# ------------------------------------------------------------------------------------------------ the children

def _device(torch, call):
    from yalps_amd import tensors
    ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
    bnd = [None if a is None else torch.from_numpy(a).cuda() for a in call.bounds_stacked()]
    operands = tuple(tensors._strides(t, True, k in (1, 3)) for k, t in enumerate(ops))
    bounds = [None if t is None else (tensors._strides(t, True, False) or (None, 0, 0, 0)) for t in bnd]
    return ops, bnd, operands, bounds


OUTPUTS = ("x", "objective", "status", "nodes", "node_pivots", "root_pivots")


def run_call(torch, handle, call, trace_cap=TRACE_CAP, want=OUTPUTS):
    """One BCall through MilpDense.solve (yalps_milpdense_solve_bounds): the six sentinel-filled output tensors (the pointers of
    `want` passed), every tree's status, result and best tableau, its trace, and the launches."""
    B, n = len(call.lps), call.n
    ops, bnd, operands, bounds = _device(torch, call)
    full = lambda shape, dtype: torch.full(shape, -7, dtype=dtype, device="cuda")
    outs = dict(x=full((B, n), torch.float64), objective=full((B,), torch.float64), status=full((B,), torch.int32),
                nodes=full((B,), torch.int64), node_pivots=full((B,), torch.int64), root_pivots=full((B,), torch.int64))
    stats = handle.solve(B, n, call.m_ub, call.m_eq, operands, integers=call.ints, binaries=call.bins, maximize=call.maximize,
                         precision=call.precision, max_pivots=call.max_pivots, check_cycles=call.check, tolerance=call.tolerance,
                         max_iterations=call.max_iterations, trace_cap=trace_cap, lb=bounds[0], ub=bounds[1], upper=call.idx,
                         **{k: (outs[k].data_ptr() if outs[k].numel() else None) for k in want})
    keep = min(B, 16)  # (the queue call: the first trees' tableaux and traces stand for all; the tensors are compared whole)
    sols = [handle.solution(i) for i in range(keep)]
    pad = lambda a, size: np.concatenate([a, np.zeros(size - a.size, a.dtype)])
    traces = [[(MD.LB_hex(t["eval"]), [(s, v, MD.LB_hex(c)) for s, v, c in t["cuts"]], t["status"], MD.LB_hex(t["result"]), t["n_pivots"], t["height"])
               for t in handle.trace(i)] for i in range(keep)]
    info = handle.info()
    after = [None if t is None else t.cpu().numpy() for t in ops + bnd]
    unchanged = all(a is None or a.tobytes() == b.tobytes() for a, b in zip(after, call.stacked() + list(call.bounds_stacked())))
    import json
    out = {k: t.cpu().numpy() for k, t in outs.items()}
    out.update(tree_status=np.array([NM.STATUS.index(s[0]) for s in sols], np.int32), tree_result=np.array([s[1] for s in sols], np.float64),
               height=np.array([s[2] for s in sols], np.int32), col0=np.stack([pad(s[3], call.hmax) for s in sols]),
               pos=np.stack([pad(s[4], call.w + call.hmax) for s in sols]), var=np.stack([pad(s[5], call.w + call.hmax) for s in sols]),
               traces=np.array(json.dumps(traces)), launches=np.int64(info["launches"]), reruns=np.int64(info["reruns"]),
               overflows=np.int64(stats["overflows"]), kernels=np.array(" ".join(k["kernel"] for k in info["kernels"])),
               classes=np.array([k["class"] for k in info["kernels"]], np.int64), grids=np.array([k["grid"] for k in info["kernels"]], np.int64),
               aux=np.array([k.get("aux", -1) for k in info["kernels"]], np.int64), unchanged=np.bool_(unchanged))
    return out


def public(torch, call, stats=None, **views):
    """A BCall through milp_batch; views: tensors to pass in place of the stacked copies, by name."""
    from yalps_amd import tensors
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    names = ("c", "A_ub", "b_ub", "A_eq", "b_eq")
    ops = [views.get(k, dev(a)) for k, a in zip(names, call.stacked())]
    lb, ub = (views.get(k, dev(a)) for k, a in zip(("lb", "ub"), call.bounds_stacked()))
    return tensors.milp_batch(*ops, lb=lb, ub=ub, upper=call.upper, integers=call.integers, binaries=call.binaries, maximize=call.maximize,
                              precision=call.precision, max_pivots=call.max_pivots, check_cycles=call.check, tolerance=call.tolerance,
                              max_iterations=call.max_iterations, stats=stats)


def plumbing(torch, out):
    import ctypes as C
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kernels_of = lambda stats: np.array(" ".join(k["kernel"] for k in stats["kernels"]))

    def put(tag, d):
        out.update({"%s/%s" % (tag, k): v for k, v in d.items()})

    # the table's rule call once more with clean numbers where the poisoned one has NaN: the same answer
    put("clean at binaries", MD.answer(public(torch, rule_calls()[1])))
    put("NaN at binaries public", MD.answer(public(torch, table_call("NaN at binaries"))))

    # shared bounds: [n] tensors (a batch stride of 0) against [B, n] copies
    per, shared = view_call()
    lb, ub = shared.bounds_stacked()
    put("shared", MD.answer(public(torch, shared, lb=dev(lb[0]), ub=dev(ub[0]))))
    put("shared copies", MD.answer(public(torch, shared)))
    # views: lb every other element of a wider tensor, ub a transposed slice behind a storage offset, A_ub transposed
    lb, ub = per.bounds_stacked()
    B, n = lb.shape
    lb_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda")
    lb_wide[:, ::2] = dev(lb)
    ub_t = torch.full((n + 2, B + 1), -9.0, dtype=torch.float64, device="cuda")
    ub_t[2:, 1:] = dev(ub.T)
    A_t = dev(per.stacked()[1].transpose(0, 2, 1))
    views = dict(lb=lb_wide[:, ::2], ub=ub_t[2:, 1:].t(), A_ub=A_t.transpose(1, 2))
    assert views["lb"].stride() == (2 * n, 2) and views["ub"].stride() == (1, B + 1) and views["ub"].storage_offset() == 2 * (B + 1) + 1
    stats = {}
    put("views", MD.answer(public(torch, per, stats, **views)))
    out["views/kernels"] = kernels_of(stats)
    out["views/unchanged"] = np.bool_(bool((lb_wide[:, 1::2] == -9.0).all().item()) and bool((ub_t[:2] == -9.0).all().item()))

    # the producer of lb on a side stream, directly before the call on that stream
    side = torch.cuda.Stream()
    half = dev(lb) * 0.5
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big @ big * 2.0 ** -11  # (work in front of the producer: every entry stays 1.0)
        made = half * 2.0 + big[:B, :n] - 1.0
        put("stream", MD.answer(public(torch, per, lb=made)))
    out["stream/lb"] = made.cpu().numpy()
    del side

    # B = 0
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    stats = {}
    empty = tensors.milp_batch(z(0, 3), z(0, 2, 3), z(0, 2), lb=z(0, 3), ub=z(3), upper=(0, 2), integers=[1], stats=stats)
    out["empty/shapes"] = np.array([d for t in empty for d in t.shape], np.int64)
    out["empty/launches"] = np.int64(stats["launches"])

    # no integer and no binary variable: linprog_batch with the same bounds
    call = lp_call()
    ops = [dev(a) for a in call.stacked()]
    lb, ub = (dev(a) for a in call.bounds_stacked())
    stats = {}
    put("no integers/milp", MD.answer(tensors.milp_batch(*ops, lb=lb, ub=ub, upper=(0, 2, 5), maximize=True, stats=stats)))
    out["no integers/kernels"] = kernels_of(stats)
    lp = tensors.linprog_batch(*ops, lb=lb, ub=ub, upper=(0, 2, 5), maximize=True)
    put("no integers/lp", dict(x=lp.x.cpu().numpy(), objective=lp.objective.cpu().numpy(), status=lp.status.cpu().numpy(), pivots=lp.pivots.cpu().numpy()))

    # a boundless call: milp_batch without lb / ub, yalps_milpdense_solve_bounds with both descriptors NULL, yalps_milpdense_solve
    call = MD.table_call("several nodes")
    ops = [dev(a) for a in call.stacked()]
    stats = {}
    put("boundless/public", MD.answer(tensors.milp_batch(*ops, integers=call.integers, maximize=True, stats=stats)))
    out["boundless/public kernels"] = kernels_of(stats)
    handle = nat.MilpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    put("boundless/solve", MD.run_call(torch, handle, call))
    _, operands = MD._device_operands(torch, call)
    B, n = len(call.lps), call.n
    full = lambda shape, dtype: torch.full(shape, -7, dtype=dtype, device="cuda")
    outs = dict(x=full((B, n), torch.float64), objective=full((B,), torch.float64), status=full((B,), torch.int32),
                nodes=full((B,), torch.int64), node_pivots=full((B,), torch.int64), root_pivots=full((B,), torch.int64))
    descs, ints = nat._dense_operands(operands), nat._index_list(call.ints)
    nat.milpdense_check(nat.milpdense_lib().yalps_milpdense_solve_bounds(
        handle.handle, B, n, call.m_ub, call.m_eq, *(C.byref(o) for o in descs), None, None, 0, None, ints.size, ints.ctypes.data, 0, None, 1,
        call.precision, call.max_pivots, 0, call.tolerance, call.max_iterations, 0, *(outs[k].data_ptr() for k in OUTPUTS), None))
    put("boundless/abi", {k: t.cpu().numpy() for k, t in outs.items()})
    out["boundless/abi kernels"] = np.array(" ".join(k["kernel"] for k in handle.info()["kernels"]))

    # partial outputs: the pointers that are passed are written, the others are not missed
    for want in PARTIAL:
        put("partial %s" % ("+".join(want) or "none"), run_call(torch, handle, partial_call(), want=want))

    # refusals: a host pointer for lb and for ub, by name, nothing launched, nothing written
    call = partial_call()
    _, _, operands, bounds = _device(torch, call)
    B, n = len(call.lps), call.n
    host = np.zeros((B, n))
    pinned = torch.zeros((B, n), dtype=torch.float64).pin_memory()
    x = torch.full((B, n), -7.0, dtype=torch.float64, device="cuda")
    messages = []
    for name, p in (("lb", host.ctypes.data), ("ub", pinned.data_ptr())):
        kw = dict(lb=bounds[0], ub=bounds[1])
        kw[name] = (p, n, 1, 0)
        try:
            handle.solve(B, n, call.m_ub, call.m_eq, operands, integers=call.ints, binaries=call.bins, upper=call.idx, x=x.data_ptr(), **kw)
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    out["refusal/messages"] = np.array(messages)
    out["refusal/untouched"] = np.bool_(bool((x == -7.0).all().item()) and not host.any())
    put("refusal/after", run_call(torch, handle, call))
    handle.close()

    # the identity-block route: explicit rows under A_ub, no bounds
    call = identity_call()
    put("identity/bounded", MD.answer(public(torch, call)))
    rows = identity_operands(call)
    stacked = [dev(np.stack([r[k] for r in rows])) for k in range(3)]
    put("identity/rows", MD.answer(tensors.milp_batch(*stacked, integers=True, maximize=True)))


def child_table(path):
    torch = MD._torch_first()
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
    out = MD.answer(public(torch, call, stats))
    out.update(reruns=np.int64(stats["reruns"]), launches=np.int64(stats["launches"]), overflows=np.int64(stats["overflows"]),
               passes=np.int64(1 + max(k["pass"] for k in stats["kernels"])), grids=np.array([k["grid"] for k in stats["kernels"]], np.int64),
               kernels=np.array(" ".join(k["kernel"] for k in stats["kernels"])),
               rerun_trees=np.array(tensors._milp_handles[next(iter(tensors._milp_handles))].info()["rerun_trees"], np.int64))
    np.savez(path, **out)


def child_mix(path):
    _public(MD._torch_first(), mix_call(), path)


def child_hist(path):
    import os
    assert os.environ.get("YALPS_MILPDENSE_HIST") == str(HIST)
    _public(MD._torch_first(), hist_call(), path)


if __name__ == "__main__":
    {"table": child_table, "mix": child_mix, "hist": child_hist}[sys.argv[1]](sys.argv[2])
