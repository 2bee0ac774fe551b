"""Helpers of tests/test_milp_dense_free_model.py and tests/test_milp_dense_free.py (TEST INFRASTRUCTURE): the table of dense
MILP calls with free variables -- milp_batch_free(free=) -- and the child processes that run them on the GPU (tests/_milp_dense.py says
why children: torch first).  Each child writes everything its calls left behind to one .npz; the tests compare those files with
tests/_np_milp_dense_free.py: the oracle-driven search on the split tableau, moved back.

  table()         [FCall]: every call of the child "table", through _native.MilpDense with a trace
  child "table"   the table, then the plumbing through milp_batch_free and the equalities with the other calls
  child "mix"     mix_call() through milp_batch_free under the environment the test sets (YALPS_MILPDENSE_GRID / _ARENA / _ARENA_MAX)
  child "hist"    hist_call() through milp_batch_free under YALPS_MILPDENSE_HIST=4: the rerun of a free root refills the split tableau
                  from the operands, and the free epilogue reads what the last pass left
"""
import math
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _milp_dense as MD
from tests import _milp_dense_bounds as MDB
from tests import _np_milp_dense as NM
from tests import _np_milp_dense_bounds as NB
from tests import _np_milp_dense_free as NF

INF, NAN = math.inf, math.nan
TRACE_CAP = MD.TRACE_CAP
BUDGET = 48.0                 # maxIterations of a generated call (free_milp says why)
OUTPUTS = MDB.OUTPUTS
f = MD.f


def free_milp(rng, n, m_ub, m_eq, ints, bins, free, mode="both", grain=0.25):
    """MDB.bounded_milp's MILP around a point of its box, with the variables `free` freed: every second one of them gets a
    negative objective coefficient, so that the maximum pushes it down, and each a guard row -x[j] <= -(l[j] - d[j]) under A_ub so
    that it stops, below zero for most: l = ceil(lb) and d whole at an integer variable, d at a fraction at a continuous one.  (A
    free integer variable that an LP leaves at a fraction v starts a chain that no cut ends: q >= ceil(-v) is answered by p going
    up with it, x stays at v with the same objective, and the next cut is on p -- the reference's search too walks it until
    maxIterations.  So the guards are whole, such fractions come from the other rows alone, and every call has a small budget.)
    mode "none": neither lb nor ub (the guards and the positive first row bound the MILP)."""
    c, A_ub, b_ub, A_eq, b_eq, lb, ub = MDB.bounded_milp(rng, n, m_ub, m_eq, ints, bins, "ub" if mode == "none" else mode, grain)
    c = c.copy()
    free = list(free)
    c[free[::2]] *= -1.0
    low = np.zeros(n) if lb is None else NB.effective_lower(lb, n, sorted(set(ints) | set(bins)), sorted(bins))
    whole = np.array([j in set(ints) for j in free], bool)
    drop = 1.25 + 0.5 * (np.arange(len(free)) % 3) if grain is not None else 0.5 + rng.random(len(free))
    drop = np.where(whole, 1.0 + np.arange(len(free)) % 3, drop)
    guards = np.zeros((len(free), n))
    guards[np.arange(len(free)), free] = -1.0
    A = guards if A_ub is None else np.concatenate([A_ub, guards])
    b = -(low[free] - drop) if b_ub is None else np.concatenate([b_ub, -(low[free] - drop)])
    return c, A, b, A_eq, b_eq, lb, (None if mode == "none" else ub)


def call(name, B, n, m_ub, m_eq, ints=(), bins=(), free=(), mode="both", upper=True, grain=0.25, seed=0, **options):
    """m_ub counts the generator's rows; the call has len(free) guard rows more."""
    rng = np.random.default_rng([20261401, n, m_ub, m_eq, seed])
    options.setdefault("maximize", True)
    options.setdefault("max_iterations", BUDGET)
    fidx = NF.free_set(n, free, sorted(bins))
    out = NF.FCall(name, [free_milp(rng, n, m_ub, m_eq, ints, bins, fidx, mode, grain) for _ in range(B)], upper, free, integers=list(ints),
                   binaries=list(bins), **options)
    out.exact = grain is not None
    return out


def class_call(name, w, h, fr, n_int, seed=0, **options):
    """A root of h x w: fr free variables -- the first fr - 1, continuous, and the last variable, which is integer -- 4 bound rows
    on the first 4 variables, n_int integer variables (the last ones), no binary, data whose rounding shows."""
    n = w - 1 - fr
    free = list(range(fr - 1)) + [n - 1]
    return call(name, 1, n, h - 1 - 4 - fr, 0, ints=range(n - n_int, n), free=free, upper=(0, 1, 2, 3), grain=None, seed=seed, **options)


def hand_calls():
    """The rules on hand-made data."""
    none = (None, None)
    # p0 = 1.5 and q1 = 1.5 at the root: the first cut is on column 1 (the list ascends), under "twins first" on column 4.  The
    # objective holds both at their fractions, so the chain of free_milp's note starts here: twelve nodes, no solution.
    tie = NF.FCall("tie between a p and a q", [(f(1.0, -1.0), np.array([[1.0, 0.0], [0.0, -1.0]]), f(b0, 1.5), None, None, *none) for b0 in (1.5, 2.5)],
                   free=[0, 1], integers=[0, 1], maximize=True, max_iterations=12.0)
    # nothing stops x0 on its way down: the twin's column is unbounded, x0 = -inf
    fall = NF.FCall("unbounded through a twin", [(c, np.array([[1.0, 1.0]]), f(3.5), None, None, f(0.5, -0.25), f(9.0, 4.0)) for c in (f(-1.0, 0.0), f(-2.0, 1.0))],
                    free=[0], integers=[0, 1], maximize=True)
    # x0 <= 1 and x0 >= 2: free or not, no x0; the second MILP is feasible
    none_ = NF.FCall("infeasible row", [(f(1.0, 1.0), np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]]), f(1.0, b1, 2.5), None, None, f(0.0, 0.5), f(5.0, 5.0))
                                        for b1 in (-2.0, 2.5)], free=[0], integers=[0, 1], maximize=True)
    return [twin_call(), tie, fall, none_]


def picked(name, make, picks):
    """One call of the MILPs (seed, row) of make(seed): the rows of a generated shape that end the way the call is for."""
    made = {s: make(s) for s in sorted({s for s, _ in picks})}
    first = made[picks[0][0]]
    out = NF.FCall(name, [(*made[s].lps[i], made[s].lbs[i], made[s].ubs[i]) for s, i in picks], first.upper, first.free, integers=first.integers,
                   binaries=first.binaries, maximize=True, max_iterations=first.max_iterations)
    out.exact = first.exact
    return out


def twin_call():
    """A free integer variable whose optimum is a negative integer that only a cut on its twin reaches.  x0 is free and integer, its
    guard lies at a fraction (-x0 <= d + 0.5), and the objective is indifferent to it (c[0] = 0): the root leaves q0 at a fraction,
    the cut q0 >= ceil costs nothing, and the tree ends "optimal" -- where the objective pulls at x0 the same cut starts the
    chain.  The (seed, row) pairs: rows of the shape whose search cuts on column 1 + n and ends optimal with x0 < 0."""
    def make(seed):
        base = call("x", 4, 4, 2, 0, ints=[0, 3], free=[0, 1], seed=seed, max_iterations=32.0)
        lps = []
        for lp, lb, ub in zip(base.lps, base.lbs, base.ubs):
            c, b = lp[0].copy(), lp[2].copy()
            c[0] = 0.0
            b[-2] += 0.5
            lps.append((c, lp[1], b, None, None, lb, ub))
        return NF.FCall("x", lps, base.upper, base.free, integers=base.integers, maximize=True, max_iterations=32.0)
    return picked("negative optimum by the twin", make, ((47, 3), (1, 3), (24, 1), (30, 0)))


def poisoned(c, name):
    """The same call with NaN in lb at the free columns: lb is not read there."""
    lps = []
    for lp, lb, ub in zip(c.lps, c.lbs, c.ubs):
        lb = lb.copy()
        lb[list(c.fidx)] = NAN
        lps.append((*lp, lb, ub))
    out = NF.FCall(name, lps, c.upper, c.free, integers=c.integers, binaries=c.binaries, maximize=c.maximize, max_iterations=c.max_iterations)
    out.exact = c.exact
    return out


def clean_call():
    return call("clean at free", 3, 6, 3, 1, ints=[0, 3, 4], bins=[2], free=[0, 1, 4], seed=0)


R2 = BS.rows_under(LB.BOUNDS[2], 99)
# name: (w, root height, free variables, integer variables, the classes of the root, of the largest node without the twins' cuts and
# of the largest node; the seed)
SHAPES = {
    "LDS 1024": (99, R2 + 2, 6, 2, (3, 3, 3), 0),
    "256 to 1024 lanes by the twins' cuts": (99, R2 - 4, 6, 2, (2, 2, 3), 0),
    "HBM": (152, 160, 7, 2, (4, 4, 4), 0),
    "aux form": (31, 8170, 4, 2, (4, 4, 4), 0),
}
CHECKED = ("LDS 1024", "HBM")
LANES = (63, 64, 65, 129)
# (n, free, binaries): the width 1 + n + f goes over 32, a boundary of wg_unit_lanes, by one twin and by n - n_bin twins
EDGES = {"w = 32, f = 1": (30, [29], []), "w = 33, f = 1": (31, [30], []), "w = 34, f = 1": (32, [0], []),
         "w = 32, all free": (16, True, [3]), "w = 33, all free": (16, True, []), "w = 34, all free": (17, True, [3])}


def names():
    out = ["n=%d" % n for n in LANES] + list(EDGES)
    for name in SHAPES:
        out += [name] + ([name + " check"] if name in CHECKED else [])
    out += ["check at 256 lanes", "binary rows and twins", "free with a bound row, lb elsewhere", "lb only", "ub only", "no bounds", "equalities", "minimize",
            "NaN in lb at free", "negative optimum by the twin", "tie between a p and a q", "unbounded through a twin", "infeasible row",
            "timedout with a solution"]
    return out


def minimised(c):
    """The same MILPs with -c, minimised: the other sign in row 0, the same vertices."""
    out = NF.FCall(c.name, [(-lp[0], *lp[1:], lb, ub) for lp, lb, ub in zip(c.lps, c.lbs, c.ubs)], c.upper, c.free, integers=c.integers,
                   binaries=c.binaries, maximize=False, max_iterations=c.max_iterations)
    out.exact = c.exact
    return out


def table():
    T = [call("n=%d" % n, 2, n, 3, 1, ints=[0, 5, n - 1], bins=[1], free=[0, 2, n - 1], grain=None, max_iterations=24.0) for n in LANES]
    for name, (n, free, bins) in EDGES.items():
        T.append(call(name, 2, n, 3, 0, ints=[0, 2, n - 1], bins=bins, free=free, max_iterations=24.0))
        assert LB.size_class(T[-1].w, T[-1].hmax) <= 2, name
    for name, (w, h, fr, n_int, classes, seed) in SHAPES.items():
        for check in (False, True) if name in CHECKED else (False,):
            c = class_call(name + (" check" if check else ""), w, h, fr, n_int, seed=seed, max_iterations=5.0, check=check,
                           **({"max_pivots": INF} if w == 31 else {}))
            assert (c.w, c.h, c.int_twins) == (w, h, 1), (name, c.w, c.h)
            assert (LB.size_class(c.w, c.h), LB.size_class(c.w, c.h_no_twins), LB.size_class(c.w, c.hmax)) == classes, (name, c.w, c.h, c.hmax)
            assert BS.aux_hbm(c.w, c.h) == (name == "aux form")
            T.append(c)
    T += [call("check at 256 lanes", 3, 6, 3, 1, ints=[0, 3], bins=[1, 4], free=[0, 2, 3], seed=10, check=True),
          call("binary rows and twins", 3, 6, 3, 1, ints=[0, 3], bins=[1, 4], free=[0, 2, 3], seed=4),
          call("free with a bound row, lb elsewhere", 3, 5, 3, 0, ints=[0, 3], free=[0, 1], upper=(0, 2), seed=2),
          call("lb only", 3, 5, 3, 1, ints=[0, 3], bins=[2], free=[0, 4], mode="lb", seed=1),
          call("ub only", 3, 5, 3, 1, ints=[0, 3], bins=[2], free=[3], mode="ub", seed=2),
          call("no bounds", 3, 5, 3, 0, ints=[0, 3], bins=[2], free=[0, 1], mode="none", seed=3),
          call("equalities", 3, 6, 0, 2, ints=[1, 4], bins=[2], free=[1, 3], seed=6),
          minimised(call("minimize", 3, 5, 3, 1, ints=[0, 3], bins=[2], free=[0, 4], seed=0)),
          poisoned(clean_call(), "NaN in lb at free")]
    T += hand_calls()
    T.append(call("timedout with a solution", 3, 10, 10, 0, ints=range(8), free=[0, 2, 4, 9], max_iterations=6.0, seed=2))
    assert [c.name for c in T] == names(), [c.name for c in T]
    return T


_TABLE = {}


def table_call(name):
    if not _TABLE:
        _TABLE.update({c.name: c for c in table()})
    return _TABLE[name]


def mix_call():
    """MDB.mix_call's eight boxed MILPs, whose trees differ in size, with every second integer variable free: its objective
    coefficient negated and a guard row -x[j] <= 2 under A_ub (whole: free_milp says why), and a budget of 200 nodes.  The last
    two keep a root without a tree: the integral one (its guards at -x[j] <= 1) and the infeasible one."""
    mix = MDB.mix_call()
    free = mix.ints[::2]
    lps = []
    for i, (lp, lb, ub) in enumerate(zip(mix.lps, mix.lbs, mix.ubs)):
        c, A, b = lp[0].copy(), lp[1], lp[2]
        c[free] *= -1.0
        guards = np.zeros((len(free), mix.n))
        guards[np.arange(len(free)), free] = -1.0
        lps.append((c, np.concatenate([A, guards]), np.concatenate([b, np.full(len(free), 1.0 if i == 6 else 2.0)]), None, None, lb, ub))
    return NF.FCall("mix", lps, free=free, integers=mix.integers, maximize=True, max_iterations=200.0)


HIST = MDB.HIST


def hist_call():
    """MDB.hist_call's boxed MILPs (root LPs and nodes of more pivots than a history of HIST holds, checkCycles on) with every second
    integer variable free, as in mix_call: its objective coefficient negated and a guard row -x[j] <= 2 under A_ub (whole: free_milp
    says why), and a budget of 200 nodes."""
    hist = MDB.hist_call()
    free = hist.ints[::2]
    lps = []
    for lp, lb, ub in zip(hist.lps, hist.lbs, hist.ubs):
        c, A, b = lp[0].copy(), lp[1], lp[2]
        c[free] *= -1.0
        guards = np.zeros((len(free), hist.n))
        guards[np.arange(len(free)), free] = -1.0
        lps.append((c, np.concatenate([A, guards]), np.concatenate([b, np.full(len(free), 2.0)]), None, None, lb, ub))
    return NF.FCall("hist", lps, free=free, integers=hist.integers, maximize=True, check=True, max_iterations=200.0)


def lp_call():
    """No integer and no binary variable: linprog_batch(free=)'s problem."""
    return call("no integers", 4, 6, 4, 2, free=[1, 4], grain=None, seed=2)


def view_call():
    """B = 5, n = 6: per-MILP bounds (given as views) -- and, as "shared", one lb / ub for the batch ([n] tensors, batch stride 0)."""
    per = call("views", 5, 6, 3, 1, ints=[0, 2, 4], bins=[5], free=[0, 3], upper=(0, 2, 3), seed=3)
    shared = NF.FCall("shared", [(*lp, per.lbs[0], per.ubs[0]) for lp in per.lps], (0, 2, 3), per.free, integers=per.integers, binaries=per.binaries,
                      maximize=True, max_iterations=per.max_iterations)
    return per, shared


def concat_call():
    """Whole-number data, every variable integer, no lb: the caller's other route -- the negated columns appended with torch.cat, the
    integer set extended, the halves subtracted -- is the same MILP with an integer optimal value."""
    make = lambda seed: call("concat", 4, 5, 3, 0, ints=range(5), free=[0, 2], mode="ub", grain=1.0, seed=seed)
    return picked("concat", make, ((0, 0), (0, 3), (3, 2), (3, 3)))  # (the rows whose trees end "optimal" with nodes)


def plain_call():
    """The free=() calls: a bounded MILP without free variables."""
    return MDB.partial_call()


# ------------------------------------------------------------------------------------------------ the children

class WithFree:
    """A MilpDense whose solve passes `free` (and the entry point) on: MDB.run_call then runs an FCall."""

    def __init__(self, handle, free, entry=None):
        self.handle, self.free, self.entry = handle, list(free), entry

    def solve(self, *args, **kw):
        return self.handle.solve(*args, free=self.free, entry=self.entry, **kw)

    def __getattr__(self, name):
        return getattr(self.handle, name)


def run_call(torch, handle, call, want=OUTPUTS):
    return MDB.run_call(torch, WithFree(handle, call.fidx), call, want=want)


def public(torch, call, stats=None, **views):
    """An FCall through milp_batch_free; views: tensors to pass in place of the stacked copies, by name."""
    from yalps_amd import tensors
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ops = [views.get(k, dev(a)) for k, a in zip(("c", "A_ub", "b_ub", "A_eq", "b_eq"), call.stacked())]
    lb, ub = (views.get(k, dev(a)) for k, a in zip(("lb", "ub"), call.bounds_stacked()))
    return tensors.milp_batch_free(*ops, lb=lb, ub=ub, upper=call.upper, free=call.free, integers=call.integers, binaries=call.binaries,
                              maximize=call.maximize, precision=call.precision, max_pivots=call.max_pivots, check_cycles=call.check,
                              tolerance=call.tolerance, max_iterations=call.max_iterations, stats=stats)


def plumbing(torch, out):
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kernels_of = lambda stats: np.array(" ".join(k["kernel"] for k in stats["kernels"]))

    def put(tag, d):
        out.update({"%s/%s" % (tag, k): v for k, v in d.items()})

    # rule 2: NaN in lb at the free columns against clean numbers there
    put("clean at free", MD.answer(public(torch, clean_call())))
    put("NaN in lb at free public", MD.answer(public(torch, table_call("NaN in lb at free"))))

    # shared bounds, views, a side stream (as tests/_milp_dense_bounds.py)
    per, shared = view_call()
    lb, ub = shared.bounds_stacked()
    put("shared", MD.answer(public(torch, shared, lb=dev(lb[0]), ub=dev(ub[0]))))
    lb, ub = per.bounds_stacked()
    B, n = lb.shape
    lb_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda")
    lb_wide[:, ::2] = dev(lb)
    ub_t = torch.full((n + 2, B + 1), -9.0, dtype=torch.float64, device="cuda")
    ub_t[2:, 1:] = dev(ub.T)
    A_t = dev(per.stacked()[1].transpose(0, 2, 1))
    c_wide = torch.full((B, 3 * n), -9.0, dtype=torch.float64, device="cuda")
    c_wide[:, 1::3] = dev(per.stacked()[0])
    views = dict(lb=lb_wide[:, ::2], ub=ub_t[2:, 1:].t(), A_ub=A_t.transpose(1, 2), c=c_wide[:, 1::3])
    assert views["lb"].stride() == (2 * n, 2) and views["ub"].stride() == (1, B + 1) and views["A_ub"].stride()[2] != 1
    stats = {}
    put("views", MD.answer(public(torch, per, stats, **views)))
    out["views/kernels"] = kernels_of(stats)
    out["views/unchanged"] = np.bool_(bool((lb_wide[:, 1::2] == -9.0).all().item()) and bool((ub_t[:2] == -9.0).all().item())
                                      and bool((c_wide[:, ::3] == -9.0).all().item()))
    side = torch.cuda.Stream()
    half = dev(per.stacked()[1]) * 0.5
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big @ big * 2.0 ** -11  # (work in front of the producer: every entry stays 1.0)
        made = half * 2.0 + big[:half.shape[1], :n] - 1.0
        put("stream", MD.answer(public(torch, per, A_ub=made)))
    out["stream/A_ub"] = made.cpu().numpy()
    del side

    # B = 0
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    stats = {}
    empty = tensors.milp_batch_free(z(0, 3), z(0, 2, 3), z(0, 2), lb=z(0, 3), ub=z(3), upper=(0, 2), free=(0, 1), integers=[1], stats=stats)
    out["empty/shapes"] = np.array([d for t in empty for d in t.shape], np.int64)
    out["empty/launches"] = np.int64(stats["launches"])

    # no integer and no binary variable: linprog_batch with the same bounds and the same free variables
    call = lp_call()
    ops = [dev(a) for a in call.stacked()]
    lb, ub = (dev(a) for a in call.bounds_stacked())
    stats = {}
    put("no integers/milp", MD.answer(tensors.milp_batch_free(*ops, lb=lb, ub=ub, upper=(0, 1, 5), free=call.free, maximize=True, stats=stats)))
    out["no integers/kernels"] = kernels_of(stats)
    lp = tensors.linprog_batch(*ops, lb=lb, ub=ub, upper=(0, 1, 5), free=call.free, maximize=True)
    put("no integers/lp", dict(x=lp.x.cpu().numpy(), objective=lp.objective.cpu().numpy(), status=lp.status.cpu().numpy(), pivots=lp.pivots.cpu().numpy()))

    # free=(): milp_batch, milp_batch_free(free=()), yalps_milpdense_solve_free with n_free = 0 and yalps_milpdense_solve_bounds, bounded; and the same three
    # ways (the last: yalps_milpdense_solve) without bounds
    handle = nat.MilpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    call = plain_call()
    stats = {}
    put("plain/public", MD.answer(MDB.public(torch, call, stats)))
    out["plain/public kernels"] = kernels_of(stats)
    stats = {}
    ops = [dev(a) for a in call.stacked()]
    lb, ub = (dev(a) for a in call.bounds_stacked())
    put("plain/public free=()", MD.answer(tensors.milp_batch_free(*ops, lb=lb, ub=ub, upper=call.upper, free=(), integers=call.integers,
                                                             binaries=call.binaries, maximize=True, stats=stats)))
    out["plain/public free=() kernels"] = kernels_of(stats)
    put("plain/bounds", MDB.run_call(torch, handle, call))
    put("plain/free entry", MDB.run_call(torch, WithFree(handle, (), "free"), call))
    base = MD.table_call("several nodes")
    put("boundless/solve", MD.run_call(torch, handle, base))
    put("boundless/free entry", MD.run_call(torch, WithFree(handle, (), "free"), base))
    stats = {}
    put("boundless/public", MD.answer(tensors.milp_batch_free(*[dev(a) for a in base.stacked()], free=(), integers=base.integers, maximize=True, stats=stats)))
    out["boundless/public kernels"] = kernels_of(stats)

    # refusals: a host pointer for lb and for ub, by name, nothing launched, nothing written
    call = table_call("binary rows and twins")
    _, _, operands, bounds = MDB._device(torch, call)
    B, n = len(call.lps), call.n
    host = np.zeros((B, n))
    pinned = torch.zeros((B, n), dtype=torch.float64).pin_memory()
    x = torch.full((B, n), -7.0, dtype=torch.float64, device="cuda")
    messages = []
    for name, p in (("lb", host.ctypes.data), ("ub", pinned.data_ptr())):
        kw = dict(lb=bounds[0], ub=bounds[1])
        kw[name] = (p, n, 1, 0)
        try:
            handle.solve(B, n, call.m_ub, call.m_eq, operands, integers=call.ints, binaries=call.bins, upper=call.idx, free=call.fidx, x=x.data_ptr(), **kw)
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    for bad, kw in (("binary", dict(free=[1])), ("range", dict(free=[n])), ("order", dict(free=[2, 2]))):
        try:
            handle.solve(B, n, call.m_ub, call.m_eq, operands, integers=call.ints, binaries=call.bins, upper=call.idx, lb=bounds[0], ub=bounds[1],
                         x=x.data_ptr(), **kw)
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    out["refusal/messages"] = np.array(messages)
    out["refusal/untouched"] = np.bool_(bool((x == -7.0).all().item()) and not host.any())
    put("refusal/after", run_call(torch, handle, call))
    handle.close()

    # the concatenated route: [c, -c_F], [A_ub, -A_ub[:, F]] built with torch.cat, the integer set extended, the halves subtracted
    call = concat_call()
    put("concat/free", MD.answer(public(torch, call)))
    c, A, b = (dev(a) for a in call.stacked()[:3])
    F = list(call.fidx)
    wide_ub = torch.cat([dev(call.bounds_stacked()[1]), torch.zeros((len(call.lps), len(F)), dtype=torch.float64, device="cuda")], dim=1)
    # (x[j] <= ub[j] of a free variable is a row p - q <= ub, not a bound of the wider problem: the bounds of the others only)
    listed = [j for j in call.idx if j not in F]
    unit = torch.zeros((len(call.lps), len(F), call.n + len(F)), dtype=torch.float64, device="cuda")
    for t, j in enumerate(F):
        unit[:, t, j], unit[:, t, call.n + t] = 1.0, -1.0
    A_cat = torch.cat([torch.cat([A, -A[:, :, F]], dim=2), unit], dim=1)
    b_cat = torch.cat([b, dev(call.bounds_stacked()[1])[:, F]], dim=1)
    got = tensors.milp_batch(torch.cat([c, -c[:, F]], dim=1), A_cat, b_cat, ub=wide_ub, upper=listed,
                             integers=list(call.ints) + [call.n + t for t, j in enumerate(F) if j in call.ints], maximize=True)
    put("concat/cat", MD.answer(got))


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


def child_mix(path, call=None):
    torch = MD._torch_first()
    from yalps_amd import tensors
    stats = {}
    out = MD.answer(public(torch, call or mix_call(), stats))
    out.update(reruns=np.int64(stats["reruns"]), launches=np.int64(stats["launches"]), overflows=np.int64(stats["overflows"]),
               passes=np.int64(1 + max(k["pass"] for k in stats["kernels"])), grids=np.array([k["grid"] for k in stats["kernels"]], np.int64),
               kernels=np.array(" ".join(k["kernel"] for k in stats["kernels"])),
               rerun_trees=np.array(tensors._milp_handles[next(iter(tensors._milp_handles))].info()["rerun_trees"], np.int64))
    np.savez(path, **out)


def child_hist(path):
    import os
    assert os.environ.get("YALPS_MILPDENSE_HIST") == str(HIST)
    child_mix(path, hist_call())


if __name__ == "__main__":
    {"table": child_table, "mix": child_mix, "hist": child_hist}[sys.argv[1]](sys.argv[2])
