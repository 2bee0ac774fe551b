"""Helpers of tests/test_lp_dense_free_model.py and tests/test_lp_dense_free.py (TEST INFRASTRUCTURE): the calls the tests of
yalps_lpdense_solve_free / linprog_batch(free=) / linprog_objective_bounds(free=) make, and the three child processes that make
them on the GPU (tests/_lp_dense.py says why children: torch first).  Each child writes everything its calls left behind to one
.npz; the tests compare those files with the C oracle on tests/_np_dense_free.py's restatement.

  FCall           LBD.BCall with free variables: per LP (c, A_ub, b_ub, A_eq, b_eq, lb, ub), one `upper` and one `free` for the call
  table(oracle)   [FCall]: whole solves at the class bounds and in the HBM forms, the statuses, the non-finite data
  child "table"   the table through _native.LpDense with kept tableaux and all eight outputs; none / some / all output pointers;
                  then the plumbing through linprog_batch and linprog_objective_bounds
  child "hist"    under YALPS_LPDENSE_HIST=4: the rerun writes x of a free variable and its reduced cost
  hard_table()    [FCall]: the small calls that tell the mutants of FD.FLAWS, each twice: at max_pivots = 0 (the start tableau) and
                  with its own options
  child "hard"    the hard table
"""
import math
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _lp_dense as LD
from tests import _lp_dense_bounds as LBD
from tests import _np_dense as ND
from tests import _np_dense_free as FD

INF = math.inf
SENTINEL = LBD.SENTINEL
OUTPUTS = LBD.OUTPUTS
STATUS_LPS = 2100             # more than class 0's grid of 8 x 256 workgroups
STATUS_BUDGET = 2.0           # max_pivots of the call "statuses": an LP of more pivots ends "cycled"
STATUS_SEED = 0               # tests/test_lp_dense_free_model.py: all four endings, and an unbounded twin
GUARD = 0.5                   # a freed variable of a generated LP is held by a row -x[j] <= GUARD: the LP stays bounded


class FCall(LBD.BCall):
    def __init__(self, name, lps, upper=True, free=(), **options):
        super().__init__(name, lps, upper, **options)
        self.free = free
        self.fidx = FD.free_set(self.n, free)
        self.f = len(self.fidx)
        self.w += self.f

    def low(self, i):
        return FD.effective_lower(self.lbs[i], self.fidx)

    def oracle_answer(self, oracle, i, flaw=None):
        """flaw: None, or one of FD.FLAWS: the answer of a kernel that had that flaw (WRONG on purpose)."""
        lp, lb, ub = self.lps[i], self.lbs[i], self.ubs[i]
        m = FD.free_tableau(*lp, lb=lb, ub=ub, upper=self.idx, free=self.fidx, maximize=self.maximize, flaw=flaw)
        start = m.copy()
        pos, var = np.arange(self.w + self.h, dtype=np.int32), np.arange(self.w + self.h, dtype=np.int32)
        status, result, npiv, _ = oracle.simplex(m, self.w, self.h, pos, var, precision=self.precision, max_pivots=self.max_pivots,
                                                 check_cycles=self.check)
        col0 = m.reshape(self.h, self.w)[:, 0].copy()
        sign = 1.0 if self.maximize else -1.0
        x, objective = FD.free_solution(col0, pos, var, status, result, sign, self.precision, lp[0], lb, self.fidx, flaw=flaw)
        marg = FD.free_marginals(m, pos, status, self.n, self.m_ub, self.m_eq, self.k, self.fidx, sign, flaw=flaw)
        return dict(status=status, result=result, n_pivots=npiv, matrix=m, start=start, col0=col0, pos=pos, var=var, x=x, objective=objective,
                    **dict(zip(OUTPUTS, marg)))


def kernel_of(call):
    """(size class, the kernel's spelling) of a call: lp_dense_free_kernel with any free variable, else what the call ran before."""
    cls = LB.size_class(call.w, call.h)
    name = "lp_dense_free_kernel" if call.f else "lp_dense_bounds_kernel" if call.has_lb or call.has_ub else "lp_dense_kernel"
    return cls, "%s<%d%s%s>" % (name, 1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")


def random_lp(rng, n, m_ub, m_eq, mode, free):
    """LBD.random_lp (small integers around a point of the box) with the point's free coordinates moved by -4 .. 4: optima at
    negative x, and LPs unbounded downwards through a free variable that no row holds."""
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    lb, ub = LBD.random_bounds(rng, n, "both")
    x0 = lb + ints(0, 3, n)
    for j in free:
        x0[j] += ints(-4, 5, 1)[0]
    A_ub, A_eq = ints(-2, 4, m_ub, n), ints(-2, 4, m_eq, n)
    return (ints(-2, 5, n), A_ub if m_ub else None, A_ub @ x0 + ints(0, 4, m_ub) if m_ub else None, A_eq if m_eq else None,
            A_eq @ x0 if m_eq else None, lb if mode in ("lb", "both") else None, ub if mode in ("ub", "both") else None)


def random_call(name, B, n, m_ub, m_eq, mode="both", upper=True, free=(), seed=0, **options):
    rng = np.random.default_rng([20270101, B, n, m_ub, m_eq, len(mode), seed])
    fidx = FD.free_set(n, free)
    if mode in ("none", "lb"):
        upper = True
    return FCall(name, [random_lp(rng, n, m_ub, m_eq, mode, fidx) for _ in range(B)], upper, free, **options)


def freed_call(name, oracle, w, h, f, k, seed=3, B=1, **options):
    """Dense LPs of the oracle's generator, maximised, as a tableau of h x w with f twins and k bound rows: n = w - 1 - f variables
    of which the first, the middle and the last .. are free (f of them), each held by a guard row -x[j] <= GUARD; h - 1 - k - f rows of
    the generator; lb in eighths (not read at the free variables), a box on the first k variables -- the first is free."""
    n, m = w - 1 - f, h - 1 - k - f
    assert n > f > 0 and m > 0 and k <= n, (name, w, h, f, k)
    free = tuple(sorted({(t * (n - 1)) // (f - 1) for t in range(f)})) if f > 1 else (n - 1,)
    assert len(free) == f and free[-1] == n - 1, (name, free)
    rng = np.random.default_rng([20270102, w, h, f, k])
    lps = []
    for i in range(B):
        c, A, b = ND.from_tableau(oracle.dense_lp(m, n, seed + i), n + 1, m + 1)
        guard = np.zeros((f, n))
        guard[np.arange(f), list(free)] = -1.0
        lb = rng.integers(-2, 3, n).astype(np.float64) / 8.0
        ub = lb + rng.integers(2, 9, n).astype(np.float64) / 8.0
        lps.append((c, np.vstack([A, guard]), np.concatenate([b, np.full(f, GUARD)]), None, None, lb, ub))
    return FCall(name, lps, upper=tuple(range(k)), free=free, maximize=True, **options)


def bound_shapes():
    """LBD.bound_shapes()'s six points (odd widths), and the first class once more at an even width."""
    h0 = BS.rows_under(LB.BOUNDS[0], 48)
    return LBD.bound_shapes() + [(0, 48, h0), (0, 48, h0 + 1)]


def statuses_call(seed=STATUS_SEED):
    return random_call("statuses", STATUS_LPS, 4, 4, 0, upper=(0, 1), free=(1, 3), seed=seed, maximize=True, max_pivots=STATUS_BUDGET)


def nan_lb_calls():
    """lb holding NaN at every free index and finite values elsewhere, and the same call with 0.0 there."""
    a = random_call("nan lb at free", 6, 5, 4, 1, free=(0, 3), upper=(0, 1))
    b = random_call("zero lb at free", 6, 5, 4, 1, free=(0, 3), upper=(0, 1))
    for lb_a, lb_b in zip(a.lbs, b.lbs):
        lb_a[[0, 3]] = math.nan
        lb_b[[0, 3]] = 0.0
    return a, b


def nonfinite_call():
    """An infinite coefficient in a free column with lb given (the product with +0.0 is NaN: the row's right-hand side), -inf
    likewise, and ub = +inf at a free variable `upper` lists."""
    call = random_call("nonfinite", 6, 5, 3, 1, free=(1, 4), upper=(1, 2))
    call.lps[0][1][0, 1] = INF
    call.lps[1][3][0, 4] = -INF
    call.ubs[2][1] = INF
    call.lps[3][0][4] = INF
    return call


def hist_call(oracle):
    """LD.hist_call's four LPs (checkCycles, more pivots than 2 * HIST) with their first and last variable freed behind guard rows,
    lb in eighths and a box wide enough not to bind early."""
    base = LD.hist_call(oracle)
    rng = np.random.default_rng(20270103)
    n, free = base.n, (0, base.n - 1)
    lps = []
    for c, A, b, _, _ in base.lps:
        guard = np.zeros((2, n))
        guard[[0, 1], list(free)] = -1.0
        lb = rng.integers(-2, 3, n).astype(np.float64) / 8.0
        lps.append((c, np.vstack([A, guard]), np.concatenate([b, [GUARD, GUARD]]), None, None, lb, lb + 64.0))
    return FCall("hist free", lps, upper=(0, 1), free=free, maximize=True, check=True)


def names():
    out = ["class %d bound %s w=%d" % (k, "under" if j % 2 == 0 else "over", w) for j, (k, w, h) in enumerate(bound_shapes())]
    return out + ["HBM 301x280", "aux", "statuses", "nan lb at free", "zero lb at free", "nonfinite", "hist free clean"]


def table(oracle):
    T = []
    for j, (k, w, h) in enumerate(bound_shapes()):
        assert LB.size_class(w, h) == k + j % 2, (k, w, h)
        T.append(freed_call("class %d bound %s w=%d" % (k, "under" if j % 2 == 0 else "over", w), oracle, w, h, 3 if w % 2 else 4, 4, check=j == 3))
    assert LB.size_class(280, 301) == 4 and not BS.aux_hbm(280, 301)
    T.append(freed_call("HBM 301x280", oracle, 280, 301, 5, 6, check=True))
    m_ub, n = LD.AUX_SHAPE
    assert BS.aux_hbm(n + 1, m_ub + 1)
    T.append(freed_call("aux", oracle, n + 1, m_ub + 1, 2, 3, max_pivots=INF))
    T += [statuses_call(), *nan_lb_calls(), nonfinite_call()]
    clean = hist_call(oracle)
    clean.name = "hist free clean"
    T.append(clean)
    assert [c.name for c in T] == names()
    return T


def partial_call():
    return random_call("partial", 8, 5, 4, 3, free=(1, 4))


PARTIAL = LBD.PARTIAL


# ------------------------------------------------------------------------------------------------ the hard calls
# Small calls whose start tableau (max_pivots = 0) or whose answer tells the mutants of FD.FLAWS from the canonical statement;
# tests/test_lp_dense_free_model.py shows with the oracle alone which call tells which.
START_MODES = ("none", "lb", "ub", "both")
ROUNDING_PRECISION = 0.25


def zeros_call():
    """Operands holding +0.0 and -0.0 in the free columns: a twin zero is the other zero."""
    call = random_call("signed zeros", 4, 5, 3, 2, free=(0, 2), upper=(2, 3))
    for i, lp in enumerate(call.lps):
        lp[0][0], lp[0][2] = (0.0, -0.0) if i % 2 else (-0.0, 0.0)
        lp[1][:, 0], lp[1][1, 2] = 0.0, -0.0
        lp[3][0, 0], lp[3][1, 2] = -0.0, 0.0
    return call


def rounding_call():
    """precision = 0.25, data in eighths.  Minimise x0 over -x0 <= 5/8 with x0 free: the twin ends basic at 5/8, which rounds to 3/4
    (halves go up), so x0 = -3/4; rounding the difference -5/8 gives -1/2.  And random LPs in eighths under that precision, which
    ends "optimal" with reduced costs of up to a quarter still open: there the twin's term of a free variable's reduced cost shows."""
    e = lambda *v: np.array(v, np.float64) / 8.0
    pin = (e(8, 8), np.array([e(-8, 0), e(0, 8)]), e(5, 24), None, None, None, None)
    rng = np.random.default_rng(20270104)
    lps = [pin]
    for _ in range(23):
        A = rng.integers(-12, 13, (2, 2)).astype(np.float64) / 8.0
        lps.append((rng.integers(-12, 13, 2).astype(np.float64) / 8.0, A, rng.integers(0, 40, 2).astype(np.float64) / 8.0, None, None, None, None))
    return FCall("rounding", lps, free=(0,), precision=ROUNDING_PRECISION)


def hard_names():
    return (["start n=3 f=1 %s %s" % (mode, d) for mode in START_MODES for d in ("min", "max")]
            + ["n=65 free=(63,64) lb", "free=True n=5", "free in upper", "signed zeros", "rounding"])


def hard_table():
    T = [random_call("start n=3 f=1 %s %s" % (mode, d), 4, 3, 2, 1, mode=mode, free=(1,), maximize=d == "max")
         for mode in START_MODES for d in ("min", "max")]
    T += [random_call("n=65 free=(63,64) lb", 3, 65, 3, 2, mode="lb", free=(63, 64), maximize=True),
          random_call("free=True n=5", 6, 5, 4, 1, free=True),
          random_call("free in upper", 6, 5, 4, 1, upper=(1, 3), free=(1, 2), maximize=True),
          zeros_call(), rounding_call()]
    assert [c.name for c in T] == hard_names()
    return T


at_budget_0 = LBD.at_budget_0
differing = LBD.differing
_answers = {}


def answers(oracle, call, flaw=None):
    """[oracle_answer(i, flaw)] of a call, computed once per process."""
    key = (call.name, call.max_pivots, flaw)
    if key not in _answers:
        _answers[key] = [call.oracle_answer(oracle, i, flaw) for i in range(len(call.lps))]
    return _answers[key]


WORDS = ("start", "x", "objective", "reduced")


def words_of(refs):
    """The words that carry the build and the read-out -- the start tableau, x, the objective, the reduced costs -- as one array."""
    return np.concatenate([np.concatenate([np.atleast_1d(r[k]).ravel() for k in WORDS]) for r in refs])


def told(oracle, call):
    """The flaws whose words differ from the canonical ones on this call (the call at max_pivots = 0 counts with it)."""
    out = []
    for flaw in FD.FLAWS:
        if any(differing(words_of(answers(oracle, c, flaw)), words_of(answers(oracle, c))) for c in (call, at_budget_0(call))):
            out.append(flaw)
    return out


# ------------------------------------------------------------------------------------------------ the children

def run_call(torch, handle, call, want=OUTPUTS):
    """One FCall through LpDense.solve with kept tableaux, all outputs pre-filled with SENTINEL, the pointers of `want` passed."""
    B, n = len(call.lps), call.n
    ops, bnd, operands, bounds = LBD._device(torch, call)
    full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    x, objective = full((B, n), torch.float64), full((B,), torch.float64)
    status, pivots = full((B,), torch.int32), full((B,), torch.int64)
    marg = dict(ineqlin=full((B, call.m_ub), torch.float64), eqlin=full((B, call.m_eq), torch.float64), reduced=full((B, n), torch.float64),
                upper=full((B, call.k), torch.float64))
    ptr = lambda t: t.data_ptr() if t.numel() else None
    handle.solve(B, n, call.m_ub, call.m_eq, operands, maximize=call.maximize, precision=call.precision, max_pivots=call.max_pivots,
                 check_cycles=call.check, keep_tableaux=True, x=ptr(x), objective=ptr(objective), status=ptr(status), pivots=ptr(pivots),
                 lb=bounds[0], ub=bounds[1], upper=call.idx, free=call.fidx, **{("upper_out" if k == "upper" else k): ptr(marg[k]) for k in want})
    sols = [handle.solution(i) for i in range(B)]
    info = handle.info()
    after = [None if t is None else t.cpu().numpy() for t in ops + bnd]
    unchanged = all(a is None or LB.same_words(a, b, canonical_nan=False) for a, b in zip(after, call.stacked() + list(call.bounds_stacked())))
    out = dict(x=x.cpu().numpy(), objective=objective.cpu().numpy(), status=status.cpu().numpy(), pivots=pivots.cpu().numpy(),
               col0=np.stack([s[0] for s in sols]), pos=np.stack([s[1] for s in sols]), var=np.stack([s[2] for s in sols]),
               tableau=np.stack([handle.tableau(i) for i in range(B)]), launches=np.int64(info["launches"]), reruns=np.int64(info["reruns"]),
               kernels=np.array(" ".join(k["kernel"] for k in info["kernels"])), classes=np.array([k["class"] for k in info["kernels"]], np.int64),
               aux=np.array([k["aux"] for k in info["kernels"]], np.int64), grids=np.array([k["grid"] for k in info["kernels"]], np.int64),
               unchanged=np.bool_(unchanged))
    out.update({k: t.cpu().numpy() for k, t in marg.items()})
    return out


answer = LBD.answer


def public(torch, call, stats=None, duals=True, **more):
    """A call through linprog_batch, from contiguous device copies."""
    from yalps_amd import tensors
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lb, ub = call.bounds_stacked()
    kw = dict(lb=dev(lb), ub=dev(ub), free=call.free, maximize=call.maximize, precision=call.precision, max_pivots=call.max_pivots,
              check_cycles=call.check, duals=duals, stats=stats)
    if call.has_ub:
        kw["upper"] = call.upper
    kw.update(more)
    return tensors.linprog_batch(*[dev(a) for a in call.stacked()], **kw)


def views_inputs():
    """B = 6, n = 5, m_ub = 4, m_eq = 2 with per-LP operands (the views test) and with c, A_ub, lb and ub shared, b_ub per LP (the stride-0 test)."""
    call = random_call("views", 6, 5, 4, 2, upper=(1, 3, 4), free=(1, 2))
    first = call.lps[0]  # (infeasible as it stands, feasible once its right-hand sides grow)
    shared = FCall("shared", [(first[0], first[1], first[2] + i, first[3], first[4], call.lbs[0], call.ubs[0]) for i in range(len(call.lps))],
                   upper=(1, 3, 4), free=(1, 2))
    return call, shared


def gradient_call():
    """Minimise c . x with x1 free: an LP whose optimum has x1 < 0, the same with another c, and one made infeasible by its box."""
    e = lambda *v: np.array(v, np.float64) / 8.0
    lp = (e(-16, 8, 24), np.array([e(8, 16, 8), e(16, 8, 24), e(0, -8, 0)]), e(24, 64, 12), None, None, e(-8, 4, -4), e(8, 20, 12))
    other = (lp[0] * np.array([1.0, -1.0, 1.0]), *lp[1:])
    bad = list(lp)
    bad[6] = lp[6].copy()
    bad[6][0] = lp[5][0] - 1.0
    return FCall("gradient rows", [lp, other, tuple(bad)], free=(1,), precision=LBD.GRAD_PRECISION)


GRADIENT_WEIGHTS = LBD.GRADIENT_WEIGHTS


def plumbing(torch, out):
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def put(tag, d):
        out.update({"%s/%s" % (tag, k): v for k, v in d.items()})

    # free=() / False / None, with and without bounds: the kernels and the bits of the call without the argument
    call = LBD.partial_call()
    ops = [dev(a) for a in call.stacked()]
    lb, ub = (dev(a) for a in call.bounds_stacked())
    for tag, kw in (("today plain", {}), ("today bounds", dict(lb=lb, ub=ub))):
        stats = {}
        put(tag, answer(tensors.linprog_batch(*ops, duals=True, stats=stats, **kw)))
        out[tag + "/kernels"] = np.array(" ".join(k["kernel"] for k in stats["kernels"]))
        for name, none in (("()", ()), ("False", False), ("None", None)):
            stats = {}
            put("%s free=%s" % (tag, name), answer(tensors.linprog_batch(*ops, duals=True, stats=stats, free=none, **kw)))
            out["%s free=%s/kernels" % (tag, name)] = np.array(" ".join(k["kernel"] for k in stats["kernels"]))

    # refusals: a host pointer for lb, ub or upper_out, by name, nothing launched, nothing written
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    call = random_call("refusal", 3, 2, 2, 1, free=(1,))
    _, bnd, operands, bounds = LBD._device(torch, call)
    host = np.zeros((3, 2))
    hostop = (host.ctypes.data, 2, 1, 0)
    up = torch.full((3, 2), SENTINEL, dtype=torch.float64, device="cuda")
    messages = []
    for name in ("lb", "ub", "upper_out"):
        kw = dict(lb=bounds[0], ub=bounds[1], upper=call.idx, upper_out=up.data_ptr(), free=call.fidx)
        kw[name] = host.ctypes.data if name == "upper_out" else hostop
        try:
            handle.solve(3, 2, 2, 1, operands, **kw)
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    out["refusal/messages"] = np.array(messages)
    out["refusal/untouched"] = np.bool_(bool((up == SENTINEL).all().item()) and not host.any())
    put("refusal/after", run_call(torch, handle, call))
    handle.close()

    # shared operands (a batch stride of 0) against [B, ...] copies
    call, shared = views_inputs()
    c, A_ub, b_ub, A_eq, b_eq = (dev(a) for a in shared.stacked())
    lb, ub = (dev(a) for a in shared.bounds_stacked())
    kw = dict(upper=shared.upper, free=shared.free, duals=True)
    got = tensors.linprog_batch(c[0].clone(), A_ub[0].clone(), b_ub, A_eq, b_eq, lb=lb[0].clone(), ub=ub[0].clone(), **kw)
    put("shared", answer(got))
    out["shared/names"] = np.array(" ".join(tensors.status_names(got.status)))
    put("shared copies", answer(tensors.linprog_batch(c, A_ub, b_ub, A_eq, b_eq, lb=lb, ub=ub, **kw)))

    # views: A_ub and A_eq transposed (a column stride that is not 1), c every other element of a wider tensor, ub a transposed slice
    c, A_ub, b_ub, A_eq, b_eq = call.stacked()
    lb, ub = call.bounds_stacked()
    B, n = lb.shape
    A_ub_t, A_eq_t = dev(A_ub.transpose(0, 2, 1)), dev(A_eq.transpose(0, 2, 1))
    c_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda")
    c_wide[:, ::2] = dev(c)
    ub_t = torch.full((n + 2, B + 1), -9.0, dtype=torch.float64, device="cuda")
    ub_t[2:, 1:] = dev(ub.T)
    views = (c_wide[:, ::2], A_ub_t.transpose(1, 2), dev(b_ub), A_eq_t.transpose(1, 2), dev(b_eq))
    assert views[0].stride() == (2 * n, 2) and views[1].stride()[1:] == (1, call.m_ub) and ub_t[2:, 1:].t().stride() == (1, B + 1)
    kw = dict(upper=call.upper, free=call.free, duals=True)
    put("views", answer(tensors.linprog_batch(*views, lb=dev(lb), ub=ub_t[2:, 1:].t(), **kw)))
    copies = [dev(a) for a in (c, A_ub, b_ub, A_eq, b_eq)]
    put("views copies", answer(tensors.linprog_batch(*copies, lb=dev(lb), ub=dev(ub), **kw)))
    out["views/unchanged"] = np.bool_(bool((c_wide[:, 1::2] == -9.0).all().item()) and bool((ub_t[:2] == -9.0).all().item()))

    # the producer of c on a side stream, directly before the call on that stream
    side = torch.cuda.Stream()
    half = dev(c) * 0.5
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big @ big * 2.0 ** -11  # (work in front of the producer: every entry stays 1.0)
        made = half * 2.0 + big[:B, :n] - 1.0
        put("stream", answer(tensors.linprog_batch(made, *copies[1:], lb=dev(lb), ub=dev(ub), **kw)))
    out["stream/c"] = made.cpu().numpy()
    del side

    # B = 0
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    stats = {}
    empty = tensors.linprog_batch(z(0, 3), z(0, 2, 3), z(0, 2), lb=z(0, 3), ub=z(3), upper=(0, 2), free=(1,), duals=True, stats=stats)
    out["empty/shapes"] = np.array([d for t in empty for d in t.shape], np.int64)
    out["empty/type"] = np.array(type(empty).__name__)
    out["empty/launches"] = np.int64(stats["launches"])

    # linprog_objective_bounds(free=): every operand batched and requiring grad, one row infeasible; then c and lb shared
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_()
    call = gradient_call()
    ops = [None if a is None else leaf(a) for a in call.stacked()]
    lb, ub = (leaf(a) for a in call.bounds_stacked())
    objective, duals = tensors.linprog_objective_bounds(*ops, lb=lb, ub=ub, free=call.free, precision=call.precision)
    assert objective.grad_fn is not None and not any(t.requires_grad for t in duals)
    objective.backward(torch.tensor(GRADIENT_WEIGHTS, dtype=torch.float64, device="cuda"))
    put("gradient rows", answer(duals))
    for name, t in zip(("c", "A_ub", "b_ub", "lb", "ub"), (ops[0], ops[1], ops[2], lb, ub)):
        out["gradient rows/grad_%s" % name] = t.grad.cpu().numpy()
    ops = [None if a is None else leaf(a) for a in call.stacked()]
    ops[0] = leaf(call.lps[0][0])
    lb, ub = leaf(call.lbs[0]), leaf(call.bounds_stacked()[1])
    objective, duals = tensors.linprog_objective_bounds(*ops, lb=lb, ub=ub, free=call.free, precision=call.precision)
    objective.backward(torch.tensor(GRADIENT_WEIGHTS, dtype=torch.float64, device="cuda"))
    put("gradient shared", answer(duals))
    out["gradient shared/grad_c"], out["gradient shared/grad_lb"] = ops[0].grad.cpu().numpy(), lb.grad.cpu().numpy()


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
    np.savez(path, **out)


def child_hist(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import os
    assert os.environ.get("YALPS_LPDENSE_HIST") == str(LD.HIST)
    import torch
    torch.cuda.init()
    from tests import _oracle
    call = hist_call(_oracle.load())
    stats = {}
    out = answer(public(torch, call, stats))
    out.update(reruns=np.int64(stats["reruns"]), passes=np.int64(1 + max(k["pass"] for k in stats["kernels"])),
               kernels=np.array(" ".join(k["kernel"] for k in stats["kernels"])))
    np.savez(path, **out)


def child_hard(path):
    """Every call of hard_table twice through _native.LpDense with kept tableaux -- with max_pivots = 0 ("<name> @0": the kept
    tableau is the start tableau) and with its own options -- and once through linprog_batch(duals=True)."""
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from yalps_amd import _native as nat
    out = {}
    T = hard_table()
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in T:
            for c in (at_budget_0(call), call):
                out.update({"%s/%s" % (c.name, k): v for k, v in run_call(torch, handle, c).items()})
    finally:
        handle.close()
    for call in T:
        stats = {}
        got = answer(public(torch, call, stats))
        out.update({"%s public/%s" % (call.name, k): v for k, v in got.items()})
        out["%s public/kernels" % call.name] = np.array(" ".join(k["kernel"] for k in stats["kernels"]))
    np.savez(path, **out)


if __name__ == "__main__":
    {"table": child_table, "hist": child_hist, "hard": child_hard}[sys.argv[1]](sys.argv[2])
