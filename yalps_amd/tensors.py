"""linprog_batch: batches of small dense LPs straight from torch tensors on the GPU (libyalps_lpdense.so), with variable
bounds lb <= x <= ub shifted and built on the device, free variables split and built there too, and with their dual solutions on request; linprog_objective: the optimal value as a differentiable torch function; milp_batch: batches of small
dense MILPs the same way, every branch-and-cut tree walked on the device (libyalps_milpdense.so).

This module imports torch; `import yalps_amd` does not.  linprog_batch computes nothing with torch: it supplies the device
pointers, the strides and the stream, and allocates the outputs.  linprog_objective's backward is a handful of torch
operations on the tensors linprog_batch returned.

Loading rule: torch brings its own HIP runtime, and a pointer or a stream is only good in the runtime that made it.  torch
must be initialised in the process before the first call into ANY of this package's libraries (solve, solve_many, _native
...): then they all resolve to the runtime torch loaded.  In the other order the library's runtime does not know torch's
memory, and linprog_batch refuses the call with a message that says so instead of handing the kernel a foreign pointer.
"""
import atexit
import threading
from collections import namedtuple

import torch

from . import _native

LinprogBatch = namedtuple("LinprogBatch", ("x", "objective", "status", "pivots"))
LinprogDuals = namedtuple("LinprogDuals", LinprogBatch._fields + ("ineqlin", "eqlin", "reduced_costs"))
LinprogBoundDuals = namedtuple("LinprogBoundDuals", LinprogDuals._fields + ("upper",))  # duals=True with ub given
MilpBatchResult = namedtuple("MilpBatchResult", ("x", "objective", "status", "nodes", "node_pivots", "root_pivots"))

STATUS_NAMES = _native.STATUS[:5]  # the YALPS_* codes 0..3 as solve() spells them, and 4, "timedout", which only a MILP ends with

_handles = {}  # (device index, stream) -> LpDense: stream, events and device buffers are kept and grown between calls
_milp_handles = {}  # (device index, stream) -> MilpDense, kept likewise
_fallbacks = {}  # device index -> MilpBatch: the lockstep driver, for trees that overflowed on the device
_lock = threading.Lock()  # (a handle belongs to one thread at a time)


def status_names(status):
    """The strings solve() uses -- "optimal", "infeasible", "unbounded", "cycled", and for milp_batch "timedout" -- for a
    status tensor (or any iterable of the codes)."""
    codes = status.tolist() if hasattr(status, "tolist") else list(status)
    return [STATUS_NAMES[int(k)] for k in codes]


@atexit.register
def _close_handles():
    with _lock:
        for table in (_handles, _milp_handles, _fallbacks):
            for h in table.values():
                h.close()
            table.clear()


def _operand(name, t, ndim, who="linprog_batch"):
    """A float64 tensor of `ndim` dimensions or one more (the batch in front): (tensor, B or None, its own shape)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a torch.Tensor, not %s" % (who, name, type(t).__name__))
    if t.dtype != torch.float64:
        raise TypeError("%s: %s is %s; only torch.float64 is solved" % (who, name, t.dtype))
    if t.dim() not in (ndim, ndim + 1):
        raise ValueError("%s: %s has %d dimensions, expected %d or %d (with the batch in front)" % (who, name, t.dim(), ndim, ndim + 1))
    batched = t.dim() == ndim + 1
    return t, (t.shape[0] if batched else None), tuple(t.shape[1:] if batched else t.shape)


def _strides(t, batched, matrix):
    """(ptr, batch, row, col) of yalps_lpdense_operand, in elements; None where the tensor has no element."""
    if t is None or t.numel() == 0:
        return None
    s = t.stride()
    return (t.data_ptr(), s[0] if batched else 0, s[-2] if matrix else s[-1], s[-1] if matrix else 0)


def _call_operands(who, c, A_ub, b_ub, A_eq, b_eq, check_size, vectors=None):
    """The five operands of a call, checked: (B, n, m_ub, m_eq, device, the five (ptr, batch, row, col) tuples, the tensors in
    that order with None where a side has no rows, which of them carry the batch dimension).  check_size(n, m_ub, m_eq)
    raises where the shape is above the call's limit; it runs after the shapes are known to agree and before the devices are
    looked at.  vectors: {name: tensor or None} of further [B, n] / [n] operands (lb, ub), checked like the others and
    returned as a ninth element, {name: (ptr, batch, row, col) or None}."""
    c, cB, (n,) = _operand("c", c, 1, who)
    batch = {"c": cB}
    more = {}
    for name, t in (vectors or {}).items():
        if t is not None:
            more[name], batch[name], (tn,) = _operand(name, t, 1, who)
            if tn != n:
                raise ValueError("%s: %s has %d entries, c has %d variables" % (who, name, tn, n))
    sides = []
    for tag, A, b in (("ub", A_ub, b_ub), ("eq", A_eq, b_eq)):
        if (A is None) != (b is None):
            raise ValueError("%s: A_%s and b_%s come together" % (who, tag, tag))
        if A is None:
            sides.append((None, None, 0))
            continue
        A, batch["A_" + tag], (m, An) = _operand("A_" + tag, A, 2, who)
        b, batch["b_" + tag], (bm,) = _operand("b_" + tag, b, 1, who)
        if An != n:
            raise ValueError("%s: A_%s has %d columns, c has %d variables" % (who, tag, An, n))
        if bm != m:
            raise ValueError("%s: A_%s has %d rows, b_%s has %d" % (who, tag, m, tag, bm))
        sides.append((A, b, m))
    sizes = {k: v for k, v in batch.items() if v is not None}
    if len(set(sizes.values())) > 1:
        raise ValueError("%s: the operands disagree about B: %s" % (who, ", ".join("%s has %d" % kv for kv in sizes.items())))
    B = next(iter(sizes.values()), 1)
    (A_ub, b_ub, m_ub), (A_eq, b_eq, m_eq) = sides
    check_size(n, m_ub, m_eq)
    given = (c, A_ub, b_ub, A_eq, b_eq)
    tensors = [t for t in given if t is not None] + list(more.values())
    if any(not t.is_cuda for t in tensors):
        raise ValueError("%s: the operands are read on the GPU where they lie: a CPU tensor was given "
                         "(move it with .cuda(), or use solve_many for models in host memory)" % who)
    device = c.device
    if any(t.device != device for t in tensors):
        raise ValueError("%s: the operands lie on different devices: %s" % (who, sorted({str(t.device) for t in tensors})))
    batched = tuple(batch.get(k) is not None for k in ("c", "A_ub", "b_ub", "A_eq", "b_eq"))
    operands = tuple(_strides(t, batched[k], k in (1, 3)) for k, t in enumerate(given))
    if vectors is not None:
        extra = {name: _strides(more.get(name), batch.get(name) is not None, False) for name in vectors}
        return B, n, m_ub, m_eq, device, operands, given, batched, extra
    return B, n, m_ub, m_eq, device, operands, given, batched


def _upper_set(n, upper, has_ub, who="linprog_batch"):
    """`upper` as the ascending list of 0-based variable indices whose ub entry the call reads (True: all n, where ub is given);
    raises ValueError for a duplicate, an index outside 0 .. n - 1, or a set given without ub, as milp_dense.integer_sets does."""
    if upper is True:
        return list(range(n)) if has_ub else []
    if not has_ub:
        raise ValueError("%s: upper names the variables whose ub entry is read, and no ub was given" % who)
    if upper is False or upper is None:
        upper = ()
    if isinstance(upper, (str, bytes)) or not hasattr(upper, "__iter__"):
        raise TypeError("%s: upper must be a sequence of variable indices or True, not %r" % (who, upper))
    idx = []
    for j in upper:
        if isinstance(j, bool) or int(j) != j:
            raise TypeError("%s: upper holds %r; variable indices are integers" % (who, j))
        idx.append(int(j))
    bad = [j for j in idx if not 0 <= j < n]
    if bad:
        raise ValueError("%s: upper names variable %d, outside 0 .. %d" % (who, bad[0], n - 1))
    if len(set(idx)) != len(idx):
        raise ValueError("%s: upper names variable %d twice" % (who, next(j for k, j in enumerate(idx) if j in idx[:k])))
    return sorted(idx)


def _free_set(n, free, who="linprog_batch"):
    """`free` as the ascending list of 0-based indices of the variables without a lower bound (True: all n; (), False, None:
    none); raises as _upper_set does: TypeError for a string, something that is no sequence, a bool or non-integer entry,
    ValueError for a duplicate or an index outside 0 .. n - 1."""
    if free is True:
        return list(range(n))
    if free is False or free is None:
        free = ()
    if isinstance(free, (str, bytes)) or not hasattr(free, "__iter__"):
        raise TypeError("%s: free must be a sequence of variable indices or True, not %r" % (who, free))
    idx = []
    for j in free:
        if isinstance(j, bool) or int(j) != j:
            raise TypeError("%s: free holds %r; variable indices are integers" % (who, j))
        idx.append(int(j))
    bad = [j for j in idx if not 0 <= j < n]
    if bad:
        raise ValueError("%s: free names variable %d, outside 0 .. %d" % (who, bad[0], n - 1))
    if len(set(idx)) != len(idx):
        raise ValueError("%s: free names variable %d twice" % (who, next(j for k, j in enumerate(idx) if j in idx[:k])))
    return sorted(idx)


def linprog_batch(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, *, lb=None, ub=None, upper=True, free=(), maximize=False, precision=1e-8,
                  max_pivots=8192, check_cycles=False, stats=None, duals=False):
    """Solves B dense LPs of one shape in one call, from device tensors to device tensors:

        minimize (or maximize=True: maximize)  c . x   subject to   A_ub x <= b_ub,   A_eq x = b_eq,   x >= 0

    c is [B, n] or [n]; A_ub / A_eq are [B, m, n] or [m, n]; b_ub / b_eq are [B, m] or [m]; all torch.float64 on one GPU.
    B is taken from whichever operand has the batch dimension (they must agree); with none, B = 1.  An operand without it
    is shared by all LPs: it is read with a batch stride of 0, nothing is materialised, and no operand is made contiguous
    -- transposed, sliced and expanded views are read through their strides (a last-dimension stride of 1 reads fastest).
    precision, max_pivots (may be inf) and check_cycles are the reference's options, for the whole call.

    Returns LinprogBatch(x [B, n] float64, objective [B] float64, status [B] int32, pivots [B] int64) on the inputs'
    device; status_names(status) spells the codes as solve() does.  The work is enqueued on torch's current stream of that
    device and the call returns after its one wait: the outputs are ready on return, and the inputs need only live as long
    as the call.  One int32 per LP crosses PCIe.

    The contract.  For finite data, row i is what solve() returns for the equivalent model -- constraints u0.. {"max":
    b_ub[i, r]}, then e0.. {"equal": b_eq[i, k]}, every variable listing every coefficient, zeros included -- with
    includeZeroVariables read off the dense x: "optimal" gives the variables' values (those not above precision are +0.0)
    and objective = solve()'s result; "unbounded" gives +0.0 but +inf at the unbounded variable and objective = +-inf
    (the variable whose own column the simplex found unbounded: where that column is a row's slack, no entry of x is infinite);
    "infeasible" and "cycled" give NaN everywhere.  For any data, NaN and infinities included, it is what the reference's
    `simplex` and `solution` give on the tableau as built: values are taken as they lie in memory.

    Raises TypeError / ValueError, before the library is touched, for anything but float64 tensors, mismatched B, m or n,
    a tableau (n + 1) x (1 + m_ub + 2 m_eq) above 4 MiB (solve() is the route for such models), CPU tensors and tensors on
    different devices.  stats (a dict, optional) receives "launches", "reruns", "kernels" and "gpu_ms" of the call.

    duals=True returns LinprogDuals(x, objective, status, pivots, ineqlin [B, m_ub], eqlin [B, m_eq], reduced_costs [B, n]):
    the same four tensors, bit for bit, and the dual solution of every LP, float64 on the inputs' device (a side without
    rows gives a tensor with no element, not None), written by the workgroup that solved the LP from its final tableau.
    Sign: ineqlin = d(objective) / d(b_ub), eqlin = d(objective) / d(b_eq) and reduced_costs = the objective's change per
    unit of a variable that is at zero, all in the caller's own direction, `objective` being the tensor returned.  With
    maximize=False they are scipy.optimize.linprog's ineqlin.marginals, eqlin.marginals and lower.marginals; with
    maximize=True the negations of what scipy reports for -c.  At a degenerate vertex the duals are not unique: these are
    the ones of the basis the reference's pivot rule ends in.  Every "optimal" row satisfies, up to rounding,
        objective = ineqlin . b_ub + eqlin . b_eq        and        reduced_costs = c - A_ub^T ineqlin - A_eq^T eqlin.
    Any other status -- "unbounded" too, which has no dual solution -- gives NaN in all three rows.  They equal, bit for
    bit, the "dual" and "reduced_cost" sensitivity() reports for the equivalent model.

    Bounds.  lb ([B, n] or [n], float64, read through its strides where it lies, every entry) means x >= lb and REPLACES
    x >= 0 for the call, so negative entries are legal.  ub ([B, n] or [n]) means x[j] <= ub[j] for the variables `upper` names: a
    HOST sequence of 0-based indices, or True for all n, shared by the batch -- what changes the tableau's height is host data,
    and one call has one shape.  Entries of ub at unlisted variables are never read.  A duplicate or out-of-range index, and
    an `upper` other than True without ub, raise ValueError before the library is touched.  Nothing is materialised: lb is a
    substitution x = lb + x' made on the device, which moves every right-hand side by the row's shift_sum(A[i], lb) -- a sum of
    individually rounded products in one fixed order (64 partial sums over the columns j = k mod 64 in ascending j, then folded
    by 32, 16, .. 1) -- with one subtraction, and x and the objective back with one addition each (objective += shift_sum(c, lb));
    ub adds k = len(upper) generated rows below the equality rows, in ascending index: ub[j] - lb[j] in column 0 and 1.0 in
    the variable's column.  The tableau is (n + 1) x (1 + m_ub + 2 m_eq + k), and the 4 MiB limit holds for that height.  For
    finite data row i is solve() of the equivalent model in x': linprog_batch's constraints with the shifted right-hand
    sides, then h<j> {"max": ub[j] - lb[j]} in which variable j alone has a coefficient, 1.  Without lb and ub the call is
    what it was, bit for bit, and launches the same kernels.
    With duals=True and ub given the result is LinprogBoundDuals: LinprogDuals' seven fields plus upper [B, k], the marginals
    of x[j] <= ub[j] in ascending index (scipy's upper.marginals); reduced_costs keeps its name and is the marginal of x >= lb
    (scipy's lower.marginals).  Every "optimal" row satisfies, up to rounding,
        reduced_costs = c - A_ub^T ineqlin - A_eq^T eqlin - scatter(upper)    and
        objective = ineqlin . b_ub + eqlin . b_eq + upper . ub + reduced_costs . lb.

    Free variables.  `free` is a HOST sequence of 0-based indices of the variables that have no lower bound (scipy's
    bounds=(None, ...)), or True for all n, shared by the batch -- it changes the tableau's width, and one call has one shape.
    (), False and None mean none, and such a call is the call it was: the same kernels, the same bits, with and without
    bounds.  It is checked like `upper`: a duplicate or out-of-range index raises ValueError, a string, a bool or a
    non-integer entry TypeError, before the library is touched.  Nothing is materialised: a free variable j is split on the
    device as x[j] = p[j] - q[j] with p, q >= 0; p keeps column 1 + j and the f = len(free) twins q are generated columns
    behind the n originals in ascending j, each cell the IEEE negation of the cell of column 1 + j in its row (a negation of
    the value read, not a second product: row 0 holds -(sign c[j]), a zero becomes -0.0, the negated row of an equality
    holds A_eq[k, j] again).  The tableau is (1 + n + f) x (1 + m_ub + 2 m_eq + k), and the 4 MiB limit holds for that shape.
    lb is NOT read at a free variable: its effective lower bound is +0.0 (the product with +0.0 is still formed in shift_sum,
    which runs over the n original columns alone).  A free variable that `upper` lists keeps its bound row, with -1.0 in the
    twin's column: x[j] <= ub[j] and no lower bound, scipy's (None, ub).  For finite data row i is solve() of the equivalent
    model: the bounded call's, plus one variable q<j> per free variable behind all x<j>, listing the negated coefficient of
    every constraint x<j> lists, and -c[j].  "optimal" gives x[j] = v(p) - v(q), each v the rule above on its own column,
    then + the effective lower bound where lb is given; "unbounded" gives +inf at the unbounded column, so -inf at a free
    variable whose twin it is.  reduced_costs[j] of a free variable is the full signed reduced cost, the p column's term minus
    the twin's -- about 0 at an optimum, as scipy reports -- so the two identities above hold at every j, with the effective
    lower bound in place of lb.  A call with free variables runs lp_dense_free_kernel, with or without lb / ub.
    Out of scope: per-LP `upper` and `free` sets, and inferring freeness from the data (an lb entry of -inf at a variable `free`
    does not list is taken as it lies in memory, like every other value).  milp_batch takes lb, ub and upper; milp_batch_free takes free too.

    See the module's docstring for the loading rule: torch first."""
    sets = {}

    def size(n, m_ub, m_eq):
        k = len(sets.setdefault("upper", _upper_set(n, upper, ub is not None)))
        f = len(sets.setdefault("free", _free_set(n, free)))
        w, h = n + 1 + f, 1 + m_ub + 2 * m_eq + k
        if 8 * w * h > _native.LPDENSE_MAX_BYTES:
            raise ValueError("linprog_batch: a tableau of %d x %d doubles (%d bytes) is above the batch limit of %d bytes; "
                             "solve() is the route for such models" % (h, w, 8 * w * h, _native.LPDENSE_MAX_BYTES))

    B, n, m_ub, m_eq, device, operands, _, _, bounds = _call_operands("linprog_batch", c, A_ub, b_ub, A_eq, b_eq, size,
                                                                      vectors={"lb": lb, "ub": ub})
    idx, fidx = sets["upper"], sets["free"]
    bounded = lb is not None or ub is not None
    ptr = lambda t: t.data_ptr() if t.numel() else None
    x = torch.empty((B, n), dtype=torch.float64, device=device)
    objective = torch.empty((B,), dtype=torch.float64, device=device)
    status = torch.empty((B,), dtype=torch.int32, device=device)
    pivots = torch.empty((B,), dtype=torch.int64, device=device)
    marginals = [torch.empty((B, k), dtype=torch.float64, device=device) for k in (m_ub, m_eq, n)] if duals else []
    upper_out = torch.empty((B, len(idx)), dtype=torch.float64, device=device) if duals and ub is not None else None
    more = {}
    if bounded:
        # (a bound tensor without an element -- n = 0 -- stays a descriptor, so that the call still is the bounded one)
        more = dict(lb=None if lb is None else bounds["lb"] or (None, 0, 0, 0), ub=None if ub is None else bounds["ub"] or (None, 0, 0, 0),
                    upper=idx, upper_out=None if upper_out is None else ptr(upper_out))
    if fidx:
        more["free"] = fidx
    with torch.cuda.device(device), _lock:  # (the library selects the handle's device; torch's choice comes back afterwards)
        stream = torch.cuda.current_stream(device).cuda_stream or 1  # (the default stream's handle is 0: hipStreamLegacy names it)
        key = (device.index, stream)
        handle = _handles.get(key)
        if handle is None:
            handle = _handles[key] = _native.LpDense(device.index, stream=stream)
        ms = handle.solve(B, n, m_ub, m_eq, operands, maximize=maximize, precision=precision, max_pivots=max_pivots,
                          check_cycles=check_cycles, x=ptr(x), objective=ptr(objective), status=ptr(status), pivots=ptr(pivots),
                          **{k: ptr(t) for k, t in zip(("ineqlin", "eqlin", "reduced"), marginals)}, **more)
        if stats is not None:
            info = handle.info()
            stats.update(launches=info["launches"], reruns=info["reruns"], kernels=info["kernels"], gpu_ms=ms)
    if upper_out is not None:
        return LinprogBoundDuals(x, objective, status, pivots, *marginals, upper_out)
    if duals:
        return LinprogDuals(x, objective, status, pivots, *marginals)
    return LinprogBatch(x, objective, status, pivots)


class _Objective(torch.autograd.Function):
    """objective [B] of B LPs whose five operands all carry the batch dimension (None: no rows of that kind); the solve's
    whole answer rides along as non-differentiable outputs.  Backward is the envelope theorem on what forward saved."""

    @staticmethod
    def forward(ctx, options, c, A_ub, b_ub, A_eq, b_eq):
        out = linprog_batch(c, A_ub, b_ub, A_eq, b_eq, duals=True, **options)
        ctx.sides = (A_ub is not None, A_eq is not None)
        ctx.save_for_backward(out.x, out.status, out.ineqlin, out.eqlin)
        rest = out[:1] + out[2:]
        ctx.mark_non_differentiable(*rest)
        return (out.objective, *rest)

    @staticmethod
    def backward(ctx, g, *_):
        x, status, ineqlin, eqlin = ctx.saved_tensors
        ok = (status == 0).unsqueeze(1)
        zero = torch.zeros((), dtype=x.dtype, device=x.device)
        # (where, not a product: the NaN of a row that did not end optimal times 0 would still be NaN)
        g = torch.where(ok, g.unsqueeze(1), zero)
        x, ineqlin, eqlin = torch.where(ok, x, zero), torch.where(ok, ineqlin, zero), torch.where(ok, eqlin, zero)
        need = ctx.needs_input_grad
        grads = [None, g * x if need[1] else None]
        for k, (has, y) in enumerate(zip(ctx.sides, (ineqlin, eqlin))):
            gy = g * y
            grads.append(-gy.unsqueeze(2) * x.unsqueeze(1) if has and need[2 + 2 * k] else None)
            grads.append(gy if has and need[3 + 2 * k] else None)
        return tuple(grads)


class _BoundedObjective(torch.autograd.Function):
    """_Objective for a call with lb or ub (None: absent): the same forward and the same five gradients with the full x, plus
    d lb = g reduced_costs (exactly 0 at a free variable) and d ub = g upper scattered into a [B, n] zero tensor."""

    @staticmethod
    def forward(ctx, options, sets, c, A_ub, b_ub, A_eq, b_eq, lb, ub):
        upper, free = sets
        out = linprog_batch(c, A_ub, b_ub, A_eq, b_eq, lb=lb, ub=ub, upper=upper, free=free, duals=True, **options)
        ctx.sides = (A_ub is not None, A_eq is not None)
        ctx.bounds = (lb is not None, ub is not None)
        ctx.upper = _upper_set(c.shape[-1], upper, ub is not None)
        ctx.free = _free_set(c.shape[-1], free)
        ctx.save_for_backward(out.x, out.status, out.ineqlin, out.eqlin, out.reduced_costs, *out[7:])
        rest = out[:1] + out[2:]
        ctx.mark_non_differentiable(*rest)
        return (out.objective, *rest)

    @staticmethod
    def backward(ctx, g, *_):
        x, status, ineqlin, eqlin, reduced, *upper = ctx.saved_tensors
        ok = (status == 0).unsqueeze(1)
        zero = torch.zeros((), dtype=x.dtype, device=x.device)
        g = torch.where(ok, g.unsqueeze(1), zero)
        x, ineqlin, eqlin, reduced = (torch.where(ok, t, zero) for t in (x, ineqlin, eqlin, reduced))
        need = ctx.needs_input_grad
        grads = [None, None, g * x if need[2] else None]
        for k, (has, y) in enumerate(zip(ctx.sides, (ineqlin, eqlin))):
            gy = g * y
            grads.append(-gy.unsqueeze(2) * x.unsqueeze(1) if has and need[3 + 2 * k] else None)
            grads.append(gy if has and need[4 + 2 * k] else None)
        d_lb = None
        if ctx.bounds[0] and need[7]:
            d_lb = g * reduced
            free = getattr(ctx, "free", ())
            if free:
                d_lb[:, free] = 0.0  # (lb is not read at a free variable)
        grads.append(d_lb)
        d_ub = None
        if ctx.bounds[1] and need[8]:
            d_ub = torch.zeros_like(x)
            d_ub[:, ctx.upper] = g * torch.where(ok, upper[0], zero)
        grads.append(d_ub)
        return tuple(grads)


def _objective_call(who, options, given, upper=True, free=()):
    """linprog_objective and linprog_objective_bounds behind their argument lists: given = {name: tensor or None} of the five
    operands, and of lb / ub where the call has bounds."""
    for tag in ("ub", "eq"):
        if (given["A_" + tag] is None) != (given["b_" + tag] is None):
            raise ValueError("%s: A_%s and b_%s come together" % (who, tag, tag))
    ndim = {"c": 1, "A_ub": 2, "b_ub": 1, "A_eq": 2, "b_eq": 1, "lb": 1, "ub": 1}
    sizes = {}
    for name, t in given.items():
        if t is not None:
            batched = _operand(name, t, ndim[name], who)[1]
            if batched is not None:
                sizes[name] = batched
    if len(set(sizes.values())) > 1:
        raise ValueError("%s: the operands disagree about B: %s" % (who, ", ".join("%s has %d" % kv for kv in sizes.items())))
    B = next(iter(sizes.values()), 1)
    # a shared operand as a view with a batch stride of 0, in front of the Function: autograd sums its gradient over the batch
    expanded = [None if t is None else (t if name in sizes else t.unsqueeze(0).expand(B, *t.shape)) for name, t in given.items()]
    if "lb" in given:
        has_ub = given["ub"] is not None
        _upper_set(given["c"].shape[-1], upper, has_ub, who)
        _free_set(given["c"].shape[-1], free, who)
        objective, *rest = _BoundedObjective.apply(options, (upper, free), *expanded)
        return objective, (LinprogBoundDuals if has_ub else LinprogDuals)(rest[0], objective.detach(), *rest[1:])
    objective, *rest = _Objective.apply(options, *expanded)
    return objective, LinprogDuals(rest[0], objective.detach(), *rest[1:])


def linprog_objective(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, *, maximize=False, precision=1e-8, max_pivots=8192,
                      check_cycles=False):
    """The optimal value of B dense LPs as a differentiable function of their data: (objective [B], LinprogDuals).

    The operands and options are linprog_batch's.  Forward is one linprog_batch(..., duals=True) on the detached operands;
    `objective` is LinprogDuals.objective, and carries a grad_fn when any operand requires grad.  Backward solves nothing:
    it is the envelope theorem on the tensors of the forward call, computed with torch operations on the device.  Per LP,
    with g the incoming gradient:

        dc = g x      db_ub = g ineqlin      db_eq = g eqlin      dA_ub = -g ineqlin (x) x      dA_eq = -g eqlin (x) x

    An operand without the batch dimension is shared by the LPs and receives the sum over the batch.

    A row whose status is not "optimal" contributes a zero gradient to every operand: its objective is +-inf or NaN and its
    marginals are NaN, and neither may poison the sum a shared operand receives.  The returned LinprogDuals.status says
    which rows those are; mask their objectives before reducing them to a loss.

    The optimal value is piecewise linear in b and c.  Inside a piece these are its derivatives; at a degenerate vertex,
    where pieces meet, they are one subgradient -- the one of the basis the solve ended in.  `objective` is rounded to
    `precision` as solve() rounds its result, so finite differences of it are only good to precision / step.  x itself is
    piecewise constant and is returned without a gradient.

    linprog_objective_bounds is this function for LPs with variable bounds."""
    options = dict(maximize=maximize, precision=precision, max_pivots=max_pivots, check_cycles=check_cycles)
    return _objective_call("linprog_objective", options, {"c": c, "A_ub": A_ub, "b_ub": b_ub, "A_eq": A_eq, "b_eq": b_eq})


def linprog_objective_bounds(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, *, lb=None, ub=None, upper=True, free=(), maximize=False,
                             precision=1e-8, max_pivots=8192, check_cycles=False):
    """linprog_objective with linprog_batch's bounds lb, ub and upper (a function of its own: linprog_objective keeps the
    argument list it has): (objective [B], what linprog_batch(..., lb=, ub=, upper=, duals=True) returns -- LinprogBoundDuals
    where ub is given, else LinprogDuals).  linprog_objective's five formulas hold unchanged with the full x, and

        dlb = g reduced_costs      dub = g upper, scattered into a [B, n] zero tensor (a variable `upper` does not list: 0)

    A shared lb or ub receives the sum over the batch; a row that is not "optimal" contributes exact zeros.  `free` is
    linprog_batch's: all formulas hold with the full x, which may now be negative, and dlb is exactly 0 at a free variable,
    where lb is not read.  Per-LP `upper` and `free` sets are out of scope, as in linprog_batch."""
    options = dict(maximize=maximize, precision=precision, max_pivots=max_pivots, check_cycles=check_cycles)
    given = {"c": c, "A_ub": A_ub, "b_ub": b_ub, "A_eq": A_eq, "b_eq": b_eq, "lb": lb, "ub": ub}
    return _objective_call("linprog_objective_bounds", options, given, upper, free)


def _solve_on_host(device, rows, given, batched, B, ints, bins, maximize, options, out, bounds=(None, None), bounds_batched=(False, False),
                   upper=(), free=()):
    """The trees `rows` of a milp_batch call through the lockstep driver (_native.MilpBatch.solve), as solve.milptree_solve
    sends its overflows: their operands are gathered on the device and copied to the host, their tableaux built there
    (milp_dense.packed_milp), and x / objective / status / nodes written into the output tensors `out`.  node_pivots of such
    a row is -1: the lockstep driver does not count the pivots of the nodes it consumes.  bounds = (lb, ub) tensors or None:
    gathered likewise, the tableaux are the bounded ones and x / objective are moved back (milp_dense.dense_solution).  free:
    the tableaux are the split ones, the driver branches on the twins of the free integer variables too, and the halves are
    subtracted on the way back."""
    from . import milp_dense
    idx = torch.tensor(rows, dtype=torch.int64, device=device)
    host = []
    for t, has_batch in zip(given, batched):
        if t is None:
            host.append(None)
        else:
            host.append((t.index_select(0, idx) if has_batch else t).cpu().numpy())
    lbs, ubs = (None if t is None else (t.index_select(0, idx) if has_batch else t).cpu().numpy() for t, has_batch in zip(bounds, bounds_batched))
    pick = lambda k, a, has_batch: None if a is None else (a[k] if has_batch else a)
    low_of = lambda k: milp_dense.effective_lower(pick(k, lbs, bounds_batched[0]), ints, bins, free)
    milps = [milp_dense.packed_milp(tuple(pick(k, a, hb) for a, hb in zip(host, batched)), ints, bins, maximize, options,
                                    lb=pick(k, lbs, bounds_batched[0]), ub=pick(k, ubs, bounds_batched[1]), upper=upper, free=free)
             for k in range(len(rows))]
    batch = _fallbacks.get(device.index)
    if batch is None:
        batch = _fallbacks[device.index] = _native.MilpBatch(device.index)
    statuses, results, used, _, _ = batch.solve(milps)
    n = out.x.shape[1]
    sign = 1.0 if maximize else -1.0
    xs, objs = [], []
    for k, (st, res) in enumerate(zip(statuses, results)):
        _, col0, pos, var = batch.solution(k)
        x, obj = milp_dense.dense_solution(col0, pos, var, st, float(res), sign, options["precision"], n,
                                           c=pick(k, host[0], batched[0]), low=low_of(k), free=free)
        xs.append(x)
        objs.append(obj)
    dev = lambda a, dtype: torch.as_tensor(a, dtype=dtype).to(device)
    import numpy as np
    out.x.index_copy_(0, idx, dev(np.stack(xs), torch.float64))
    out.objective.index_copy_(0, idx, dev(np.array(objs, np.float64), torch.float64))
    out.status.index_copy_(0, idx, dev(np.array([_native.STATUS.index(s) for s in statuses], np.int32), torch.int32))
    out.nodes.index_copy_(0, idx, dev(np.asarray(used, np.int64), torch.int64))
    out.node_pivots.index_fill_(0, idx, -1)


def milp_batch(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, *, lb=None, ub=None, upper=True, integers=(), binaries=(), maximize=False,
               precision=1e-8, max_pivots=8192, check_cycles=False, tolerance=0.0, max_iterations=32768, stats=None):
    """Solves B dense MILPs of one shape in one call, from device tensors to device tensors, every branch-and-cut tree walked
    on the device:

        minimize (or maximize=True: maximize)  c . x   subject to   A_ub x <= b_ub,   A_eq x = b_eq,   x >= 0,
        x[j] integer for j in integers,   x[j] in {0, 1} for j in binaries

    The operands -- shapes, broadcasting (an operand without the batch dimension is read with a batch stride of 0), strides,
    dtype, device -- the stream ("torch's current stream") and the loading rule ("torch first") are linprog_batch's.
    integers and binaries are HOST sequences of 0-based variable indices, or True for all variables, shared by the whole
    batch: binaries changes the tableau's height, and one call has one shape.  A variable named in both counts once.
    precision, max_pivots, check_cycles, tolerance and max_iterations are the reference's options, for the whole call.  The
    device reads no clock, so there is no timeout: it is the reference's default, +inf.

    Returns MilpBatchResult(x [B, n] float64, objective [B] float64, status [B] int32, nodes [B] int64, node_pivots [B]
    int64, root_pivots [B] int64) on the inputs' device: nodes is the number of branch-and-cut nodes the search consumed,
    node_pivots the sum of their pivots, root_pivots the root LP's.  status_names(status) spells the codes as solve() does;
    code 4 is "timedout" (max_iterations ran out with nodes left).

    The contract.  For finite data, row i is what solve() returns for the equivalent model -- linprog_batch's, plus
    "integers" / "binaries" naming those variables -- with includeZeroVariables read off the dense x: "optimal", and
    "timedout" with a solution, give the values of the best tableau (those not above precision are +0.0) and objective =
    solve()'s result; "unbounded" gives +0.0 but +inf at the unbounded variable and objective = +-inf; "infeasible",
    "cycled" and "timedout" without a solution give NaN everywhere.  For any data it is what the reference's `simplex`,
    `branchAndCut` and `solution` give on the tableau as built: tableauModel's -- linprog_batch's rows, then one row per
    binary variable in ascending index (column 0 and the variable's column 1.0), so width n + 1 and height
    1 + m_ub + 2 m_eq + len(binaries).

    With no integer variable at all solve() never enters branchAndCut, and neither does this call: x, objective, status and
    root_pivots are linprog_batch's x, objective, status and pivots bit for bit, and nodes = node_pivots = 0.

    What crosses PCIe per call: upwards the call's description, the two index lists and 152 bytes of descriptors per
    MILP; downwards one int32 per MILP per pass (a pass: the root LPs, the trees, and once more for those trees whose
    frontier or cycle history outgrew its first allocation and run again with four times the room).  A tree whose frontier
    outgrows the largest arena (65536 open nodes) cannot finish on the device: those rows, and only those, are gathered on
    the device, copied to the host and solved by the lockstep driver (_native.MilpBatch), and their x, objective, status and
    nodes are written into the output tensors; their node_pivots is -1, which that driver does not count.

    Raises TypeError / ValueError, before the library is touched, for what linprog_batch refuses, for a duplicate or an
    out-of-range index in integers or binaries, and for a largest possible node -- 8 (n + 1) (height + 2 n_integers) bytes,
    two cuts per integer variable -- above 4 MiB (solve() is the route for such models).  stats (a dict, optional) receives
    "launches", "reruns", "overflows", "kernels" and "gpu_ms" of the call (and "root_ms", "tree_ms", "epilogue_ms", its parts).

    Bounds.  lb, ub and upper are linprog_batch's: float64 device tensors [B, n] or [n] read through their strides, lb REPLACES
    x >= 0 (negative entries are legal), `upper` is a HOST sequence of the variables whose ub entry is read, or True, shared by
    the batch; values are taken as they lie.  Three rules come from the variables being integer, all decided on the host:
      1. the effective lower bound l_eff[j] is lb[j] at a continuous variable, ceil(lb[j]) at an integer one (x integer and
         x >= lb mean x >= ceil(lb); IEEE ceil: -0.5 gives -0.0, NaN and the infinities pass through) and +0.0 at a binary
         one, where lb is not read.  The substitution x = l_eff + x' keeps "x' integral <=> x integral", so the trees branch
         on x'.  Everything linprog_batch does with lb is done with l_eff: every right-hand side moves by shift_sum(row, l_eff)
         in linprog_batch's order of summation, a bound row holds ub[j] - l_eff[j], x = x' + l_eff and objective = objective' +
         shift_sum(c, l_eff).
      2. a binary variable has no bound row of its own and its ub is not read: upper=True means every variable that is not
         binary, and an explicit `upper` that names a binary variable raises ValueError.
      3. rows: linprog_batch's, then the k = len(upper) bound rows in ascending index, then the binary rows: height
         1 + m_ub + 2 m_eq + k + len(binaries), and the 4 MiB limit counts the bound rows.
    For finite data row i is solve() of the equivalent model in x' (linprog_batch's with the shifted right-hand sides, h<j>
    {"max": ub[j] - l_eff[j]}, "integers" / "binaries" as given), moved back.  With no integer and no binary variable x, objective,
    status and root_pivots are linprog_batch(..., lb=, ub=, upper=)'s bit for bit.  Without lb and ub the call launches the
    kernels it always launched and returns the same bits.  Nothing of size B x n is materialised.  Out of scope: free
    variables in this function -- milp_batch_free is this call with linprog_batch's `free` -- per-MILP sets, and duals (a node's duals are
    not the model's).

    See the module's docstring for the loading rule: torch first."""
    return _milp_call(c, A_ub, b_ub, A_eq, b_eq, (), **dict(lb=lb, ub=ub, upper=upper, integers=integers, binaries=binaries, maximize=maximize, precision=precision, max_pivots=max_pivots,
                           check_cycles=check_cycles, tolerance=tolerance, max_iterations=max_iterations, stats=stats))


def milp_batch_free(c, A_ub=None, b_ub=None, A_eq=None, b_eq=None, *, lb=None, ub=None, upper=True, free=(), integers=(), binaries=(),
                    maximize=False, precision=1e-8, max_pivots=8192, check_cycles=False, tolerance=0.0, max_iterations=32768, stats=None):
    """milp_batch with free variables (a function of its own: milp_batch keeps the argument list it has, as linprog_objective
    does beside linprog_objective_bounds).  Every argument but `free`, the result and the contract are milp_batch's; the
    messages of what is refused say "milp_batch".

    Free variables.  `free` is linprog_batch's: a HOST sequence of 0-based indices of the variables without a lower bound, or
    True, shared by the batch and checked like `integers` (TypeError / ValueError before the library is touched).  (), False
    and None mean none, and such a call is the call it was: the same kernels by name, the same bits.  The rules, all decided
    on the host:
      1. the split is linprog_batch's: x[j] = p[j] - q[j]; p keeps column 1 + j, the f = len(free) twins q are generated columns
         behind the n originals in ascending j, each cell the IEEE negation of the cell written at column 1 + j of that row (one
         strided read of the operand, not a second product), -1.0 in the bound row of a free variable `upper` lists, +0.0 in
         every other generated row, the binary rows included.  Width 1 + n + f.
      2. lb is not read at a free variable: l_eff[j] is +0.0 there, with no ceil, integer or not; the product with +0.0 is
         still formed and added in shift_sum, which runs over the n original columns only.  Everywhere else l_eff is rule 1 of
         the bounds.
      3. a binary variable cannot be free: free=True means every variable that is not binary, and an explicit `free` that names
         a binary variable raises ValueError, as `upper` does.
      4. a free integer variable has two integer columns: the trees are handed the n_int columns 1 + j in ascending j, then the
         twin columns of the free integer variables in ascending j (the whole list ascends), so that q is integral where p is.
         n_int_eff = n_int + |free & integers|, and the largest possible node is 8 (1 + n + f) (height + 2 n_int_eff) bytes:
         the 4 MiB refusal counts exactly that, and says so.
      5. the rows are unchanged: linprog_batch's, then the k bound rows, then the binary rows.
      6. x[j] of a free variable is read off the best tableau by linprog_batch's rule: "optimal" and "timedout" with a solution
         give v(p) - v(q), each v the rule above on its own column (basic and above precision: rounded; else +0.0), one
         subtraction, then + l_eff[j] where lb is given; "unbounded" gives +inf at the unbounded column, so -inf where that
         column is a twin; any other status NaN.  objective = objective' + shift_sum(c, l_eff), one addition.
    For finite data row i is solve() of the equivalent model in x', moved back: linprog_batch(free=)'s model -- one variable
    q<j> per free variable behind all x<j>, listing the negated coefficient of every constraint x<j> lists, and -c[j] -- with
    "integers" / "binaries" naming the variables, and "integers" naming the twins q<j> of the free integer variables too.  With
    no integer and no binary variable x, objective, status and root_pivots are linprog_batch(..., lb=, ub=, upper=, free=)'s
    bit for bit, and nodes = node_pivots = 0.  A call with free variables runs milp_dense_free_root_kernel and
    milp_dense_free_solution_kernel, with or without lb / ub; an overflowed tree of such a call is answered by the lockstep
    driver on the split tableau and moved back.  Nothing of size B x n or B x f is materialised.
    Hold a free integer variable by whole numbers: every row sees p and q as p - q, so where an LP leaves such a variable at a
    fraction v that the objective pushes against, the cut q >= ceil(-v) is answered by p rising with it, x stays at v, the next
    cut is on p, and the chain ends only at max_iterations ("timedout") -- in the reference's search as in this one.
    Out of scope: per-MILP sets, duals (a node's duals are not the model's), and inferring freeness from the data (an lb entry
    of -inf at a variable `free` does not list is taken as it lies in memory).

    See the module's docstring for the loading rule: torch first."""
    return _milp_call(c, A_ub, b_ub, A_eq, b_eq, free, **dict(lb=lb, ub=ub, upper=upper, integers=integers, binaries=binaries, maximize=maximize, precision=precision, max_pivots=max_pivots,
                           check_cycles=check_cycles, tolerance=tolerance, max_iterations=max_iterations, stats=stats))


def _milp_call(c, A_ub, b_ub, A_eq, b_eq, free, *, lb, ub, upper, integers, binaries, maximize, precision, max_pivots, check_cycles, tolerance,
               max_iterations, stats):
    """milp_batch and milp_batch_free behind their argument lists."""
    from . import milp_dense
    sets = {}

    def size(n, m_ub, m_eq):
        ints, bins = sets["ints"], sets["bins"] = milp_dense.integer_sets(n, integers, binaries)
        idx = sets["upper"] = milp_dense.bound_rows(_upper_set(n, upper, ub is not None, "milp_batch"), bins, upper is True)
        fidx = sets["free"] = milp_dense.free_set(_free_set(n, free, "milp_batch"), bins, free is True)
        twins = len(set(fidx) & set(ints))
        nbytes = milp_dense.largest_node_bytes(n, m_ub, m_eq, len(ints), len(bins), len(idx), len(fidx), twins)
        if fidx and nbytes > _native.MILPDENSE_MAX_BYTES:
            w, rows = n + 1 + len(fidx), 1 + m_ub + 2 * m_eq + len(idx) + len(bins)
            raise ValueError("milp_batch: the largest possible node, %d x %d doubles (%d bytes: %d twin columns of free variables, %d "
                             "rows and two cuts for each of %d integer columns -- %d integer variables and the twins of the %d free "
                             "ones among them), is above the batch limit of %d bytes; solve() is the route for such models"
                             % (nbytes // (8 * w), w, nbytes, len(fidx), rows, len(ints) + twins, len(ints), twins, _native.MILPDENSE_MAX_BYTES))
        if nbytes > _native.MILPDENSE_MAX_BYTES:
            raise ValueError("milp_batch: the largest possible node, %d x %d doubles (%d bytes: %d rows and two cuts for each of %d "
                             "integer variables), is above the batch limit of %d bytes; solve() is the route for such models"
                             % (nbytes // (8 * (n + 1)), n + 1, nbytes, 1 + m_ub + 2 * m_eq + len(idx) + len(bins), len(ints), _native.MILPDENSE_MAX_BYTES))

    B, n, m_ub, m_eq, device, operands, given, batched, bounds = _call_operands("milp_batch", c, A_ub, b_ub, A_eq, b_eq, size,
                                                                                vectors={"lb": lb, "ub": ub})
    ints, bins, idx, fidx = sets["ints"], sets["bins"], sets["upper"], sets["free"]
    more = {}
    if fidx:
        more["free"] = fidx
    if lb is not None or ub is not None:
        # (a bound tensor without an element -- n = 0 -- stays a descriptor, so that the call still is the bounded one)
        more.update(lb=None if lb is None else bounds["lb"] or (None, 0, 0, 0), ub=None if ub is None else bounds["ub"] or (None, 0, 0, 0),
                    upper=idx)
    out = MilpBatchResult(torch.empty((B, n), dtype=torch.float64, device=device), torch.empty((B,), dtype=torch.float64, device=device),
                          torch.empty((B,), dtype=torch.int32, device=device), *(torch.empty((B,), dtype=torch.int64, device=device) for _ in range(3)))
    ptr = lambda t: t.data_ptr() if t.numel() else None
    with torch.cuda.device(device), _lock:  # (the library selects the handle's device; torch's choice comes back afterwards)
        stream = torch.cuda.current_stream(device).cuda_stream or 1  # (the default stream's handle is 0: hipStreamLegacy names it)
        key = (device.index, stream)
        handle = _milp_handles.get(key)
        if handle is None:
            handle = _milp_handles[key] = _native.MilpDense(device.index, stream=stream)
        call = handle.solve(B, n, m_ub, m_eq, operands, integers=ints, binaries=bins, maximize=maximize, precision=precision,
                            max_pivots=max_pivots, check_cycles=check_cycles, tolerance=tolerance, max_iterations=max_iterations,
                            x=ptr(out.x), objective=ptr(out.objective), status=ptr(out.status), nodes=ptr(out.nodes),
                            node_pivots=ptr(out.node_pivots), root_pivots=ptr(out.root_pivots), **more)
        over = handle.overflowed() if call["overflows"] else []
        if stats is not None:
            info = handle.info()
            stats.update(launches=info["launches"], reruns=info["reruns"], overflows=len(over), kernels=info["kernels"],
                         gpu_ms=call["gpu_ms"], root_ms=call["root_ms"], tree_ms=call["tree_ms"], epilogue_ms=call["epilogue_ms"])
        if over:
            options = {"precision": float(precision), "maxPivots": float(max_pivots), "checkCycles": bool(check_cycles),
                       "tolerance": float(tolerance), "timeout": float("inf"), "maxIterations": float(max_iterations)}
            _solve_on_host(device, over, given, batched, B, ints, bins, bool(maximize), options, out, (lb, ub),
                           tuple(t is not None and t.dim() == 2 for t in (lb, ub)), idx, fidx)
    return out
