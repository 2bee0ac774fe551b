"""solve(model, options) -> Solution: the reference's public entry point
(/root/reference/src/YALPS.ts:8-92) with the dense-tableau simplex running on the MI355X.

Host side (model construction, branch and cut, result marshalling) mirrors the reference; the
hot path -- `simplex(tableau, options)`, src/simplex.ts:144 -- is libyalps_hip.so.  There is no
CPU fallback: without the HIP library and a gfx950 device `solve` raises.
"""
import math
import threading

from . import _native
from .branch_and_cut import branch_and_cut
from .model import apply_variant, tableau_model, tableau_model_with_bounds, variant_patch_cells

# src/YALPS.ts:52-60
_DEFAULTS = {
    "precision": 1e-8,
    "checkCycles": False,
    "maxPivots": 8192,
    "tolerance": 0,
    "timeout": math.inf,
    "maxIterations": 32768,
    "includeZeroVariables": False,
}

default_options = dict(_DEFAULTS)  # a copy, like the reference's exported `defaultOptions` (:65)

NODE_BATCH_MAX_BYTES = 4 << 20  # root tableaux above this size are never batched (see _solve_with)
SPARSE_MIN_BYTES = 128 << 10  # below this the dense tableau goes through the single-workgroup path (small_kernel), which
#                               reads it in place from pinned host memory: nothing to save by shipping cells


def round_to_precision(num, precision):
    """src/util.ts:1-4 with JS Math.round: halves toward +infinity, and a zero keeps the sign of its argument (-0 on
    [-0.5, -0]).  Divisions by zero give what IEEE gives, as in the reference: 1 / +-0 is +-infinity, and a rounding of 0
    (any precision above 2) makes the result 0 / 0 = NaN."""
    def js_round(x):
        if x != x or math.isinf(x):
            return x
        f = math.floor(x)
        r = f + 1.0 if x - f >= 0.5 else float(f)
        return math.copysign(0.0, x) if r == 0.0 else r
    if precision == 0:
        rounding = math.copysign(math.inf, precision)
    else:
        rounding = js_round(1.0 / precision)
    v = js_round((num + 2.220446049250313e-16) * rounding)
    if rounding == 0:
        return math.nan
    # precision 0: inf / inf (or NaN) divided in hardware, as the reference divides.  The NaN's bits are the ISA's default
    # NaN (x86-64: sign bit set, 0xfff8...; aarch64: 0x7ff8...), so they equal the reference's on the same ISA; the MILP
    # records (tests/golden/simplex_milp.json.gz) were made on x86-64.
    return v / rounding


def hip_simplex(tableau, options):
    """The drop-in for src/simplex.ts:144 `simplex(tableau, options)`: in place, through the C ABI
    (yalps_simplex_f64).  Returns (status, result).  A tableau built with sparse=True that has no
    dense matrix yet goes up as its written cells and only column 0 + the permutations come back
    (yalps_simplex_sparse_f64) -- all that solution() reads (src/YALPS.ts:18-19,32)."""
    if tableau.matrix is None:
        row, col, val = tableau.cells
        status, result, _, tableau.col0, tableau.position_of_variable, tableau.variable_at_position = \
            _native.simplex_sparse(tableau.width, tableau.height, row, col, val, precision=options["precision"],
                                   max_pivots=options["maxPivots"], check_cycles=options["checkCycles"])
        return status, result
    status, result, _ = _native.simplex_host(
        tableau.matrix, tableau.width, tableau.height, tableau.position_of_variable, tableau.variable_at_position,
        precision=options["precision"], max_pivots=options["maxPivots"], check_cycles=options["checkCycles"])
    return status, result


def solution(tabmod, status, result, options):
    """src/YALPS.ts:8-50"""
    tableau, sign, vars_ = tabmod.tableau, tabmod.sign, tabmod.variables
    precision = options["precision"]
    if status == "optimal" or (status == "timedout" and not math.isnan(result)):
        variables = []
        for i, (key, _) in enumerate(vars_):
            row = int(tableau.position_of_variable[i + 1]) - tableau.width
            value = tableau.rhs(row) if row >= 0 else 0.0
            if value > precision:
                variables.append((key, round_to_precision(value, precision)))
            elif options["includeZeroVariables"]:
                variables.append((key, 0.0))
        return {"status": status, "result": -sign * result, "variables": variables}
    if status == "unbounded":
        variable = int(tableau.variable_at_position[int(result)]) - 1
        return {"status": "unbounded", "result": sign * math.inf,
                "variables": [(vars_[variable][0], math.inf)] if 0 <= variable < len(vars_) else []}
    return {"status": status, "result": math.nan, "variables": []}  # infeasible | cycled | timedout w/o result


def _milp_on_device(tabmod, opt, stats=None):
    """A MILP whose root tableau is too big for the single-workgroup path: the root is assembled (sparse) or
    uploaded once, solved and KEPT in HBM; branch and cut builds every node next to it on the device
    (branch_and_cut_device).  No tableau ever comes back to the host."""
    from .branch_and_cut import branch_and_cut_device
    from .model import Tableau, TableauModel
    t = tabmod.tableau
    ctx = _native.Context(0)
    root = _native.DeviceTableau(ctx, t.width, t.height)
    node = None
    try:
        if t.matrix is None:
            root.assemble(t.height, *t.cells)
        else:
            root.upload(t.matrix, t.height, t.position_of_variable, t.variable_at_position)
        status, result, _, _ = root.solve(opt["precision"], opt["maxPivots"], opt["checkCycles"])
        col0, pos, var = root.download_solution()
        view = TableauModel(Tableau(None, t.width, t.height, pos, var, col0), tabmod.sign,
                            tabmod.variables, tabmod.integers)
        if status != "optimal":
            return solution(view, status, result, opt)
        node = _native.DeviceTableau(ctx, t.width, t.height + 2 * len(tabmod.integers))
        int_tabmod, int_status, int_result = branch_and_cut_device(view, root, node, result, opt, stats)
        return solution(int_tabmod, int_status, int_result, opt)
    finally:
        if node is not None:
            node.close()
        root.close()
        ctx.close()


def _milp_native(tabmod, opt, node_batch=0, stats=None):
    """A model with integers through yalps_milp_f64: root simplex and the whole branch and cut (the reference's
    queue order, every node LP on the GPU) in ONE native call; only what solution() reads comes back."""
    from .model import Tableau, TableauModel
    t = tabmod.tableau
    status, result, height, col0, pos, var, st = _native.milp(
        t.dense(), t.width, t.height, t.position_of_variable, t.variable_at_position, tabmod.integers, tabmod.sign,
        precision=opt["precision"], max_pivots=opt["maxPivots"], check_cycles=opt["checkCycles"], tolerance=opt["tolerance"],
        timeout=opt["timeout"], max_iterations=opt["maxIterations"], node_batch=node_batch)
    if stats is not None:
        stats.update(st)
    view = TableauModel(Tableau(None, t.width, height, pos, var, col0), tabmod.sign, tabmod.variables, tabmod.integers)
    return solution(view, status, result, opt)


def _solve_with(simplex, model, options=None, node_batch=0, stats=None, sparse=False, device_nodes=False, native=False):
    """src/YALPS.ts:73-92 with the simplex backend as a parameter (tests drive the host logic
    with the CPU oracle through this; the product binds the HIP backend below)."""
    tabmod = tableau_model(model, sparse=sparse)
    opt = dict(_DEFAULTS)
    if options:
        opt.update({k: v for k, v in options.items() if v is not None})
    nbytes = 8 * tabmod.tableau.width * tabmod.tableau.height
    if native and tabmod.integers:
        return _milp_native(tabmod, opt, node_batch, stats)
    if device_nodes and tabmod.integers and nbytes > SPARSE_MIN_BYTES and not (node_batch > 1 and nbytes <= NODE_BATCH_MAX_BYTES):
        return _milp_on_device(tabmod, opt, stats)
    if sparse and (tabmod.integers or nbytes <= SPARSE_MIN_BYTES):
        tabmod.tableau.dense()  # branch and cut reads the whole root matrix (src/branchAndCut.ts:28,38-41)
    status, result = simplex(tabmod.tableau, opt)
    if not tabmod.integers or status != "optimal":
        return solution(tabmod, status, result, opt)
    # one workgroup per node only pays while a node's tableau is small (it streams through one CU);
    # large roots (Vendor Selection: 23 MB) are better off on the whole-chip kernels, one node at a time
    small = 8 * tabmod.tableau.width * tabmod.tableau.height <= NODE_BATCH_MAX_BYTES
    if node_batch > 1 and not opt["checkCycles"] and small:
        from .branch_and_cut import branch_and_cut_batched
        int_tabmod, int_status, int_result = branch_and_cut_batched(tabmod, result, opt, node_batch, stats)
    else:
        int_tabmod, int_status, int_result = branch_and_cut(simplex, tabmod, result, opt)
    return solution(int_tabmod, int_status, int_result, opt)


def solve(model, options=None, node_batch=None, stats=None, sparse=True, device_nodes=True, native=True):
    """Runs the solver on `model` (see yalps_amd.model) with `options` (keys as in the reference's
    `Options`, src/types.ts:203-265).  Returns {"status", "result", "variables": [(key, value)]}.

    node_batch > 1: branch and cut evaluates that many frontier nodes per GPU batch (speculatively,
    best first; results are committed in the reference's pop order, so the outcome is the same as
    node_batch = 0, which re-solves one node at a time).  Default: 32 with the native driver
    (Large Farm MIP: 120 ms one node at a time, 28 ms in batches of 32), 0 with the Python drivers.

    sparse: a model without integer variables is shipped as the cells tableauModel writes and its
    tableau is assembled in HBM (same tableau, same pivots, 16 B per cell over PCIe instead of
    8*width*height); False = always the dense host tableau.

    device_nodes: a MILP whose root tableau exceeds the single-workgroup size keeps it in HBM and builds
    every branch-and-cut node there (yalps_tableau_apply_cuts); False = the reference's flow, every node
    through the host-array drop-in call.

    native: a model with integers is handed to yalps_milp_f64 -- root simplex and the whole branch and cut in
    one native call (same queue order, same node LPs); False = the Python drivers of branch_and_cut.py."""
    if node_batch is None:
        node_batch = 32 if native else 0
    return _solve_with(hip_simplex, model, options, node_batch, stats, sparse, device_nodes, native)


_lpbatch = None  # the process's LpBatch: stream, events and device buffers are kept and grown between solve_many calls
_lpbatch_lock = threading.Lock()  # (a handle belongs to one thread at a time)


def lpbatch_simplex(tableaux, options, stats=None):
    """The batched backend of solve_many: every tableau (built with sparse=True, no dense matrix) through ONE
    yalps_lpbatch_solve; column 0 and the permutations land in the tableaux as hip_simplex leaves them.
    Returns [(status, result)]."""
    global _lpbatch
    with _lpbatch_lock:
        if _lpbatch is None:
            _lpbatch = _native.LpBatch(0)
        batch = _lpbatch
        statuses, results, _, _ = batch.solve(
            [(t.width, t.height, *t.cells, o["precision"], o["maxPivots"], o["checkCycles"]) for t, o in zip(tableaux, options)])
        for i, t in enumerate(tableaux):
            t.col0, t.position_of_variable, t.variable_at_position = batch.solution(i)
        if stats is not None:
            info = batch.info()
            stats.update(launches=info["launches"], reruns=info["reruns"], kernels=info["kernels"])
    return [(s, float(r)) for s, r in zip(statuses, results)]


_milpbatch = None  # the process's MilpBatch, kept like _lpbatch
MILP_NODE_BATCH = 8  # nodes a tree asks for per round in solve_many (see milpbatch_solve)


def milpbatch_solve(items, stats=None, node_batch=None):
    """The batched MILP backend of solve_many: items = [(tabmod, options)] (tableaux built with sparse=True) through ONE
    yalps_milpbatch_solve -- a root pass, then rounds in which the nodes all unfinished trees want share their launches.
    Returns per model (status, result, height, col0, positionOfVariable, variableAtPosition) of its best tableau.

    node_batch (default MILP_NODE_BATCH): the node a tree popped plus its next-best node_batch - 1 frontier nodes per round.
    The value rests on the "node_batch_sweep" table of profiles/milp_batch_throughput.json (the mixed workload of 2944
    trees): throughput rises steeply from 1 to 8 and is flat from 8 to 32, where repeated runs of the table order 8, 16 and
    32 differently (within 6 % of each other); 8 is the smallest value on the plateau and evaluates the fewest nodes that
    are never used."""
    global _milpbatch
    with _lpbatch_lock:
        if _milpbatch is None:
            _milpbatch = _native.MilpBatch(0)
        batch = _milpbatch
        packed = _native.PackedMilps([(tm.tableau.width, tm.tableau.height, *tm.tableau.cells, tm.integers, tm.sign, o)
                                      for tm, o in items])
        statuses, results, used, evaluated, call = batch.solve(packed, node_batch or MILP_NODE_BATCH)
        out = [(s, float(r), *batch.solution(i)) for i, (s, r) in enumerate(zip(statuses, results))]
    if stats is not None:
        stats.update(node_rounds=call["rounds"], nodes_evaluated=int(evaluated.sum()), nodes_used=int(used.sum()),
                     milp_launches=call["launches"])
    return out


_milptree = None  # the process's MilpTree, kept like _lpbatch


def milptree_solve(items, stats=None, fallback=None, make=None):
    """The device-search MILP backend of solve_many(milp_search="device"): items = [(tabmod, options)] through ONE
    yalps_milptree_solve -- a root pass, then every tree walked to its end by one workgroup (milp_tree_kernel), no rounds.
    Returns what milpbatch_solve returns.  A tree whose frontier outgrew the largest arena comes back "overflow": those go
    through `fallback` (milpbatch_solve) together and their answers are spliced in.  make: () -> the MilpTree to use (tests)."""
    global _milptree
    with _lpbatch_lock:
        if make is not None:
            batch = make()
        else:
            if _milptree is None:
                _milptree = _native.MilpTree(0)
            batch = _milptree
        packed = _native.PackedMilps([(tm.tableau.width, tm.tableau.height, *tm.tableau.cells, tm.integers, tm.sign, o)
                                      for tm, o in items])
        statuses, results, used, _, call = batch.solve(packed)
        out = [(s, float(r), *batch.solution(i)) for i, (s, r) in enumerate(zip(statuses, results))]
        info = batch.info()
    over = [i for i, s in enumerate(statuses) if s == "overflow"]
    more = {}
    if over:
        for i, o in zip(over, (fallback or milpbatch_solve)([items[i] for i in over], more)):
            out[i] = o
    if stats is not None:
        walked = sum(int(u) for s, u in zip(statuses, used) if s != "overflow")
        stats.update(tree_launches=call["launches"], tree_reruns=info["reruns"], tree_overflows=len(over),
                     nodes_used=walked + more.get("nodes_used", 0))
    return out


def milp_batchable(tabmod, opt):
    """A model with integers joins the MILP batch when its largest possible node (2 cuts per integer variable) is within
    4 MiB and its timeout is infinite or <= 0: a finite positive timeout keeps solve(), whose clock counts that model alone."""
    t = tabmod.tableau
    timeout = opt["timeout"]
    return (bool(tabmod.integers) and 8 * t.width * (t.height + 2 * len(tabmod.integers)) <= _native.MILPBATCH_MAX_BYTES
            and (timeout == math.inf or timeout <= 0))


def _solve_many_with(batch_simplex, solve_one, models, options=None, stats=None, milp_backend=None):
    """solve_many with its backends as parameters (tests drive the routing and the marshalling with the CPU oracle):
    batch_simplex(tableaux, options, stats) -> [(status, result)] for the models without integers whose tableau is at most
    NODE_BATCH_MAX_BYTES, solve_one(model, options) for every other model (integers, larger LPs), results in input order.
    milp_backend(items, stats) (None: no MILP batch, every model with integers goes to solve_one) takes the models with
    integers that milp_batchable accepts, as [(tabmod, options)], and returns each one's best tableau (milpbatch_solve)."""
    from .model import Tableau, TableauModel
    models = list(models)
    opts = list(options) if isinstance(options, (list, tuple)) else [options] * len(models)
    if len(opts) != len(models):
        raise ValueError("solve_many: %d models but %d option sets" % (len(models), len(opts)))
    out = [None] * len(models)
    batched = []  # (index, tabmod, merged options)
    milps = []
    routed = {"batched": 0, "milp": 0, "large": 0}
    for i, (model, o) in enumerate(zip(models, opts)):
        tabmod = tableau_model(model, sparse=True)
        t = tabmod.tableau
        opt = dict(_DEFAULTS)
        if o:
            opt.update({k: v for k, v in o.items() if v is not None})
        if milp_backend is not None and milp_batchable(tabmod, opt):
            routed["milp"] += 1
            milps.append((i, tabmod, opt))
            continue
        if tabmod.integers or 8 * t.width * t.height > NODE_BATCH_MAX_BYTES:
            routed["milp" if tabmod.integers else "large"] += 1
            out[i] = solve_one(model, o)
            continue
        batched.append((i, tabmod, opt))
    routed["batched"] = len(batched)
    if milp_backend is not None:
        routed.update(milp_batched=len(milps), node_rounds=0, nodes_evaluated=0, nodes_used=0)
    if stats is not None:
        stats.update(routed)
    if batched:
        results = batch_simplex([b[1].tableau for b in batched], [b[2] for b in batched], stats)
        for (i, tabmod, opt), (status, result) in zip(batched, results):
            out[i] = solution(tabmod, status, result, opt)
    if milps:
        results = milp_backend([(m[1], m[2]) for m in milps], stats)
        for (i, tabmod, opt), (status, result, height, col0, pos, var) in zip(milps, results):
            view = TableauModel(Tableau(None, tabmod.tableau.width, height, pos, var, col0), tabmod.sign, tabmod.variables,
                                tabmod.integers)
            out[i] = solution(view, status, result, opt)
    return out


def solve_many(models, options=None, stats=None, milp_search="host"):
    """[solve(m, o) for m, o in zip(models, options)] -- same dicts, same order -- in at most two batched GPU calls plus
    solve() for what fits neither.  `options` is one dict for all models or one per model.

    Models without integer variables and a tableau of at most 4 MiB: ONE yalps_lpbatch_solve, one workgroup per LP.
    Models with integer variables whose largest possible node (8 * width * (height + 2 * n_integers) bytes) is within 4 MiB:
    ONE yalps_milpbatch_solve -- every root in a root pass, then all branch-and-cut trees advance together, the nodes they
    want next sharing launches round by round; each tree's node sequence, best tableau and result are what solve() gives
    for it alone.  The clock: only a timeout of +inf, or <= 0 (timed out before the first node, deterministic), is batched;
    a model with a finite positive timeout goes through solve(), whose clock counts that model's own work.
    Everything else (larger LPs, larger MILPs) goes through solve() one by one.

    stats (a dict, optional) receives how many models went which way ("batched" LPs, "milp" = every model with integers,
    "milp_batched" of them in the MILP batch, "large"), the LP batch's launches, and "node_rounds", "nodes_evaluated",
    "nodes_used" of the MILP batch.

    milp_search="device" sends the MILP batch through yalps_milptree_solve instead (milptree_solve: the search loop runs
    inside the kernel, one workgroup per tree; same routing, same answers; stats then has "tree_launches", "tree_reruns",
    "tree_overflows" and "nodes_used").  "host", the default, is the lockstep driver above."""
    if milp_search == "host":
        return _solve_many_with(lpbatch_simplex, solve, models, options, stats, milpbatch_solve)
    if milp_search != "device":
        raise ValueError("solve_many: milp_search must be \"host\" or \"device\", not %r" % (milp_search,))
    return _solve_many_with(lpbatch_simplex, solve, models, options, stats, milptree_solve)


_lpvariants = None  # the process's LpVariants, kept like _lpbatch


def lpvariants_simplex(tableau, patches, options, stats=None):
    """The patched backend of solve_variants: the base tableau (built with sparse=True) and every variant's patch -- sorted
    [(flat index, value)] -- through ONE yalps_lpvar_solve.  Returns per variant (status, result, col0, positionOfVariable,
    variableAtPosition)."""
    import numpy as np
    global _lpvariants
    w = tableau.width
    offsets = np.zeros(len(patches) + 1, np.int64)
    np.cumsum([len(p) for p in patches], out=offsets[1:])
    total = int(offsets[-1])
    idx = np.fromiter((k for p in patches for k, _ in p), np.int64, total)
    val = np.fromiter((v for p in patches for _, v in p), np.float64, total)
    packed = _native.PackedVariants(w, tableau.height, *tableau.cells, patches,
                                    [(o["precision"], o["maxPivots"], o["checkCycles"]) for o in options],
                                    flat=(offsets, idx // w, idx % w, val))
    with _lpbatch_lock:
        if _lpvariants is None:
            _lpvariants = _native.LpVariants(0)
        lv = _lpvariants
        statuses, results, _, _ = lv.solve(packed)
        out = [(s, float(r), *lv.solution(i)) for i, (s, r) in enumerate(zip(statuses, results))]
        if stats is not None:
            info = lv.info()
            stats.update(launches=info["launches"], reruns=info["reruns"], kernels=info["kernels"])
    return out


def _solve_variants_with(variants_backend, solve_many_fn, model, variants, options=None, stats=None):
    """solve_variants with its backends as parameters (tests drive the routing and the marshalling with the CPU oracle):
    variants_backend(tableau, patches, options, stats) -> per variant (status, result, col0, pos, var) for the variants that
    only patch the base tableau, solve_many_fn(models, options, stats) for the variants materialised with apply_variant
    (a base with integers or above NODE_BATCH_MAX_BYTES, a variant that changes the structure); results in input order."""
    from .model import Tableau, TableauModel
    variants = list(variants)
    opts = list(options) if isinstance(options, (list, tuple)) else [options] * len(variants)
    if len(opts) != len(variants):
        raise ValueError("solve_variants: %d variants but %d option sets" % (len(variants), len(opts)))
    tabmod, bounds_info = tableau_model_with_bounds(model, sparse=True)
    t = tabmod.tableau
    patchable = not tabmod.integers and 8 * t.width * t.height <= NODE_BATCH_MAX_BYTES
    out = [None] * len(variants)
    patched, materialised = [], []  # (index, patch, merged options) | (index, model, options as given)
    for i, (v, o) in enumerate(zip(variants, opts)):
        patch = variant_patch_cells(tabmod, bounds_info, v) if patchable else None
        if patch is None:
            materialised.append((i, apply_variant(model, v), o))
            continue
        opt = dict(_DEFAULTS)
        if o:
            opt.update({k: x for k, x in o.items() if x is not None})
        patched.append((i, patch, opt))
    if stats is not None:
        stats.update(patched=len(patched), materialised=len(materialised), base_cells=int(t.cells[0].size),
                     patch_cells=sum(len(p[1]) for p in patched), launches=0, reruns=0, kernels=[])
    if patched:
        results = variants_backend(t, [p[1] for p in patched], [p[2] for p in patched], stats)
        for (i, _, opt), (status, result, col0, pos, var) in zip(patched, results):
            view = TableauModel(Tableau(None, t.width, t.height, pos, var, col0), tabmod.sign, tabmod.variables, tabmod.integers)
            out[i] = solution(view, status, result, opt)
    if materialised:
        sub = {} if stats is not None else None
        results = solve_many_fn([m[1] for m in materialised], [m[2] for m in materialised], sub)
        for (i, _, _), r in zip(materialised, results):
            out[i] = r
        if stats is not None:
            stats["solve_many"] = sub
    return out


def solve_variants(model, variants, options=None, stats=None):
    """[solve(apply_variant(model, v), o) for v, o in zip(variants, options)] -- same dicts, same order -- for many variants
    of ONE model: other bounds, other objective and constraint coefficients of existing variables (yalps_amd.model.apply_variant
    says what a variant is).  `options` is one dict for all variants or one per variant.

    The model is walked once.  Where it has no integer variables and its tableau is at most 4 MiB, a variant that keeps the
    tableau's structure costs only its patch -- the handful of cells it changes -- on the host and over PCIe, and all such
    variants go through ONE yalps_lpvar_solve: the base is assembled once on the device and every variant starts from a copy
    of it.  Every other variant (a base with integers, a larger base, a replaced constraint with other finite sides) is
    materialised with apply_variant and handed to solve_many in one call; nothing is refused that solve would accept.

    stats (a dict, optional) receives "patched" and "materialised" (variants that went each way), "base_cells",
    "patch_cells" (all patches together), "launches", "reruns" and "kernels" of the native call, and under "solve_many" the
    stats of the materialised variants' call."""
    return _solve_variants_with(lpvariants_simplex, solve_many, model, variants, options, stats)


_lpwarm = None  # the process's LpWarm, kept like _lpbatch


def lpwarm_simplex(tableau, base_options, patches, options, stats=None):
    """The warm backend of reoptimize_variants: the base tableau (built with sparse=True) with the options of its own solve,
    and every variant's patch -- sorted [(flat index, value)], cells of row 0 and column 0 of the initial tableau -- through
    ONE yalps_lpwarm_solve.  Returns ((status, result, pivots) of the base, per variant (status, result, pivots, col0,
    positionOfVariable, variableAtPosition)), the second None where the base did not end optimal."""
    import numpy as np
    global _lpwarm
    w = tableau.width
    offsets = np.zeros(len(patches) + 1, np.int64)
    np.cumsum([len(p) for p in patches], out=offsets[1:])
    total = int(offsets[-1])
    idx = np.fromiter((k for p in patches for k, _ in p), np.int64, total)
    val = np.fromiter((v for p in patches for _, v in p), np.float64, total)
    b = base_options
    packed = _native.PackedWarm(w, tableau.height, *tableau.cells, patches,
                                [(o["precision"], o["maxPivots"], o["checkCycles"]) for o in options],
                                flat=(offsets, idx // w, idx % w, val),
                                base_options=(b["precision"], b["maxPivots"], b["checkCycles"]))
    with _lpbatch_lock:
        if _lpwarm is None:
            _lpwarm = _native.LpWarm(0)
        lw = _lpwarm
        ran = lw.solve(packed)
        out = None
        if ran is not None:
            statuses, results, pivots, _ = ran
            out = [(s, float(r), int(p), *lw.solution(i)) for i, (s, r, p) in enumerate(zip(statuses, results, pivots))]
        if stats is not None:
            info = lw.info()
            stats.update(launches=info["launches"], reruns=info["reruns"], kernels=info["kernels"])
    return lw.base, out


def _reoptimize_variants_with(warm_backend, cold_fn, model, variants, options=None, base_options=None, stats=None):
    """reoptimize_variants with its backends as parameters (tests drive the routing and the marshalling with the CPU oracle):
    warm_backend(tableau, base options, patches, options, stats) -> ((status, result, pivots) of the base, per variant
    (status, result, pivots, col0, pos, var) or None where the base is not optimal) for the variants that move only bounds
    and objective coefficients, cold_fn(model, variants, options, stats) -- solve_variants -- for everything else; results
    in input order."""
    from .model import Tableau, TableauModel
    variants = list(variants)
    opts = list(options) if isinstance(options, (list, tuple)) else [options] * len(variants)
    if len(opts) != len(variants):
        raise ValueError("reoptimize_variants: %d variants but %d option sets" % (len(variants), len(opts)))
    if stats is not None:
        stats.update(warm=0, cold=len(variants), base_status=None, base_pivots=0, pivots=[], launches=0, reruns=0, kernels=[])

    def all_cold():
        sub = {} if stats is not None else None
        out = cold_fn(model, variants, options, sub)
        if stats is not None:
            stats["solve_variants"] = sub
        return out

    tabmod, bounds_info = tableau_model_with_bounds(model, sparse=True)
    t = tabmod.tableau
    if tabmod.integers or 8 * t.width * t.height > NODE_BATCH_MAX_BYTES:
        return all_cold()
    w = t.width
    row, col, val = t.cells
    edge = (row == 0) | (col == 0)
    base0 = dict(zip((row[edge].astype("int64") * w + col[edge]).tolist(), val[edge].tolist()))  # row 0 and column 0 of the initial tableau
    warm, cold = [], []  # (index, patch without the cells that do not move, merged options) | index
    for i, (v, o) in enumerate(zip(variants, opts)):
        patch = variant_patch_cells(tabmod, bounds_info, v)
        if patch is None or any(k >= w and k % w for k, _ in patch):
            cold.append(i)  # another structure | a cell in the body of the tableau
            continue
        deltas = [x - base0.get(k, 0.0) for k, x in patch]
        if not all(math.isfinite(d) for d in deltas):
            cold.append(i)
            continue
        opt = dict(_DEFAULTS)
        if o:
            opt.update({k: x for k, x in o.items() if x is not None})
        warm.append((i, [cell for cell, d in zip(patch, deltas) if d != 0.0], opt))
    if not warm:
        return all_cold()
    base_opt = dict(_DEFAULTS)
    if base_options:
        base_opt.update({k: x for k, x in base_options.items() if x is not None})
    base, results = warm_backend(t, base_opt, [p[1] for p in warm], [p[2] for p in warm], stats)
    if stats is not None:
        stats.update(base_status=base[0], base_pivots=int(base[2]))
    if base[0] != "optimal" or results is None:
        return all_cold()
    out = [None] * len(variants)
    for (i, _, opt), (status, result, pivots, col0, pos, var) in zip(warm, results):
        view = TableauModel(Tableau(None, t.width, t.height, pos, var, col0), tabmod.sign, tabmod.variables, tabmod.integers)
        out[i] = solution(view, status, result, opt)
    if stats is not None:
        stats.update(warm=len(warm), cold=len(cold), pivots=[int(r[2]) for r in results])
    if cold:
        sub = {} if stats is not None else None
        for i, r in zip(cold, cold_fn(model, [variants[i] for i in cold], [opts[i] for i in cold], sub)):
            out[i] = r
        if stats is not None:
            stats["solve_variants"] = sub
    return out


def reoptimize_variants(model, variants, options=None, base_options=None, stats=None):
    """Many variants of ONE model, each REOPTIMISED from the optimal tableau of the model itself: the same list of dicts as
    solve_variants, in input order, for scenario analysis, parametric sweeps and pricing loops in which a variant moves
    bounds and objective coefficients.  `options` is one dict for all variants or one per variant; `base_options` are the
    options of the one solve of `model` itself (default: the defaults).

    The contract is NOT solve_variants'.  A variant that moves only right-hand sides and objective coefficients leaves the
    body of the base's optimal tableau valid and changes only its column 0 and its row 0; each answer is what `simplex`
    returns when started from that updated tableau with the base's basis (phase 1 repairs a right-hand side that went
    negative, phase 2 continues, as after every branch-and-cut node's cuts).  It is a valid answer for the variant's LP --
    the same status wherever the LP has one answer, the objective equal under the reference's validator -- but not
    necessarily the dict solve() gives: where the LP has several optimal vertices another one is possible.  maxPivots and
    checkCycles count the reoptimisation's pivots alone, so a budget that ends solve() early may not end this at all, and one
    that ends it leaves another tableau.  The reference's phase 1 makes no promise from an arbitrary basis: after large moves
    (bounds of a 300 x 280 dense LP by +-50 %: 20 of 256 variants, README) it can run into maxPivots and end "cycled" where
    a solve from the initial tableau ends "optimal".  That answer is handed back as it is; solve_variants is the call for such
    variants.

    Routing, on the host in one pass.  The whole call goes to solve_variants, with the same arguments, where the base has
    integer variables, a tableau above 4 MiB, or does not end "optimal".  A single variant goes there (all such variants in
    one call) where it changes the tableau's structure (variant_patch_cells gives None), changes a constraint coefficient
    (a cell with row > 0 and col > 0), or moves a cell by something that is not finite.  Everything else goes through ONE
    yalps_lpwarm_solve: the base is solved once on the device, and every variant starts from a copy of its final tableau
    with a few records folded into column 0 and row 0.  Cells whose value does not differ from the base's are dropped.

    stats (a dict, optional) receives "warm" and "cold" (variants that went each way), "base_status" and "base_pivots",
    "pivots" (per warm variant, in input order), "launches", "reruns" and "kernels" of the native call, and under
    "solve_variants" the stats of the cold call."""
    return _reoptimize_variants_with(lpwarm_simplex, solve_variants, model, variants, options, base_options, stats)


# sensitivity(model, options) / sensitivity_many(models, options, stats): solve()'s answer plus duals, reduced costs and ranges
from .sensitivity import _sensitivity_many_with, sensitivity, sensitivity_many  # noqa: E402,F401
