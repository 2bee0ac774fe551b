"""Helpers of tests/test_milp_tree.py (TEST INFRASTRUCTURE): the host search of libyalps_milptree.so driven with the C oracle or
with a synthetic evaluator, a Python restatement of the rules of yalps_amd/csrc/milp_tree_rules.cuh with one switch per
decision site, and the shapes of the GPU tests."""
import hashlib
import math
import struct

import numpy as np

from tests import _batch_shapes as BS
from tests import _bnc as B
from tests import _lp_batch as LB
from tests import _milp_batch as MB
from tests import _milps as ML

NAN, INF = math.nan, math.inf
MUTANTS = ("siftup_left_on_ties", "push_lower_first", "mfv_inclusive", "new_cut_first")


def bits(x):
    return "nan" if math.isnan(x) else B.hexd(x)


def run_tree_search(nat, oracle, roots, arena=None, arena_max=None):
    """nat.milp_tree_search over `roots` (MB.Root) with the oracle as evaluator, shaped as MB.run_search's answer."""
    ev = MB.OracleEvaluator(oracle, roots)
    consumed = [[] for _ in roots]
    out, reruns = nat.milp_tree_search([r.packed() for r in roots], ev, arena=arena, arena_max=arena_max,
                                       consumed=lambda m, e, cuts: consumed[m].append((e, cuts)))
    nodes = [[dict(ev.log.get(ev.key(m, cuts), {"cuts": "never evaluated"}), eval=B.hexd(e)) for e, cuts in seq]
             for m, seq in enumerate(consumed)]
    return out, nodes, ev, reruns


# ---------------------------------------------------------------------------------------------- a synthetic evaluator

def _hash(*parts):
    h = hashlib.sha256(repr(parts).encode()).digest()
    return struct.unpack("<4Q", h)


class Synthetic:
    """Roots and node results that are a fixed hash of (tree seed, cut list): many equal results and evaluations, -0.0 results,
    infeasible and cycled nodes, integer variables that are basic or not.  `p_frac` steers the size of the trees."""
    RESULTS = (-0.0, 0.0, 1.0, 1.0, 1.5, 2.0, 2.0, 2.0, 3.0, -1.0)
    VALUES = (0.0, 1.0, 2.0, 0.5, 1.5, 2.5, 0.25, 3.75, -0.5, -0.0)

    def __init__(self, seed, n_int, p_frac=0.45, root_status="optimal", root_result=None, opt=None, sign=1.0):
        self.seed, self.n_int, self.p_frac = seed, n_int, p_frac
        self.w, self.h = n_int + 3, n_int + 2
        self.ints = list(range(1, n_int + 1))
        self.opt = MB.options(opt)
        self.sign = sign
        self.status = root_status
        self.result = self.RESULTS[_hash(seed, "r")[0] % len(self.RESULTS)] if root_result is None else root_result
        self.col0, self.pos, self.var = self.node_view(())

    def node_view(self, key, integral=False):
        """column 0 and the permutations of the node with cut list `key`: integer variable j basic in row j + 1 (or, every fifth,
        non-basic), its value a hash of the key."""
        h = self.h + len(key)
        x = _hash(self.seed, key, "v")
        col0 = np.zeros(h)
        for j in range(h):
            v = self.VALUES[(x[j % 4] >> (4 * (j // 4 % 12))) % len(self.VALUES)]
            col0[j] = float(round(v)) if integral else v
        n = self.w + h
        pos, var = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
        for k, v in enumerate(self.ints):
            if (x[3] >> k) % 5 != 0 and k + 1 < self.h:  # basic in row k + 1: swap with the slack there
                q = self.w + k + 1
                pos[v], pos[q] = q, v
                var[v], var[q] = q, v
        return col0, pos, var

    def packed(self):
        return (self.w, self.h, self.status, self.result, self.col0, self.pos, self.var, self.ints, self.sign, self.opt)

    def node(self, cuts):
        key = tuple((int(s), int(v), B.hexd(x)) for s, v, x in cuts)
        x = _hash(self.seed, key, "s")
        u = (x[0] % 10000) / 10000.0
        res = self.RESULTS[x[1] % len(self.RESULTS)]
        if u < self.p_frac:
            return ("optimal", res, *self.node_view(key))
        if u < self.p_frac + 0.2:
            return ("optimal", res, *self.node_view(key, integral=True))
        if u < self.p_frac + 0.3:
            return ("cycled", NAN, None, None, None)
        return ("infeasible", NAN, None, None, None)


def synthetic_evaluator(trees, log=None):
    def evaluate(nodes):
        out = []
        for m, cuts in nodes:
            if log is not None:
                log.append((m, tuple((int(s), int(v), B.hexd(x)) for s, v, x in cuts)))
            st, res, c0, p, v = trees[m].node(cuts)
            out.append((st, res, c0 if c0 is not None else [], p if p is not None else [], v if v is not None else []))
        return out
    return evaluate


def synthetic_trees(count, seed0=0, **kw):
    rng = np.random.RandomState(seed0)
    return [Synthetic(seed0 * 100000 + k, int(rng.randint(1, 13)), **kw) for k in range(count)]


def same_outputs(a, b):
    """Two drivers' per-model tuples: status, result bits, height, column 0 and permutations bit for bit, nodes used."""
    if len(a) != len(b):
        return "count"
    for i, (x, y) in enumerate(zip(a, b)):
        if (x[0], bits(x[1]), x[2], x[6]) != (y[0], bits(y[1]), y[2], y[6]):
            return "model %d: %r != %r" % (i, (x[0], x[1], x[2], x[6]), (y[0], y[1], y[2], y[6]))
        if not (MB.same_words(x[3], y[3]) and np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5])):
            return "model %d: best tableau" % i
    return None


def both_drivers(nat, trees, arena=None, arena_max=None):
    """(tree search, lockstep at node_batch 1) over synthetic trees: outputs and consumed sequences of each."""
    runs = []
    for which in ("tree", "lockstep"):
        seq = []
        consumed = lambda m, e, cuts: seq.append((m, B.hexd(e), tuple((int(s), int(v), B.hexd(x)) for s, v, x in cuts)))
        roots = [t.packed() for t in trees]
        if which == "tree":
            out, _ = nat.milp_tree_search(roots, synthetic_evaluator(trees), arena=arena, arena_max=arena_max, consumed=consumed)
        else:
            out, _ = nat.milp_search(roots, synthetic_evaluator(trees), node_batch=1, consumed=consumed)
        per = [[] for _ in trees]
        for m, e, cuts in seq:
            per[m].append((e, cuts))
        runs.append((out, per))
    return runs


# ---------------------------------------------------------------------------------------------- the rules in Python

class _Item:
    __slots__ = ("eval", "cuts")

    def __init__(self, ev, cuts):
        self.eval, self.cuts = ev, cuts


def _siftdown(heap, startpos, pos):
    new = heap[pos]
    while pos > startpos:
        parent = (pos - 1) >> 1
        if new.eval < heap[parent].eval:
            heap[pos] = heap[parent]
            pos = parent
            continue
        break
    heap[pos] = new


def _siftup(heap, pos, rules):
    end, start, new = len(heap), pos, heap[pos]
    child = 2 * pos + 1
    while child < end:
        right = child + 1
        if right < end:
            if "siftup_left_on_ties" in rules:
                take_right = heap[right].eval < heap[child].eval
            else:
                take_right = not heap[child].eval < heap[right].eval
            if take_right:
                child = right
        heap[pos] = heap[child]
        pos = child
        child = 2 * pos + 1
    heap[pos] = new
    _siftdown(heap, start, pos)


def _push(heap, item):
    heap.append(item)
    _siftdown(heap, 0, len(heap) - 1)


def _pop(heap, rules):
    last = heap.pop()
    if not heap:
        return last
    ret, heap[0] = heap[0], last
    _siftup(heap, 0, rules)
    return ret


def _js_round(x):
    if not abs(x) < INF:
        return x
    f = math.floor(x)
    return f + 1.0 if x - f >= 0.5 else float(f)


def _mfv(width, col0, pos, ints, rules):
    highest, variable, value = 0.0, 0, 0.0
    for v in ints:
        row = int(pos[v]) - width
        if row < 0:
            continue
        val = float(col0[row])
        frac = abs(val - _js_round(val))
        if frac > highest or ("mfv_inclusive" in rules and frac >= highest and frac > 0.0):
            highest, variable, value = frac, v, val
    return variable, value, highest


def python_search(root, evaluate_one, rules=frozenset(), incumbents=None):
    """milp_tree_rules.cuh restated (mt_begin / mt_next / mt_consume) on one root `(w, h, status, result, col0, pos, var, ints,
    sign, options)`; evaluate_one(cuts) -> (status, result, col0, pos, var).  Returns (status, result bits, consumed
    [(eval bits, cuts)]); incumbents (a list, optional) receives the height of every incumbent in turn."""
    w, h, status, result, col0, pos, var, ints, sign, opt = root
    precision, max_iter, tol = opt["precision"], opt["maxIterations"], opt["tolerance"]
    timedout = opt["timeout"] <= 0
    if status != "optimal" or not ints:
        return status, bits(result), []
    variable, value, frac = _mfv(w, col0, pos, ints, rules)
    if frac <= precision:
        return "optimal", bits(result), []
    heap, seq = [], []
    _push(heap, _Item(result, [(-1, variable, float(np.ceil(value)))]))
    _push(heap, _Item(result, [(1, variable, float(math.floor(value)))]))
    threshold = result * (1.0 - sign * tol)
    best, found, it = INF, False, 0.0
    while it < max_iter and heap and best >= threshold and not timedout:
        br = _pop(heap, rules)
        if br.eval > best:
            break
        seq.append((B.hexd(br.eval), tuple((s, v, B.hexd(x)) for s, v, x in br.cuts)))
        st, res, c0, p, _ = evaluate_one(br.cuts)
        if st == "optimal" and res < best:
            variable, value, frac = _mfv(w, c0, p, ints, rules)
            if frac <= precision:
                found, best = True, res
                if incumbents is not None:
                    incumbents.append(h + len(br.cuts))
            else:
                upper, lower = [], []
                for cut in br.cuts:
                    if cut[1] == variable:
                        (lower if cut[0] < 0 else upper).append(cut)
                    else:
                        upper.append(cut)
                        lower.append(cut)
                new_lo, new_up = (1, variable, float(math.floor(value))), (-1, variable, float(np.ceil(value)))
                if "new_cut_first" in rules:
                    lower, upper = [new_lo] + lower, [new_up] + upper
                else:
                    lower, upper = lower + [new_lo], upper + [new_up]
                kids = [_Item(res, upper), _Item(res, lower)]
                if "push_lower_first" in rules:
                    kids.reverse()
                for k in kids:
                    _push(heap, k)
        it += 1.0
    unfinished = (timedout or it >= max_iter) and bool(heap) and best >= threshold
    return ("timedout" if unfinished else "optimal" if found else "infeasible"), bits(best if found else NAN), seq


# ---------------------------------------------------------------------------------------------- GPU shapes

def incumbent_heights(oracle, model, opt):
    """(nodes consumed, the heights of the successive incumbents) of one model, by python_search over the oracle."""
    root = MB.Root(oracle, model, opt)
    ev, heights = MB.OracleEvaluator(oracle, [root]), []
    _, _, seq = python_search(root.packed(), lambda cuts: ev.one(0, cuts), incumbents=heights)
    return len(seq), heights


def grid_one_models():
    """(name, model, options) that ONE workgroup walks in sequence (YALPS_MILPTREE_GRID=1): see test_one_workgroup_many_trees."""
    return [
        ("two incumbents", MB.packing_model(40, 40, 6, 1), {}),
        ("integral root", ML._model("maximize", [1.0, 1.0], [[1, 0], [0, 1]], [{"max": 2.0}, {"max": 3.0}], range(2)), {}),
        ("root infeasible", BS.infeasible_model(), {}),
        ("timeout <= 0", ML.make("ties", 1)[0], {"timeout": 0}),
        ("maxIterations 0", ML.make("break", 1)[0], {"maxIterations": 0}),
        ("20 nodes", MB.packing_model(30, 30, 8, 33), {"maxIterations": 20}),
        ("ties again", ML.make("ties", 2)[0], {}),
    ]


def shape_models():
    """(name, model, options): roots just under each LDS class bound (so the tree's largest node is of the next class), under the
    LDS -> HBM bound, under the aux bound (tall 8161 x 31 and wide 41 x 8151), and a tree with one integer variable."""
    one = BS.packing(40, 40, 1, 3, 0.6)
    rows = [("under bound %d" % k, BS.bound_model(k), {"maxIterations": 12}) for k in range(4)]
    rows += [("tall under the aux bound", BS.packing(8160, 30, 6, 1, 0.3), {"maxIterations": 6}),
             ("wide under the aux bound", BS.wide_model(), {"maxIterations": 6}),
             ("one integer", one, {"maxIterations": 16}),
             ("one integer, check", one, {"maxIterations": 16, "checkCycles": True})]
    return rows


def negzero_cut_models():
    """(name, model, options) whose first cut has the value -0.0: under a precision of 0.4 phase 2 passes over the coefficient 0.3,
    the root is optimal with x2 = -0.5 in column 0, and Math.ceil(-0.5) is -0.0."""
    rows = [[0.3, 1], [1, 0]], [{"max": 0.5}, {"max": 10 / 3}]
    return [("-0.0 cut, objective %s" % (obj,), ML._model("maximize", obj, *rows, ints=[1]), {"precision": 0.4}) for obj in ([1, 1], [2, 1])]


def largest_class(milp):
    w, h, n = milp[0], milp[1], len(milp[5])
    return LB.size_class(w, h + 2 * n)


def spelling(symbol):
    """kernel<T[,check][,lds]> of a mangled lp_batch_kernel / milp_tree_kernel symbol, as yalps_milptree_info spells it."""
    from tests import _census
    name, args = _census.parse(symbol)
    assert name in ("lp_batch_kernel", "milp_tree_kernel") and len(args) == 3, (symbol, name, args)
    lanes, check, lds = args
    return "%s<%d%s%s>" % (name, lanes, ",check" if check else "", ",lds" if lds else "")


# ---------------------------------------------------------------------------------------------- a handle on a caller's stream

def stream_milps():
    return [MB.milp_of(MB.record_model(r), r["options"]) for r in MB.batchable_records()[:30]]


def outputs(tree, out, count):
    """What a solve left behind, as arrays: statuses, result words, nodes used, and a digest of every best tableau."""
    sols = [tree.solution(i) for i in range(count)]
    return dict(status=np.array(out[0]), result=np.asarray(out[1]).view(np.int64), used=np.asarray(out[2]),
                height=np.array([s[0] for s in sols]), best=np.array([B.sha(*s[1:]) for s in sols]))


def caller_stream_child(path):
    """stream_milps() through a MilpTree on a stream torch made, its outputs to `path` (.npz).  A process of its own, for the
    reason tests/_variant_shapes.py::caller_stream_child gives: torch has to be loaded before the library."""
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from yalps_amd import _native as nat
    milps = stream_milps()
    stream = torch.cuda.Stream()
    t = nat.MilpTree(0, stream=stream.cuda_stream)
    try:
        np.savez(path, **outputs(t, t.solve(milps), len(milps)))
    finally:
        t.close()  # (before the stream is dropped)
    del stream


if __name__ == "__main__":
    import sys
    caller_stream_child(sys.argv[1])
