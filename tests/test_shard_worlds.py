"""The row-shard kernels at world sizes 4 to 8 and on uneven partitions, in one process (tests/_shard_world.py): one
HipShardOps per rank on one stream, the all-gather a torch.cat.  Until now no HIP shard kernel had taken a decision from more
than three gathered slots, and every partition came from sharded.partition(): blocks that differ by at most one row, empty
ranks at the end only.  Here: the owner lookup up to g = 7, the reduction over up to 8 candidates with cross-rank ties, the
winner's row fetched from slots beyond 2 * gstride, ranks with no rows (a tableau of height 1: the objective row travels as
the "candidate"), one-row ranks, an empty rank in the middle, every row on the first or on the last rank of 8.

The inputs put the decision on the rank boundaries (tie_input: identical rows across every boundary); every world carries a
finite pivot budget -- without one these degenerate inputs do not end.  The numpy stand-ins of tests/_shard_numpy.py define
what a world does; the single-process oracle is the judge.  Everything is compared bit for bit: status, pivot count, result,
the tableau assembled from each rank's own rows, EVERY rank's objective row, pos and var, and, on the GPU, the keys of every
gathered slot at every pivot against the stand-in's.

Not covered here: the native loop yalps_shard_run and with it dshard_sweep_kernel as a launch of its own beyond
3 ranks, RCCL between ranks, full-size tableaux.

Slowest GPU case, measured on an MI355X: 0.5 s, the stand-in's reference run included (dshard_kernel<512,16,panel>, 101 x 9001 over
8 ranks, 40 pivots); the 101 GPU tests and the 94 CPU tests of this module together: 13 s."""
import functools

import numpy as np
import pytest

from tests import _golden as G
from tests import _shard_world as W
from tests._shard_numpy import NumpyDelayedShardOps, NumpyShardOps

STANDINS = {
    "numpy": NumpyShardOps,
    "numpy-delayed4": functools.partial(NumpyDelayedShardOps, depth=4),
    "numpy-delayed16": functools.partial(NumpyDelayedShardOps, depth=16),
}


def partition(h, nranks):
    from yalps_amd import sharded
    return sharded.partition(h, nranks)


def worlds(h):
    """name -> bounds for a tableau of height h (h >= 36), as fractions of h where they are not counted in rows."""
    out = {"even%d" % k: partition(h, k) for k in (4, 5, 7, 8)}
    out["fib"] = [1, 2, 3, 5, 8, 13, 21, 34, h]          # blocks of 1, 1, 2, 3, 5, 8, 13 rows, the rest on the last rank
    out["gaps"] = [1, 1, 2, 2, 2, h // 2, h, h, h]        # empty first, two empty in the middle, two last; rank 1 has one row
    out["last"] = [1] * 8 + [h]                           # every row on rank 7
    out["first"] = [1] + [h] * 8                          # every row on rank 0
    return out


def owners(bounds):
    return sum(1 for a, b in zip(bounds, bounds[1:]) if b > a)


class Case:
    """One world: the input (tie_input's arguments), the bounds, the budget; `ties`: the tie condition is asserted (at least
    two ranks own rows; phase-1 recipe); `check`: checkCycles on a given matrix instead."""

    def __init__(self, name, M, N, seed, bounds, budget, phase1=True, matrix=None, check=False, precision=1e-8):
        self.name, self.M, self.N, self.seed, self.bounds, self.budget = name, M, N, seed, list(bounds), float(budget)
        self.phase1, self.matrix, self.check, self.precision = phase1, matrix, check, precision
        self.w, self.h = N + 1, M + 1
        self.ties = matrix is None and owners(bounds) >= 2

    def __repr__(self):
        return "%s %dx%d seed %s bounds %s budget %d" % (self.name, self.h, self.w, self.seed, self.bounds, self.budget)


@functools.lru_cache(maxsize=None)
def _reference_of(oracle, case):
    """(input, the oracle's run, the plain stand-in's world): computed once per case, shared, never changed."""
    m = case.matrix() if case.matrix else W.tie_input(oracle.dense_lp, case.M, case.N, case.seed, case.bounds, case.phase1)
    exp = W.oracle_run(oracle, m, case.w, case.h, case.budget, precision=case.precision, check_cycles=case.check)
    ref = W.run_world(NumpyShardOps, m, case.w, case.h, case.bounds, case.budget, precision=case.precision, check_cycles=case.check)
    for a in [m, ref["keys"], ref["matrix"]] + [exp[k] for k in ("matrix", "pos", "var")]:
        a.setflags(write=False)
    return m, exp, ref


def reference(oracle, case):
    """... with the condition every tie case must meet BEFORE anything is compared: at least 5 pivots with a cross-rank tie
    of the ratio keys and at least 1 with a cross-rank tie of the RHS keys (phase-1 recipe); on the feasible variant, where
    every pivot is a phase-2 pivot, at least 1 pivot whose row the tie rule chose among the ratio candidates."""
    m, exp, ref = _reference_of(oracle, case)
    if case.ties:
        ratio, rhs, by_ratio, by_rhs = W.cross_rank_ties(ref["keys"], ref["pivots"])
        if case.phase1:
            assert ratio >= 5 and rhs >= 1, ("the input does not tie across ranks: change the seed", case, ratio, rhs)
        else:
            assert by_ratio >= 1, ("no phase-2 pivot was decided by a cross-rank tie: change the seed", case, ratio, by_ratio)
    return m, exp, ref


# ---- CPU: both stand-ins through the one-process world, small widths ------------------------------------------------------
def _chvatal(hh, ww):
    """Chvatal's cycling LP (the reference's own test case) padded with all-zero rows and columns (they never leave / enter),
    as tests/test_sharded.py's `chvatal-wide`."""
    def make():
        from tests import _oracle
        rec = next(r for r in G.records("cases") if r["name"] == "Chvatal Cycling")
        big = np.zeros((hh, ww))
        big[:rec["height"], :rec["width"]] = G.initial_matrix(rec, _oracle.load()).reshape(rec["height"], rec["width"])
        return big.reshape(-1)
    return make


# Chvatal's three constraint rows on ranks 4, 5 and 6 of 8, ranks 0-3 empty, the zero rows on rank 7
CHVATAL_BOUNDS = [1, 1, 1, 1, 1, 2, 3, 4, 40]

# The edge records of tests/golden (ties, the early break, +inf ratios, signed zeros, the flush band, subnormals: the families
# tests/test_edge_paths.py runs on 1-3 ranks) on two 8-rank worlds: the tie worlds above all end at their budgets, these end
# "optimal", "unbounded", "infeasible", "cycled" by budget and by the detector -- with pivots pending where the updates are delayed.
EDGE_FAMILIES = ("E1", "E2", "E2b", "E3u", "E4", "E5", "E8", "E9c")
EDGE_WORLDS = ("even8", "gaps")


@functools.lru_cache(maxsize=None)
def edge_cases(M, N):
    from tests import _edges as E

    def initial(rec):
        def make():
            from tests import _oracle
            return E.initial(rec, _oracle.load().dense_lp)
        return make
    out = []
    for rec in G.records("edges"):
        if (rec["M"], rec["N"]) != (M, N) or rec["family"] not in EDGE_FAMILIES:
            continue
        o = G.options(rec)
        for wname in EDGE_WORLDS:
            c = Case("%s-%s" % (E.label(rec), wname), M, N, None, worlds(M + 1)[wname], o["max_pivots"], matrix=initial(rec),
                     check=o["check_cycles"], precision=o["precision"])
            c.sha256, c.ending = G.expected(rec)["final_sha256"], (G.expected(rec)["status"], G.expected(rec)["n_pivots"])
            out.append((wname, c))
    assert {c.ending[0] for _, c in out} == {"optimal", "unbounded", "infeasible", "cycled"}, (M, N)
    return tuple(out)


CPU_CASES = [
    Case("41x31-even8", 40, 30, 7, partition(41, 8), 60),
    Case("41x31-gaps", 40, 30, 7, [1, 1, 2, 2, 2, 20, 41, 41, 41], 60),
    Case("41x31-last", 40, 30, 7, [1, 1, 1, 1, 1, 1, 1, 1, 41], 60),
    Case("41x31-first", 40, 30, 7, [1, 41, 41, 41, 41, 41, 41, 41, 41], 60),
    Case("41x31-even4", 40, 30, 7, partition(41, 4), 60),
    Case("41x31-even5", 40, 30, 7, partition(41, 5), 60),
    Case("42x34-fib", 41, 33, 4, [1, 2, 3, 5, 8, 13, 21, 34, 42], 60),
    Case("42x34-even7", 41, 33, 4, partition(42, 7), 60),
    Case("121x301-even8", 120, 300, 1, partition(121, 8), 60),
    Case("121x301-uneven", 120, 300, 1, [1, 2, 2, 60, 61, 61, 119, 120, 121], 60),
    Case("41x31-even8-feasible", 40, 30, 7, partition(41, 8), 60, phase1=False),
    Case("41x31-gaps-feasible", 40, 30, 7, [1, 1, 2, 2, 2, 20, 41, 41, 41], 60, phase1=False),
    Case("42x34-fib-feasible", 41, 33, 4, [1, 2, 3, 5, 8, 13, 21, 34, 42], 60, phase1=False),
    Case("chvatal-check", 39, 150, None, CHVATAL_BOUNDS, 500, matrix=_chvatal(40, 151), check=True),
] + [c for _, c in edge_cases(200, 150)]


def _check_record(case, got):
    """An edge record's world against the golden record itself, beside the oracle's run."""
    if hasattr(case, "sha256"):
        assert (got["status"], got["pivots"]) == case.ending, (got["status"], got["pivots"], case.ending)
        assert G.sha256(got["matrix"]) == case.sha256, case


@pytest.mark.filterwarnings("ignore:overflow encountered in scalar divide:RuntimeWarning")  # (E3u: +inf ratios, meant)
@pytest.mark.parametrize("kind", list(STANDINS))
@pytest.mark.parametrize("case", CPU_CASES, ids=[c.name for c in CPU_CASES])
def test_standin_world_equals_the_oracle(oracle, case, kind):
    """Every stand-in, every world of the table: the world's result is the single-process oracle's, bit for bit, on every
    rank -- so the stand-ins define what an empty, a one-row and a middle-empty rank do.  The delayed stand-ins must also
    gather the very slots the plain one gathers (same keys at every pivot)."""
    m, exp, ref = reference(oracle, case)
    got = ref if kind == "numpy" else W.run_world(STANDINS[kind], m, case.w, case.h, case.bounds, case.budget, precision=case.precision,
                                                  check_cycles=case.check)
    W.check_world(got, exp, case)
    _check_record(case, got)
    if case.check:
        assert exp["status"] == "cycled" and exp["pivots"] < case.budget, (exp["status"], exp["pivots"])  # (hasCycle, not the budget)
    n = got["pivots"]
    assert np.array_equal(got["keys"][:n].view(np.int64), ref["keys"][:n].view(np.int64))


def test_a_world_with_two_slots_swapped_is_rejected(oracle, monkeypatch):
    """The comparison has teeth: an all-gather that delivers rank 2's slot in rank 5's place (and the reverse) to everybody
    leaves the ranks in agreement with each other -- and must not pass."""
    case = CPU_CASES[0]
    m, exp, _ = reference(oracle, case)
    slot = 8 + 2 * ((case.w - 1 + 15) // 16 * 16)
    plain = W.gather

    def swapped(ops):
        cat = plain(ops).view(len(ops), slot)
        cat[[2, 5]] = cat[[5, 2]]
        for o in ops:
            o.recv.copy_(cat.reshape(-1))
        return cat.reshape(-1)
    monkeypatch.setattr(W, "gather", swapped)
    with pytest.raises(AssertionError):
        W.check_world(W.run_world(NumpyShardOps, m, case.w, case.h, case.bounds, case.budget), exp)


def test_a_world_whose_owner_lookup_stops_at_three_ranks_is_rejected(oracle, monkeypatch):
    """... and an owner lookup that never yields more than g = 2 -- all the suite had ever asked of the kernels' loop."""
    case = CPU_CASES[0]
    m, exp, _ = reference(oracle, case)

    def owner(self, grow):
        g = 0
        for k in range(1, min(self.nranks, 3)):
            if grow >= self.bounds[k]:
                g = k
        return g
    monkeypatch.setattr(NumpyShardOps, "_owner", owner)
    with pytest.raises(AssertionError):
        W.check_world(W.run_world(NumpyShardOps, m, case.w, case.h, case.bounds, case.budget), exp)


def test_tie_counts_of_a_known_key_table():
    """cross_rank_ties on keys written by hand: phase 1 until no rank has an RHS candidate, ties counted per key."""
    inf, none = np.inf, float(W.NONE)
    keys = np.array([
        [[-inf, 3, -2.0, 3], [-inf, 9, -2.0, 9], [inf, none, inf, none]],   # phase 1: both keys tie, the RHS tie decides
        [[1.5, 2, -1.0, 4], [1.5, 8, -3.0, 8], [inf, none, inf, none]],     # phase 1: ratio tie only
        [[2.5, 2, inf, none], [2.5, 8, inf, none], [9.0, 11, inf, none]],   # phase 2: the ratio tie decides
        [[2.5, 2, inf, none], [3.5, 8, inf, none], [inf, none, inf, none]], # phase 2: no tie
        [[1.0, 2, inf, none], [1.0, 8, inf, none], [inf, none, inf, none]], # beyond `pivots`: not counted
    ])
    assert W.cross_rank_ties(keys, 4) == (3, 1, 1, 1)


# ---- GPU: HipShardOps through the same world ---------------------------------------------------------------------------
# kernel -> (M, N, switches read by yalps_tableau_set_shard, what tab.info()["streaming"] must start with, and -- after the
# run -- what a name in `launched` must contain, seed of the phase-1 recipe, seed of the feasible variant, budget, delay depth,
# seed of the two short budgets: an RHS tie within the first 2 * depth pivots)
KERNELS = {
    "pivot": (200, 150, {}, "pivot_kernel", "pivot_kernel", 4, 4, 60, 0, None),
    "wide-inplace": (120, 3000, {"YALPS_HIP_SHARD_DELAY": "0"}, "wide_kernel", ",inplace>", 3, 1, 37, 0, None),
    "dshard-l2": (120, 3000, {"YALPS_HIP_DELAY_MIN_ROWS": "1", "YALPS_HIP_DELAY_DEPTH": "4"},
                  "dshard_kernel<512,4>,delay_depth:4", "dshard_kernel<512,4>", 3, 1, 37, 4, 1),
    "dshard-panel": (100, 9000, {"YALPS_HIP_DELAY_MIN_ROWS": "1", "YALPS_HIP_DELAY_DEPTH": "16", "YALPS_HIP_SHARD_PANEL": "1"},
                     "dshard_kernel<512,16,panel>,delay_depth:16", "dshard_kernel<512,16,panel>", 1, 1, 40, 16, 1),
}
FEASIBLE_WORLDS = ("even8", "fib", "gaps")  # the feasible variant (phase 2 only) runs on these


def _gpu_cases():
    out = []
    for kname, (M, N, _, _, _, seed1, seed2, budget, depth, seed3) in KERNELS.items():
        for wname, bounds in worlds(M + 1).items():
            out.append((kname, wname, Case("%s-%s" % (kname, wname), M, N, seed1, bounds, budget)))
        for wname in FEASIBLE_WORLDS:
            out.append((kname, wname, Case("%s-%s-feasible" % (kname, wname), M, N, seed2, worlds(M + 1)[wname], budget, phase1=False)))
        if depth:  # budgets that end between two sweeps and on a sweep
            for b in (2 * depth + 1, 2 * depth):
                out.append((kname, "even8", Case("%s-even8-budget%d" % (kname, b), M, N, seed3, partition(M + 1, 8), b)))
        # checkCycles: shard_cycle_kernel reads 8 slots and looks the owner up among ranks 4-6
        out.append((kname, "chvatal", Case("%s-chvatal-check" % kname, 39, N, None, CHVATAL_BOUNDS, 500, matrix=_chvatal(40, N + 1), check=True)))
        for wname, case in edge_cases(M, N) if (M, N) != (100, 9000) else ():  # (no record is 9001 columns wide)
            out.append((kname, wname, case))
    return out


GPU_CASES = _gpu_cases()
GPU_IDS = ["%s-%s" % (k, c.name) if hasattr(c, "sha256") else c.name for k, _, c in GPU_CASES]


def test_the_gpu_table_prints_its_worlds():
    """The bounds are written as fractions of h: here as the concrete lists (pytest -s shows them), with what every world is
    there for -- 4, 5, 7 and 8 ranks, an empty rank first / in the middle / last, a one-row rank, all rows on one rank."""
    for kname, wname, case in GPU_CASES:
        print(kname, wname, case)
        W.check_bounds(case.bounds, case.h)
    for M in {v[0] for v in KERNELS.values()}:
        ws = worlds(M + 1)
        assert sorted(len(b) - 1 for b in ws.values()) == [4, 5, 7, 8, 8, 8, 8, 8]
        assert [b[r + 1] - b[r] for b in (ws["fib"],) for r in range(7)] == [1, 1, 2, 3, 5, 8, 13]
        g = ws["gaps"]
        assert g[0] == g[1] and g[2] - g[1] == 1 and g[2] == g[3] == g[4] and g[6] == g[7] == g[8] and owners(g) == 3
        assert owners(ws["last"]) == 1 and ws["last"][7] == 1 and owners(ws["first"]) == 1 and ws["first"][1] == M + 1
    assert {c.bounds[-1] for _, w, c in GPU_CASES if w == "chvatal"} == {40}


_hip_error = []  # a world that ended in a HIP error: no further world is started in this process


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:overflow encountered in scalar divide:RuntimeWarning")
@pytest.mark.parametrize("kname,wname,case", GPU_CASES, ids=GPU_IDS)
def test_hip_world_equals_the_oracle(oracle, monkeypatch, kname, wname, case):
    """HipShardOps on every rank of the world, all on torch's current stream.  Each rank's kernel is asserted before anything
    is compared: on an even partition every rank's, on an uneven one the largest rank's (the block size decides nb and the
    rows per workgroup, and so the kernel plan_shard picks; the slots are the same whichever kernel fills them)."""
    from yalps_amd import sharded
    assert not _hip_error, "not run: an earlier world ended in a HIP error: %s" % _hip_error[0]
    _, _, env, streaming, launched = KERNELS[kname][:5]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, exp, ref = reference(oracle, case)  # (the tie condition, from the stand-in's keys)
    try:
        got = W.run_world(functools.partial(sharded.HipShardOps, device=0), m, case.w, case.h, case.bounds, case.budget,
                          precision=case.precision, check_cycles=case.check)
    except AssertionError:
        raise
    except Exception as e:
        _hip_error.append(repr(e))
        raise
    names = [i["streaming"] for i in got["info"]]
    sizes = [b - a for a, b in zip(case.bounds, case.bounds[1:])]
    even = wname.startswith("even")
    for r, i in enumerate(got["info"]):
        if even or sizes[r] == max(sizes):
            assert i["streaming"].startswith(streaming), (r, names, sizes)
            assert any(launched in k for k in i["launched"].split("+")), (r, i["launched"])
        if case.check:
            assert "shard_cycle_kernel" in i["launched"].split("+"), (r, i["launched"])
    note = (case, names)
    W.check_world(got, exp, note)
    _check_record(case, got)
    if case.check:
        assert exp["status"] == "cycled" and exp["pivots"] < case.budget, (exp["status"], exp["pivots"])
    n = got["pivots"]
    assert np.array_equal(got["keys"][:n].view(np.int64), ref["keys"][:n].view(np.int64)), note


@pytest.mark.gpu
def test_set_shard_refuses_bounds_that_decrease():
    """yalps_tableau_set_shard checked bounds[0], bounds[nranks] and the caller's own block only: [1, 50, 30, 121] on rank 0
    with 50 uploaded rows went through and left the kernels' owner lookup undefined.  Now YALPS_E_ARG, naming the first
    offending index; a rank without rows (bounds[k] == bounds[k + 1]) is still accepted, anywhere."""
    from tests import _oracle
    from yalps_amd import _native
    w, h, local = 31, 121, 50
    m = _oracle.load().dense_lp(local - 1, w - 1, 3)
    ident = np.arange(w + h, dtype=np.int32)
    ctx = _native.Context(0)
    try:
        for bounds, bad in (([1, 50, 30, 121], 2), ([1, 50, 121, 120, 121], 3), ([1, 50, 49, 40, 121], 2)):
            t = _native.DeviceTableau(ctx, w, local)
            try:
                t.upload(m, local, ident[:w + local].copy(), ident[:w + local].copy())
                with pytest.raises(_native.NativeError, match=r"bounds\[%d\] = %d < bounds\[%d\] = %d" % (bad, bounds[bad], bad - 1, bounds[bad - 1])):
                    t.set_shard(0, len(bounds) - 1, bounds, h, ident, ident.copy())
            finally:
                t.close()
        for rank, bounds in ((0, [1, 50, 50, 121]), (2, [1, 1, 1, 50, 50, 121, 121, 121, 121]), (1, [1, 1, 50, 121])):
            t = _native.DeviceTableau(ctx, w, local)
            try:
                t.upload(m, local, ident[:w + local].copy(), ident[:w + local].copy())
                t.set_shard(rank, len(bounds) - 1, bounds, h, ident, ident.copy())
                assert t.shard_slot_doubles() == 8 + 2 * 32
            finally:
                t.close()
    finally:
        ctx.close()
