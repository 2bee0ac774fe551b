"""A whole world of row shards in ONE process (TEST INFRASTRUCTURE): one ops object per rank, the all-gather a torch.cat.

yalps_shard_select writes a rank's slot to a pointer, yalps_shard_apply reads every slot from a pointer, and the collective
between them belongs to the caller -- so the ranks of a world need neither processes nor gloo: `run_world` restates the
loop of yalps_amd.sharded.sharded_simplex over a list of ops.  The ops class is a parameter: NumpyShardOps and
NumpyDelayedShardOps (tests/_shard_numpy.py) drive it on the CPU, HipShardOps (private_stream=False: every rank enqueues
on torch's current stream, which orders all their steps) on the GPU.  Any non-decreasing bounds from 1 to h, 1 to 8 ranks:
empty ranks anywhere, one-row ranks, every row on one rank.  Nothing is read back inside the loop but the status polls;
all comparing is the caller's, on what `run_world` returns."""
import numpy as np
import torch

from tests import _golden as G

NONE = 2147483647
MAX_RANKS = 8


def tie_input(dense_lp, M, N, seed, bounds, phase1=True):
    """dense_lp(M, N, seed) with the `phase1` recipe of tests/_shard_worker.py (one row "-a x <= -b", exact zeros), then
    identical rows planted across every rank boundary: row b = row b - 1 for every interior bound 1 < b < h, and row h - 1 =
    row 1 (the first rank that has rows against the last).  Identical rows stay bit-identical until one of them is the
    pivot row: their ratio keys and RHS keys tie across ranks, and only the lower-global-row rule decides.
    phase1=False leaves the one row as it is: the start is feasible, every pivot is a phase-2 pivot (the ratio candidates
    decide, where the recipe's solves spend most of their pivots in phase 1)."""
    w, h = N + 1, M + 1
    m = dense_lp(M, N, seed)
    A = m.reshape(h, w)
    if phase1:
        A[h // 3] *= -1.0
    A[5::7, 3::5] = 0.0
    for b in sorted(set(bounds)):
        if 1 < b < h:
            A[b] = A[b - 1]
    A[h - 1] = A[1]
    return m


def check_bounds(bounds, h):
    assert 1 <= len(bounds) - 1 <= MAX_RANKS and bounds[0] == 1 and bounds[-1] == h, bounds
    assert all(a <= b for a, b in zip(bounds, bounds[1:])), bounds


def gather(ops):
    """The all-gather: every rank's send slot, in rank order, into every rank's recv.  Returns the gathered tensor."""
    cat = torch.cat([o.send for o in ops])
    for o in ops:
        o.recv.copy_(cat)
    return cat


def run_world(make_ops, m, w, h, bounds, max_pivots, precision=1e-8, check_every=8, check_cycles=False):
    """Drives one solve of the (h x w) tableau `m` over len(bounds) - 1 ranks; make_ops(local, w, bounds, rank, h, pos, var)
    builds a rank.  At every poll all ranks must report the same (status, result, pivots).
    Returns a dict: status (name), result, pivots, matrix (assembled from every rank's OWN rows), and per rank obj (its
    replica of the objective row), pos, var; keys: float64 [steps, ranks, 4] = (ratio key, ratio row, RHS key, RHS row) of
    every rank as gathered at every step (step k decides pivot k + 1 while the solve runs); info: per rank, tab.info() of an
    ops object that has a device tableau (its kernels), else {}."""
    from yalps_amd import sharded
    assert np.isfinite(max_pivots), "every world carries a finite pivot budget"
    check_bounds(bounds, h)
    nranks = len(bounds) - 1
    ident = np.arange(w + h, dtype=np.int32)
    ops, heads = [], []
    try:
        for r in range(nranks):
            ops.append(make_ops(sharded.local_rows(m, w, h, bounds, r), w, bounds, r, h, ident, ident.copy()))
        slot = ops[0].send.numel()
        for o in ops:
            o.begin(precision, max_pivots, check_cycles)
        while True:
            for _ in range(check_every):
                for o in ops:
                    o.select()
                heads.append(gather(ops).view(nranks, slot)[:, :4].clone())
                for o in ops:
                    o.apply()
            polls = [o.poll() for o in ops]
            for r, p in enumerate(polls):
                assert p[0] == polls[0][0] and p[2] == polls[0][2] and G.same_number(p[1], polls[0][1]), (r, p, polls[0])
            if polls[0][0] >= 0:
                break
        status, result, pivots = polls[0]
        full = np.zeros((h, w))
        out = {"status": sharded.STATUS[status], "result": result, "pivots": pivots, "obj": [], "pos": [], "var": []}
        for r, o in enumerate(ops):
            lm, pos, var = o.download()
            lm = lm.reshape(-1, w)
            assert lm.shape[0] == 1 + bounds[r + 1] - bounds[r], (r, lm.shape)
            full[bounds[r]:bounds[r + 1]] = lm[1:]
            out["obj"].append(lm[0].copy())
            out["pos"].append(np.array(pos, copy=True))
            out["var"].append(np.array(var, copy=True))
        full[0] = out["obj"][0]
        out["matrix"] = full.reshape(-1)
        out["keys"] = torch.stack(heads).cpu().numpy()
        out["info"] = [o.tab.info() if hasattr(o, "tab") else {} for o in ops]
        return out
    finally:
        for o in ops:
            o.close()


def oracle_run(oracle, m, w, h, max_pivots, precision=1e-8, check_cycles=False):
    ref = m.copy()
    pos = np.arange(w + h, dtype=np.int32)
    var = pos.copy()
    status, result, pivots, _ = oracle.simplex(ref, w, h, pos, var, precision=precision, max_pivots=max_pivots, check_cycles=check_cycles)
    return {"status": status, "result": result, "pivots": pivots, "matrix": ref, "pos": pos, "var": var}


def check_world(got, exp, note=""):
    """Bit for bit: status, pivot count, result, the assembled tableau, and EVERY rank's objective row, pos and var."""
    w = got["obj"][0].size
    assert (got["status"], got["pivots"]) == (exp["status"], exp["pivots"]), (got["status"], got["pivots"], exp["status"], exp["pivots"], note)
    assert G.same_number(got["result"], exp["result"]), (got["result"], exp["result"], note)
    for r in range(len(got["obj"])):
        assert np.array_equal(got["obj"][r].view(np.int64), exp["matrix"][:w].view(np.int64)), ("objective row of rank %d" % r, note)
        assert np.array_equal(got["pos"][r], exp["pos"]), ("pos of rank %d" % r, note)
        assert np.array_equal(got["var"][r], exp["var"]), ("var of rank %d" % r, note)
    bad = np.flatnonzero(got["matrix"].view(np.int64) != exp["matrix"].view(np.int64))
    assert bad.size == 0, ("%d entries differ, first in row %d" % (bad.size, bad[0] // w), note)


def cross_rank_ties(keys, pivots):
    """(ratio ties, RHS ties, pivots decided by a ratio tie, by an RHS tie) over the steps that decided a pivot.  A ratio
    (RHS) tie: the winning ratio (RHS) key among the gathered slots is held by two or more ranks, so that the reduction over
    the slots has to fall back on the lower global row.  Both keys travel at every step, whatever the phase; a tie is `deciding` where it is in the key
    the phase reads -- the RHS key in phase 1, which lasts until the first step at which no rank has an RHS candidate
    (src/simplex.ts:120), the ratio key after it -- so that the pivot row itself was chosen by that rule."""
    ratio = rhs = by_ratio = by_rhs = 0
    phase = 1
    for k in range(min(pivots, keys.shape[0])):
        if phase == 1 and np.all(keys[k, :, 3] == NONE):
            phase = 2
        tied = []
        for key, row in ((keys[k, :, 0], keys[k, :, 1]), (keys[k, :, 2], keys[k, :, 3])):
            have = row != NONE
            tied.append(bool(have.any()) and int(np.count_nonzero(have & (key == key[have].min()))) >= 2)
        ratio += tied[0]
        rhs += tied[1]
        by_ratio += tied[0] and phase == 2
        by_rhs += tied[1] and phase == 1
    return ratio, rhs, by_ratio, by_rhs
