"""Child process of tests/test_kernel_census.py: every row-shard census row at world size 1, in one process.
usage: python -m tests._census_shards <rows.json> <out.npz>

rows.json: [{"key", "M", "N", "env", "check", "budget"}, ...].  One context (and one host-transport communicator) per value
of YALPS_HIP_BLOCKS, which the context reads when it is created; every other switch is set in the environment before the
tableau is created and partitioned (yalps_tableau_set_shard reads them there).  The input is tests/test_kernel_census.py's
(dense_lp with one row negated and a lattice of exact zeros).  For row i the npz holds r<i>_status, r<i>_result, r<i>_pivots,
r<i>_launched, the final tableau r<i>_matrix and both permutations r<i>_pos, r<i>_var."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def census_input(orc, M, N):
    w, h = N + 1, M + 1
    m = orc.dense_lp(M, N, 23)
    A = m.reshape(h, w)
    A[h // 3] *= -1.0
    A[5::7, 3::5] = 0.0
    return m


def main():
    import torch  # noqa: F401  (the library's comm helpers expect torch loaded, as in the multi-rank workers)
    from tests import _oracle
    from yalps_amd import _native, sharded
    rows = json.load(open(sys.argv[1]))
    out = {}
    orc = _oracle.load()
    switches = sorted({k for r in rows for k in r["env"]})
    contexts = {}
    try:
        for i, r in enumerate(rows):
            for k in switches:
                os.environ.pop(k, None)
            os.environ.update(r["env"])
            blocks = r["env"].get("YALPS_HIP_BLOCKS", "")
            if blocks not in contexts:
                ctx = _native.Context(0)
                contexts[blocks] = (ctx, sharded.native_comm(ctx, 0, 1, transport="host"))
            ctx, comm = contexts[blocks]
            M, N = r["M"], r["N"]
            w, h = N + 1, M + 1
            m = census_input(orc, M, N)
            ident = np.arange(w + h, dtype=np.int32)
            ops = sharded.HipShardOps.__new__(sharded.HipShardOps)
            ops.ctx, ops.perm_len = ctx, w + h
            ops.tab = _native.DeviceTableau(ctx, w, h)
            try:
                ops.tab.upload(m, h, ident, ident.copy())
                ops.tab.set_shard(0, 1, sharded.partition(h, 1), h, ident, ident.copy())
                status, result, pivots = sharded.sharded_simplex_native(ops, comm, max_pivots=r["budget"], check_cycles=r["check"])
                info = ops.tab.info()
                got, pos, var = ops.tab.download(perm_len=w + h)
            finally:
                ops.tab.close()
            key = "r%d_" % i
            out[key + "status"], out[key + "result"], out[key + "pivots"] = status, result, pivots
            out[key + "launched"] = info.get("launched", "")
            out[key + "matrix"], out[key + "pos"], out[key + "var"] = got, pos, var
            print("row %s: %s %d pivots, launched=%s" % (r["key"], status, pivots, info.get("launched")), flush=True)
    finally:
        for ctx, comm in contexts.values():
            comm.close()
            ctx.close()
    np.savez(sys.argv[2], **out)
    print("ok")


if __name__ == "__main__":
    main()
