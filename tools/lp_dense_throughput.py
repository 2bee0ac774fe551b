"""LPs per second of a batch of dense LPs that already lie on the GPU as tensors: (a) linprog_batch from the resident tensors,
outputs as tensors; (b) the bare LpDense.solve on the same pointers into preallocated outputs; and what a tensor user paid before
libyalps_lpdense.so -- (c) LpBatch.solve on the same LPs pre-packed on the host (the packing not counted), (d) the packing of
the host numpy tableaux (dense_cells + PackedLps) and LpBatch.solve inside the clock (the copy of the tensors to the host not
even counted).  Same box, same run; per figure the median of `--repeats` timed windows of at least 0.1 s after two warm-up calls, with min and max;
the kernels' own time per call (HIP events, median) next to it.  Writes profiles/lp_dense_throughput.json.

    python tools/lp_dense_throughput.py [--repeats 5] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the package's libraries: yalps_amd/tensors.py says why)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

torch.cuda.init()

from yalps_amd import _native as N  # noqa: E402
from yalps_amd import tensors  # noqa: E402

WORKLOADS = {"dense30": (30, 30, 4096), "dense96": (96, 80, 2048), "dense300": (300, 280, 256)}


WINDOW = 0.1  # seconds a timed repeat lasts at least: a route that answers in a fraction of a millisecond is called again and again


def timed(fn, repeats):
    """Seconds per call of `repeats` timed windows after a warm-up; a window is as many calls as fill WINDOW (by a second warm-up call)."""
    fn()  # warm-up
    t0 = time.perf_counter()
    fn()
    inner = max(1, int(WINDOW / max(time.perf_counter() - t0, 1e-9)) + 1)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ts.append((time.perf_counter() - t0) / inner)
    return ts


def rate(count, ts):
    return {"lps_per_s": count / statistics.median(ts), "lps_per_s_min": count / max(ts), "lps_per_s_max": count / min(ts),
            "seconds_per_call": ts, "lps": count}


def figures(M, N_, count, repeats):
    w, h = N_ + 1, M + 1
    dense = [N.dense_lp(M, N_, 1 + s) for s in range(count)]  # host numpy, flat row-major: row 0 = 0, c; rows 1.. = b, A
    T = np.stack(dense).reshape(count, h, w)
    assert not T[:, 0, 0].any()
    c, A, b = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (T[:, 0, 1:], T[:, 1:, 1:], T[:, 1:, 0]))
    packed = N.PackedLps([(w, h, *N.dense_cells(m, w, h), 1e-8, 8192.0, False) for m in dense])
    batch = N.LpBatch(0)
    bare = N.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    x = torch.empty((count, N_), dtype=torch.float64, device="cuda")
    objective = torch.empty((count,), dtype=torch.float64, device="cuda")
    status = torch.empty((count,), dtype=torch.int32, device="cuda")
    pivots = torch.empty((count,), dtype=torch.int64, device="cuda")
    operands = (tensors._strides(c, True, False), tensors._strides(A, True, True), tensors._strides(b, True, False), None, None)
    torch.cuda.synchronize()
    try:
        ms = {"linprog_batch": [], "lpdense": [], "lpbatch": [], "lpbatch_packing": []}
        held = {}

        def fa():
            stats = {}
            held["a"] = tensors.linprog_batch(c, A, b, maximize=True, stats=stats)
            ms["linprog_batch"].append(stats["gpu_ms"])
            held["launches"] = [(k["kernel"], k["class"], k["lps"], k["grid"], k["lds"]) for k in stats["kernels"]]

        def fb():
            ms["lpdense"].append(bare.solve(count, N_, M, 0, operands, maximize=True, x=x.data_ptr(), objective=objective.data_ptr(),
                                            status=status.data_ptr(), pivots=pivots.data_ptr()))

        def fc():
            held["c"] = batch.solve(packed)
            ms["lpbatch"].append(held["c"][3])

        def fd():
            p = N.PackedLps([(w, h, *N.dense_cells(m, w, h), 1e-8, 8192.0, False) for m in dense])
            ms["lpbatch_packing"].append(batch.solve(p)[3])

        row = {"lps": count, "linprog_batch": rate(count, timed(fa, repeats)), "lpdense_solve": rate(count, timed(fb, repeats)),
               "lpbatch_prepacked": rate(count, timed(fc, repeats)), "lpbatch_with_packing": rate(count, timed(fd, repeats))}
        # the routes solve the same LPs: same statuses, same pivot counts, same objective bits
        a, (statuses, results, piv, _) = held["a"], held["c"]
        assert tensors.status_names(a.status) == list(statuses) == tensors.status_names(status)
        assert np.array_equal(a.pivots.cpu().numpy(), piv) and np.array_equal(pivots.cpu().numpy(), piv)
        assert np.array_equal(a.objective.cpu().numpy().view(np.int64), (-results).view(np.int64))
        assert torch.equal(a.x, x) and torch.equal(a.objective, objective)
        pv = np.asarray(piv, np.float64)
        row.update(optimal=int(sum(s == "optimal" for s in statuses)), pivots_mean=float(pv.mean()), pivots_min=int(pv.min()),
                   pivots_max=int(pv.max()), gpu_ms={k: statistics.median(v[2:]) for k, v in ms.items()}, launches=held["launches"],
                   operand_bytes=int(8 * (c.numel() + A.numel() + b.numel())), cell_bytes=int(16 * packed.row.size))
        for k in ("lpbatch_prepacked", "lpbatch_with_packing"):
            row["linprog_batch_over_" + k] = row["linprog_batch"]["lps_per_s"] / row[k]["lps_per_s"]
            row["linprog_batch_beats_%s_beyond_spread" % k] = row["linprog_batch"]["lps_per_s_min"] > row[k]["lps_per_s_max"]
        row["kernel_ms_lpdense_over_lpbatch"] = statistics.median(ms["lpdense"][2:]) / statistics.median(ms["lpbatch"][2:])
        return row
    finally:
        bare.close()
        batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_dense_throughput.json"))
    args = ap.parse_args()
    result = {"repeats": args.repeats, "workloads": {}}
    for name, (M, N_, count) in WORKLOADS.items():
        if args.only is not None and name not in args.only.split(","):
            continue
        row = figures(M, N_, count, args.repeats)
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) and "lps_per_s" in v else v)
                                for k, v in row.items() if k not in ("gpu_ms", "launches")}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
