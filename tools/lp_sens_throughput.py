"""LPs per second of a batch of independent LPs WITH their sensitivity ranges: (a) one LpSens.solve (yalps_lpsens_solve) of
pre-packed arrays plus ranges(i) of every LP, (b) what there was before libyalps_lpsens.so -- LpBatch.solve(keep_tableaux=True),
tableau(i) of every LP and the vectorised numpy ranging on the host (sensitivity.ranges_from_tableau) --, (c) LpBatch.solve
alone, the solve without any ranges.  Same box, same run; per figure the median of `--repeats` timed repeats after one
warm-up, with min and max.  (a) / (c) is the price of the epilogue; the kernels' own time (HIP events) is recorded next to it,
and the LPs' pivot counts.  Writes profiles/lp_sens_throughput.json.

    python tools/lp_sens_throughput.py [--repeats 5] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yalps_amd import _native as N  # noqa: E402
from yalps_amd.sensitivity import ranges_from_tableau  # noqa: E402

WORKLOADS = {"dense30": (30, 30, 4096), "dense96": (96, 80, 2048), "dense300": (300, 280, 256)}


def lps_dense(M, N_, count, seed0=1):
    return [(N_ + 1, M + 1, *N.dense_cells(N.dense_lp(M, N_, seed0 + s), N_ + 1, M + 1), 1e-8, 8192.0, False)
            for s in range(count)]


def timed(fn, repeats):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def rate(count, ts):
    return {"lps_per_s": count / statistics.median(ts), "lps_per_s_min": count / max(ts), "lps_per_s_max": count / min(ts),
            "seconds": ts, "lps": count}


def figures(lps, repeats):
    packed = N.PackedLps(lps)
    n = len(lps)
    sens, batch = N.LpSens(0), N.LpBatch(0)
    try:
        ms = {"sens": [], "keep": [], "solve": []}
        held = {}

        def a():
            out = sens.solve(packed)
            ms["sens"].append(out[3])
            held["a"] = [sens.ranges(i) for i in range(n) if out[0][i] == "optimal"]
            held["pivots"], held["statuses"] = out[2], out[0]

        def b():
            out = batch.solve(packed, keep_tableaux=True)
            ms["keep"].append(out[3])
            held["b"] = [ranges_from_tableau(batch.tableau(i), lps[i][0], lps[i][1], lps[i][5]) for i in range(n)
                         if out[0][i] == "optimal"]

        def c():
            ms["solve"].append(batch.solve(packed)[3])

        row = {"lps": n, "sens": rate(n, timed(a, repeats)), "keep_tableaux_and_host_ranging": rate(n, timed(b, repeats)),
               "solve_alone": rate(n, timed(c, repeats))}
        # the two routes give the same numbers (row0 bit for bit, the ratios as numbers)
        assert len(held["a"]) == len(held["b"]) > 0
        for x, y in zip(held["a"], held["b"]):
            assert np.array_equal(x[0].view(np.int64), y[0].view(np.int64)) and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))
        piv = np.asarray(held["pivots"], np.float64)
        row.update(optimal=len(held["a"]), pivots_mean=float(piv.mean()), pivots_min=int(piv.min()), pivots_max=int(piv.max()),
                   gpu_ms={k: v[1:] for k, v in ms.items()},
                   launches=[(k["kernel"], k["class"], k["lps"], k["grid"], k["lds"]) for k in sens.info()["kernels"]])
        row["sens_over_solve_alone"] = row["sens"]["lps_per_s"] / row["solve_alone"]["lps_per_s"]
        row["kernel_ms_sens_over_solve_alone"] = statistics.median(ms["sens"][1:]) / statistics.median(ms["solve"][1:])
        row["sens_beats_host_ranging_beyond_spread"] = row["sens"]["lps_per_s_min"] > row["keep_tableaux_and_host_ranging"]["lps_per_s_max"]
        return row
    finally:
        sens.close()
        batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_sens_throughput.json"))
    args = ap.parse_args()
    result = {"repeats": args.repeats, "workloads": {}}
    for name, (M, N_, count) in WORKLOADS.items():
        if args.only is not None and name not in args.only.split(","):
            continue
        row = figures(lps_dense(M, N_, count), args.repeats)
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) and "lps_per_s" in v else v)
                                for k, v in row.items() if k not in ("gpu_ms", "launches")}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
    if not all(r["sens_beats_host_ranging_beyond_spread"] for r in result["workloads"].values()):
        raise SystemExit("the slowest repeat of LpSens is not above the fastest repeat of keep_tableaux + host ranging everywhere")


if __name__ == "__main__":
    main()
