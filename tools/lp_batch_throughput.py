"""LPs per second of a batch of independent LPs: (a) one LpBatch.solve (yalps_lpbatch_solve), (b) the loop of single calls
a user writes today -- simplex_host for tableaux up to solve.SPARSE_MIN_BYTES, simplex_sparse above, as solve() chooses --,
(c) the C oracle on one core and on 16 threads with one LP per thread at a time (a contiguous slice of the LPs each).  Same box, same run; per figure the median of
`--repeats` timed repeats after one warm-up, with min and max.  Writes profiles/lp_batch_throughput.json, and with
--classes the class table profiles/lp_batch_classes.json: the same LDS-form workloads with other lane counts and
workgroups per CU (YALPS_LPBATCH_LANES / YALPS_LPBATCH_PER_CU), which is what the committed class table rests on.

    python tools/lp_batch_throughput.py [--repeats 5] [--loop-sample 512] [--only NAME] [--no-baselines] [--classes]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _golden as G  # noqa: E402
from tests import _lp_batch as B  # noqa: E402
from tests import _oracle  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd.solve import SPARSE_MIN_BYTES  # noqa: E402


def workloads(orc, only=None):
    def lps_dense(M, N_, count, seed0=1):
        return [(N_ + 1, M + 1, *N.dense_cells(N.dense_lp(M, N_, seed0 + s), N_ + 1, M + 1), 1e-8, 8192.0, False)
                for s in range(count)]
    out = {}
    if only in (None, "dense30", "mix"):
        out["dense30"] = lps_dense(30, 30, 4096)
    if only in (None, "dense96", "mix"):
        out["dense96"] = lps_dense(96, 80, 2048)
    if only in (None, "golden_lds", "mix"):
        recs = [r for kind in ("cases", "mixed", "dense") for r in G.records(kind)
                if 0 <= B.size_class(r["width"], r["height"]) < 4]
        base = [B.record_lp(r, orc) for r in recs]
        out["golden_lds"] = (base * (2048 // len(base) + 1))[:max(2048, len(base))]
    if only in (None, "dense300", "mix"):
        out["dense300"] = lps_dense(300, 280, 256)
    if only in (None, "mix"):
        mix = out["dense30"] + out["dense96"] + out["golden_lds"] + out["dense300"]
        order = np.random.default_rng(1).permutation(len(mix))
        out["mix"] = [mix[j] for j in order]
    return {k: v for k, v in out.items() if only in (None, k)}


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


def batch_figure(lps, repeats, env=None):
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        b = N.LpBatch(0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        t0 = time.perf_counter()
        packed = N.PackedLps(lps)
        pack_s = time.perf_counter() - t0
        gpu_ms = []
        ts = timed(lambda: gpu_ms.append(b.solve(packed)[3]), repeats)
        fig = rate(len(lps), ts)
        # the same with the packing of the Python tuples into the three cell arrays inside the clock, as solve_many pays it
        fig["with_packing"] = rate(len(lps), timed(lambda: b.solve(N.PackedLps(lps)), repeats))
        fig.update(pack_seconds=pack_s, gpu_ms=gpu_ms[1:], launches=[(k["kernel"], k["class"], k["lps"], k["grid"], k["lds"])
                                                                     for k in b.info()["kernels"]])
        return fig
    finally:
        b.close()


def loop_figure(lps, repeats, sample):
    lps = lps[:sample]
    dense_in = [B.scatter(lp) if 8 * lp[0] * lp[1] <= SPARSE_MIN_BYTES else None for lp in lps]

    def run():
        for lp, m in zip(lps, dense_in):
            w, h = lp[0], lp[1]
            if m is None:
                N.simplex_sparse(w, h, lp[2], lp[3], lp[4], precision=lp[5], max_pivots=lp[6], check_cycles=lp[7])
            else:
                pos = np.arange(w + h, dtype=np.int32)
                N.simplex_host(m.copy(), w, h, pos, pos.copy(), precision=lp[5], max_pivots=lp[6], check_cycles=lp[7],
                               copyback=N.COPYBACK_SOLUTION)
    return rate(len(lps), timed(run, repeats))


def oracle_figure(orc, lps, repeats, threads, sample):
    """One LP per thread at a time, every thread a contiguous slice of the LPs (no task per LP).  The inputs are copied
    before the clock starts.  What stays inside: one ctypes call per LP, whose Python part holds the interpreter lock, so
    for LPs of a few microseconds the threads figure is bounded by that dispatch, not by 16 cores."""
    lps = lps[:sample]
    dense_in = [B.scatter(lp) for lp in lps]
    perms = [np.arange(lp[0] + lp[1], dtype=np.int32) for lp in lps]
    bounds = [len(lps) * t // threads for t in range(threads + 1)]
    work = []

    def prepare():
        work[:] = [(m.copy(), p.copy(), p.copy()) for m, p in zip(dense_in, perms)]

    def run_slice(t):
        for j in range(bounds[t], bounds[t + 1]):
            lp, (m, pos, var) = lps[j], work[j]
            orc.simplex(m, lp[0], lp[1], pos, var, precision=lp[5], max_pivots=lp[6], check_cycles=lp[7])

    with ThreadPoolExecutor(threads) as pool:
        def run():
            if threads == 1:
                run_slice(0)
            else:
                list(pool.map(run_slice, range(threads)))
        ts = []
        for k in range(repeats + 1):  # (the first one is the warm-up)
            prepare()
            t0 = time.perf_counter()
            run()
            ts.append(time.perf_counter() - t0)
    return rate(len(lps), ts[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-sample", type=int, default=512, help="LPs of each workload the single-call loop and the oracle are timed on")
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--classes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_batch_throughput.json"))
    ap.add_argument("--classes-out", default=os.path.join(ROOT, "profiles", "lp_batch_classes.json"))
    args = ap.parse_args()
    orc = _oracle.load()
    if args.classes:
        return classes(args)
    result = {"repeats": args.repeats, "loop_sample": args.loop_sample, "workloads": {}}
    for name, lps in workloads(orc, args.only).items():
        row = {"lps": len(lps), "batch": batch_figure(lps, args.repeats)}
        if not args.no_baselines:
            row["loop"] = loop_figure(lps, args.repeats, args.loop_sample)
            row["oracle_1_core"] = oracle_figure(orc, lps, args.repeats, 1, args.loop_sample)
            row["oracle_16_threads"] = oracle_figure(orc, lps, args.repeats, 16, args.loop_sample)
            a = row["batch"]
            row["batch_beats_loop_and_16_threads_beyond_spread"] = all(
                a["lps_per_s_min"] > row[k]["lps_per_s_max"] for k in ("loop", "oracle_16_threads"))
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) else v) for k, v in row.items()}),
              "with packing", round(row["batch"]["with_packing"]["lps_per_s"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


def classes(args):
    """Same-box table of lane counts and workgroups per CU per LDS class, one dense workload per class."""
    def lps_dense(M, N_, count):
        return [(N_ + 1, M + 1, *N.dense_cells(N.dense_lp(M, N_, 1 + s), N_ + 1, M + 1), 1e-8, 8192.0, False) for s in range(count)]
    table = {"repeats": args.repeats, "rows": []}
    for cls, (M, N_, count, per_cus) in {0: (30, 30, 4096, (8, 4, 2)), 1: (60, 50, 2048, (4, 2)), 2: (96, 80, 2048, (2, 1)),
                                           3: (130, 120, 1024, (1,))}.items():
        lps = lps_dense(M, N_, count)
        for lanes in (256, 1024):
            for per_cu in per_cus:
                if lanes == 1024 and per_cu > 2:
                    continue  # (32 waves per CU: at most two workgroups of 16 waves)
                env = {"YALPS_LPBATCH_LANES": ",".join([str(lanes)] * 4), "YALPS_LPBATCH_PER_CU": ",".join([str(per_cu)] * 5)}
                fig = batch_figure(lps, args.repeats, env)
                row = {"class": cls, "shape": [M, N_], "lps": count, "lds_bytes": B.lds_bytes(N_ + 1, M + 1), "lanes": lanes,
                       "workgroups_per_cu": per_cu, "lps_per_s": fig["lps_per_s"], "lps_per_s_min": fig["lps_per_s_min"],
                       "lps_per_s_max": fig["lps_per_s_max"], "gpu_ms": fig["gpu_ms"]}
                table["rows"].append(row)
                print(json.dumps(row), flush=True)
    out = args.classes_out
    with open(out, "w") as f:
        json.dump(table, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
