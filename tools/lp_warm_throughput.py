"""Variants per second of ONE model under moved bounds and objective coefficients, reoptimised from the base's optimal tableau
against solved from the initial one: (a) reoptimize_variants and (b) solve_variants from the model and variant dicts, (c) one
LpWarm.solve (yalps_lpwarm_solve, the base's solve inside the clock) and (d) one LpVariants.solve (yalps_lpvar_solve) of
pre-packed arrays, with the kernels' HIP-event time of (c) and (d) and the pivots all variants took, warm and cold.  The
workloads are those of tools/lp_variants_throughput.py; every variant moves 2..5 bounds and 2..5 objective coefficients by up
to +-1 % ("small") or +-50 % ("large") of their value.  Same box, same run; per figure the median of `--repeats` timed repeats
after one warm-up, with the slowest and the fastest.  Writes profiles/lp_warm_throughput.json.

    python tools/lp_warm_throughput.py [--repeats 5] [--only NAME]
    python tools/lp_warm_throughput.py --pivots-only      (no GPU: the pivot totals alone, by the C oracle)
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

from tests import _lp_variants as V  # noqa: E402
from yalps_amd.model import tableau_model_with_bounds, variant_patch_cells  # noqa: E402

WORKLOADS = {"dense30": (30, 30, 4096), "dense96": (96, 80, 2048), "dense300": (300, 280, 256)}
SIZES = {"small": 0.01, "large": 0.5}


def moved_variants(model, M, N_, count, size, seed=1):
    """Per variant a seeded handful (2..5 each) of bounds and objective coefficients, each scaled by 1 + size * u, u in [-1, 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        rows = rng.choice(M, int(rng.integers(2, 6)), replace=False) + 1
        cols = rng.choice(N_, int(rng.integers(2, 6)), replace=False) + 1
        scale = lambda: 1.0 + size * (2.0 * float(rng.random()) - 1.0)
        out.append({"constraints": {"c%d" % r: {"max": model["constraints"]["c%d" % r]["max"] * scale()} for r in rows},
                    "variables": {"x%d" % j: {"obj": model["variables"]["x%d" % j]["obj"] * scale()} for j in cols}})
    return out


def timed(fn, repeats):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def rate(count, ts):
    return {"variants_per_s": count / statistics.median(ts), "variants_per_s_slowest": count / max(ts),
            "variants_per_s_fastest": count / min(ts), "seconds": ts, "variants": count}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def patches_of(model, variants):
    tabmod, info = tableau_model_with_bounds(model, sparse=True)
    patches = [variant_patch_cells(tabmod, info, v) for v in variants]
    w = tabmod.tableau.width
    assert all(p is not None and all(k < w or k % w == 0 for k, _ in p) for p in patches)
    return tabmod.tableau, patches


def oracle_pivots(oracle, model, variants):
    """(warm, cold, base, cut) by the C oracle: the pivots of every variant from tests/_np_warm.py's warm tableau and from its
    own initial tableau, the base's, and how many warm variants ran into maxPivots."""
    from tests import _np_warm as NW
    t, patches = patches_of(model, variants)
    w, h = t.width, t.height
    base, b0 = NW.solve_base(oracle, t.cells, w, h), NW.edge_cells(t.cells, w)
    assert base["status"] == "optimal"
    warm = cold = cut = 0
    start = NW.dense_of(t.cells, w, h)
    for patch in patches:
        answer = NW.warm_answer(oracle, base, w, h, b0, patch)
        warm += answer["n_pivots"]
        cut += answer["status"] == "cycled"
        m = start.copy()
        for k, v in patch:
            m[k] = v
        pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
        cold += oracle.simplex(m, w, h, pos, var)[2]
    return warm, cold, base["n_pivots"], cut


def workload(name, size, repeats):
    from yalps_amd import _native as N
    from yalps_amd import solve as S
    M, N_, count = WORKLOADS[name]
    model = V.dense_model(N, M, N_, 1, holes=False)
    variants = moved_variants(model, M, N_, count, SIZES[size])
    row = {"shape": [M, N_], "variants": count, "perturbation": SIZES[size]}

    stats = {}
    row["reoptimize_variants"] = rate(count, timed(lambda: S.reoptimize_variants(model, variants, None, None, stats), repeats))
    assert (stats["warm"], stats["cold"], stats["base_status"]) == (count, 0, "optimal"), stats
    row["routing"] = {k: stats[k] for k in ("warm", "cold", "base_pivots", "launches", "reruns")}
    row["kernels"] = [(k["kernel"], k["class"], k["lps"], k["grid"], k["lds"]) for k in stats["kernels"]]
    cold_stats = {}
    row["solve_variants"] = rate(count, timed(lambda: S.solve_variants(model, variants, None, cold_stats), repeats))
    assert (cold_stats["patched"], cold_stats["materialised"]) == (count, 0), cold_stats

    t, patches = patches_of(model, variants)
    w = t.width
    as_arrays = [(np.array([k // w for k, _ in p], np.int32), np.array([k % w for k, _ in p], np.int32),
                  np.array([v for _, v in p], np.float64)) for p in patches]
    warm_packed = N.PackedWarm(w, t.height, *t.cells, as_arrays)
    cold_packed = N.PackedVariants(w, t.height, *t.cells, as_arrays)
    lw, lv = N.LpWarm(0), N.LpVariants(0)
    try:
        ms = []
        row["lpwarm_prepacked"] = rate(count, timed(lambda: ms.append(lw.solve(warm_packed)[3]), repeats))
        row["lpwarm_gpu_ms"] = spread(ms[1:])
        warm_status, warm_result, warm_pivots, _ = lw.solve(warm_packed)
        ms = []
        row["lpvariants_prepacked"] = rate(count, timed(lambda: ms.append(lv.solve(cold_packed)[3]), repeats))
        row["lpvariants_gpu_ms"] = spread(ms[1:])
        cold_status, cold_result, cold_pivots, _ = lv.solve(cold_packed)
    finally:
        lw.close()
        lv.close()
    row["pivots"] = {"warm": int(warm_pivots.sum()), "cold": int(cold_pivots.sum()), "base": int(lw.base[2])}
    row["warm_statuses"] = {k: warm_status.count(k) for k in sorted(set(warm_status))}
    row["same_status"] = int(sum(a == b for a, b in zip(warm_status, cold_status)))
    row["same_result_bits"] = int((warm_result.view(np.int64) == cold_result.view(np.int64)).sum())
    row["largest_relative_result_difference"] = float(np.nanmax(np.abs(warm_result - cold_result) / np.maximum(np.abs(cold_result), 1.0)))
    row["reoptimize_beats_solve_variants_beyond_spread"] = \
        row["reoptimize_variants"]["variants_per_s_slowest"] > row["solve_variants"]["variants_per_s_fastest"]
    row["lpwarm_beats_lpvariants_beyond_spread"] = \
        row["lpwarm_prepacked"]["variants_per_s_slowest"] > row["lpvariants_prepacked"]["variants_per_s_fastest"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--pivots-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_warm_throughput.json"))
    args = ap.parse_args()
    if args.pivots_only:
        from tests import _oracle
        oracle = _oracle.load()
        more = []
        for name, (M, N_, count) in WORKLOADS.items():
            model = V.dense_model(oracle, M, N_, 1, holes=False)
            for size in SIZES:
                warm, cold, base, cut = oracle_pivots(oracle, model, moved_variants(model, M, N_, count, SIZES[size]))
                print("%s %s: %d pivots warm, %d cold (base %d, %d variants, %d warm variants ran into maxPivots)" % (
                    name, size, warm, cold, base, count, cut), flush=True)
                if warm >= cold:
                    more.append("%s %s" % (name, size))
        if more:
            raise SystemExit("more pivots warm than cold: " + ", ".join(more))
        return
    result = {"repeats": args.repeats, "workloads": {}}
    for name in WORKLOADS:
        if args.only not in (None, name):
            continue
        for size in SIZES:
            row = workload(name, size, args.repeats)
            result["workloads"]["%s %s" % (name, size)] = row
            print(name, size, json.dumps({k: (round(v["variants_per_s"]) if isinstance(v, dict) and "variants_per_s" in v else v)
                                          for k, v in row.items() if k != "kernels"}), flush=True)
            with open(args.out, "w") as f:  # (after every workload: a run cut short keeps what it measured)
                json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
