"""Variants per second of ONE model solved under many right-hand sides and objective coefficients: (a) solve_variants from
the model and variant dicts, (b) one LpVariants.solve (yalps_lpvar_solve) of pre-packed arrays, (c) what a user wrote before
solve_variants existed -- solve_many on the materialised models (apply_variant outside the clock), (d) one LpBatch.solve of
the same LPs as full cell lists, with the packing of the per-LP arrays inside the clock, and the kernels' HIP-event time
(gpu_ms) of (b) and (d): the image start against the zero pass plus cell scatter on kernel time alone.  Same box, same run;
per figure the median of `--repeats` timed repeats after one warm-up, with min and max.  Writes
profiles/lp_variants_throughput.json.

    python tools/lp_variants_throughput.py [--repeats 5] [--only NAME]
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
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import solve as S  # noqa: E402
from yalps_amd.model import apply_variant, tableau_model  # noqa: E402

WORKLOADS = {"dense30": (30, 30, 4096), "dense96": (96, 80, 2048), "dense300": (300, 280, 256)}


def seeded_variants(M, N_, count, seed=1):
    """Per variant a seeded handful (2..5 each) of right-hand sides and objective coefficients."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        rows = rng.choice(M, int(rng.integers(2, 6)), replace=False) + 1
        cols = rng.choice(N_, int(rng.integers(2, 6)), replace=False) + 1
        out.append({"constraints": {"c%d" % r: {"max": float(N_) * 0.25 * (1.0 + float(rng.random()))} for r in rows},
                    "variables": {"x%d" % j: {"obj": float(rng.random())} for j in cols}})
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
    return {"lps_per_s": count / statistics.median(ts), "lps_per_s_min": count / max(ts), "lps_per_s_max": count / min(ts),
            "seconds": ts, "lps": count}


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def workload(name, repeats):
    M, N_, count = WORKLOADS[name]
    model = V.dense_model(N, M, N_, 1, holes=False)
    variants = seeded_variants(M, N_, count)
    row = {"shape": [M, N_], "variants": count}

    stats = {}
    S.solve_variants(model, variants[:4], None, stats)
    assert (stats["patched"], stats["materialised"]) == (4, 0), stats
    row["solve_variants"] = rate(count, timed(lambda: S.solve_variants(model, variants, None, stats), repeats))
    row["routing"] = {k: stats[k] for k in ("patched", "materialised", "base_cells", "patch_cells", "launches", "reruns")}
    row["kernels"] = [(k["kernel"], k["class"], k["lps"], k["grid"], k["lds"]) for k in stats["kernels"]]

    packed = V.packed(N, model, variants)
    lv = N.LpVariants(0)
    try:
        ms = []
        row["lpvariants_prepacked"] = rate(count, timed(lambda: ms.append(lv.solve(packed)[3]), repeats))
        row["lpvariants_gpu_ms"] = spread(ms[1:])
        ref_status, ref_result = lv.solve(packed)[:2]
    finally:
        lv.close()

    models = [apply_variant(model, v) for v in variants]
    many_stats = {}
    row["solve_many_materialised"] = rate(count, timed(lambda: S.solve_many(models, None, many_stats), repeats))
    assert many_stats["batched"] == count, many_stats

    lps = []
    for m in models:
        t = tableau_model(m, sparse=True).tableau
        lps.append((t.width, t.height, *t.cells, 1e-8, 8192.0, False))
    b = N.LpBatch(0)
    try:
        row["lpbatch_with_packing"] = rate(count, timed(lambda: b.solve(N.PackedLps(lps)), repeats))
        pre = N.PackedLps(lps)
        ms = []
        row["lpbatch_prepacked"] = rate(count, timed(lambda: ms.append(b.solve(pre)[3]), repeats))
        row["lpbatch_gpu_ms"] = spread(ms[1:])
        status, result = b.solve(pre)[:2]
    finally:
        b.close()
    # (the two libraries solved the same LPs: same endings, same objective bits)
    assert status == ref_status and np.array_equal(result.view(np.int64), ref_result.view(np.int64))

    row["solve_variants_beats_solve_many_beyond_spread"] = \
        row["solve_variants"]["lps_per_s_min"] > row["solve_many_materialised"]["lps_per_s_max"]
    row["image_start_gpu_ms_over_cell_scatter_gpu_ms"] = row["lpvariants_gpu_ms"]["median"] / row["lpbatch_gpu_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_variants_throughput.json"))
    args = ap.parse_args()
    result = {"repeats": args.repeats, "workloads": {}}
    for name in WORKLOADS:
        if args.only not in (None, name):
            continue
        row = workload(name, args.repeats)
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) and "lps_per_s" in v else v)
                                for k, v in row.items() if k != "kernels"}), flush=True)
        with open(args.out, "w") as f:  # (after every workload: a run cut short keeps what it measured)
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
