"""What free variables cost on the three workloads of tools/lp_dense_throughput.py (4096 x dense-LP(30,30), 2048 x (96,80),
256 x (300,280)), same windowing: per figure the median of `--repeats` timed windows of at least 0.1 s after two warm-up calls,
with min and max, and the kernels' own time per call (HIP events, median) next to it.  Half the variables (the even indices) are
free; each is held by a guard row -x[j] <= 1/2 under A_ub, so that the LPs stay bounded and both routes solve the same LP.

  (a) linprog_batch(c, A, b, free=F): the twins generated on the device
  (b) the route a user had, pre-built outside the clock: the negated columns concatenated behind c and A_ub by torch; inside the
      clock the boundless call on n + f variables and the subtraction of the two halves of x
  (c) the same route with the cat inside the clock
      -- (b) and (c) with the bytes they materialise, (a) with the bytes of the index list
  (d) a boundless and a bounded duals=False call of this build against the parent commit's libraries (--parent-lib FILE, the
      parent's libyalps_lpdense.so with its libyalps_lpdense_bounds.so beside it), alternating: child processes of this tool, this
      build and the parent's library in turn, `--rounds` each, every child the same windows; the figure is the median over a
      side's windows, the spread its min and max.  Skipped without --parent-lib.

Writes profiles/lp_dense_free_throughput.json.

    python tools/lp_dense_free_throughput.py [--repeats 5] [--rounds 2] [--parent-lib FILE] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch  # (before the package's libraries: yalps_amd/tensors.py says why)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch.cuda.init()

from lp_dense_bounds_throughput import box, operands  # noqa: E402
from lp_dense_throughput import WORKLOADS, rate, timed  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import tensors  # noqa: E402

GUARD = 0.5


def freed(M, N_, count):
    """(c, A, b, F): the workload's operands with a guard row per free variable under A_ub; F the even indices."""
    c, A, b = operands(M, N_, count)
    F = list(range(0, N_, 2))
    guard = torch.zeros((len(F), N_), dtype=torch.float64, device="cuda")
    guard[torch.arange(len(F)), torch.tensor(F)] = -1.0
    A = torch.cat([A, guard.expand(count, len(F), N_)], dim=1).contiguous()
    b = torch.cat([b, torch.full((count, len(F)), GUARD, dtype=torch.float64, device="cuda")], dim=1).contiguous()
    return c, A, b, F


def figures(M, N_, count, repeats):
    c, A, b, F = freed(M, N_, count)
    torch.cuda.synchronize()
    ms = {"free": [], "prebuilt": [], "built_in_clock": []}
    held = {}

    def build():
        return torch.cat([c, -c[:, F]], dim=1), torch.cat([A, -A[:, :, F]], dim=2)

    def route(key, c2, A2):
        stats = {}
        out = tensors.linprog_batch(c2, A2, b, maximize=True, stats=stats)
        x = out.x[:, :N_].clone()
        x[:, F] -= out.x[:, N_:]
        held[key] = (x, out.objective, out.status, out.pivots)
        ms[key].append(stats["gpu_ms"])

    def free():
        stats = {}
        held["free"] = tensors.linprog_batch(c, A, b, free=F, maximize=True, stats=stats)
        ms["free"].append(stats["gpu_ms"])
        held["launches"] = [(k["kernel"], k["class"], k["lps"], k["grid"], k["lds"]) for k in stats["kernels"]]

    c2, A2 = build()
    row = {"lps": count, "free_variables": len(F)}
    for key, fn in (("free", free), ("prebuilt", lambda: route("prebuilt", c2, A2)), ("built_in_clock", lambda: route("built_in_clock", *build()))):
        row[key] = rate(count, timed(fn, repeats))
        print("  %dx%d %s: %.0f LPs/s" % (M, N_, key, row[key]["lps_per_s"]), file=sys.stderr, flush=True)
    a, p = held["free"], held["prebuilt"]
    # the same tableaux word for word: the same endings, pivots, x and objectives
    assert bool((a.status == p[2]).all()) and bool((a.pivots == p[3]).all())
    optimal = a.status == 0
    assert bool(torch.equal(a.objective[optimal], p[1][optimal])) and bool(torch.equal(a.x[optimal], p[0][optimal]))
    row.update(optimal=int(optimal.sum()), negative_x=int((a.x[optimal] < 0).any(dim=1).sum()), pivots_mean=float(a.pivots.double().mean()),
               gpu_ms={k: statistics.median(v[2:]) for k, v in ms.items()}, launches=held["launches"],
               operand_bytes=int(8 * (c.numel() + A.numel() + b.numel())), index_bytes=int(4 * len(F)),
               materialised_bytes=int(8 * (A2.numel() + c2.numel())), twin_bytes=int(8 * count * (A.shape[1] + 1) * len(F)))
    for k in ("prebuilt", "built_in_clock"):
        row["free_over_" + k] = row["free"]["lps_per_s"] / row[k]["lps_per_s"]
        row["free_beats_%s_beyond_spread" % k] = row["free"]["lps_per_s_min"] > row[k]["lps_per_s_max"]
        row["%s_beats_free_beyond_spread" % k] = row[k]["lps_per_s_min"] > row["free"]["lps_per_s_max"]
    row["kernel_ms_free_over_prebuilt"] = row["gpu_ms"]["free"] / row["gpu_ms"]["prebuilt"]
    return row


def child(repeats, only):
    """A boundless and a bounded call on whatever library YALPS_LPDENSE_LIB names:
    {"boundless" | "bounded": {workload: {"seconds_per_call": [...], "gpu_ms": x}}}."""
    if os.environ.get("YALPS_LPDENSE_LIB"):  # (the parent's library has no free entries to bind)
        for k in ("validate_free", "solve_free"):
            N._BATCH_LIBS["yalps_lpdense"][1].pop(k, None)
    out = {"boundless": {}, "bounded": {}}
    for name, (M, N_, count) in WORKLOADS.items():
        if only is not None and name not in only:
            continue
        c, A, b = operands(M, N_, count)
        lb, ub = box(N_, count)
        for kind, kw in (("boundless", {}), ("bounded", dict(lb=lb, ub=ub))):
            ms = []

            def fn():
                stats = {}
                tensors.linprog_batch(c, A, b, maximize=True, stats=stats, **kw)
                ms.append(stats["gpu_ms"])
                out[kind].setdefault(name, {})["kernels"] = [k["kernel"] for k in stats["kernels"]]

            ts = timed(fn, repeats)
            out[kind][name].update(seconds_per_call=ts, gpu_ms=statistics.median(ms[2:]), lps=count)
    print("CHILD " + json.dumps(out), flush=True)


def alternate(parent_lib, rounds, repeats, only):
    sides = {"this_build": [], "parent": []}
    for _ in range(rounds):
        for side in ("this_build", "parent"):
            env = dict(os.environ)
            env.pop("YALPS_LPDENSE_LIB", None)
            if side == "parent":
                env["YALPS_LPDENSE_LIB"] = os.path.abspath(parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)] + (["--only", ",".join(only)] if only else [])
            done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if done.returncode != 0:
                raise RuntimeError("%s child failed:\n%s" % (side, done.stderr[-2000:]))
            sides[side].append(json.loads(next(l for l in done.stdout.splitlines() if l.startswith("CHILD "))[6:]))
    result = {}
    for kind in ("boundless", "bounded"):
        result[kind] = {}
        for name in sides["this_build"][0][kind]:
            row = {}
            for side, runs in sides.items():
                ts = [t for r in runs for t in r[kind][name]["seconds_per_call"]]
                row[side] = dict(rate(runs[0][kind][name]["lps"], ts), gpu_ms=[r[kind][name]["gpu_ms"] for r in runs], kernels=runs[0][kind][name]["kernels"])
            a, p = row["this_build"], row["parent"]
            row["this_build_over_parent"] = a["lps_per_s"] / p["lps_per_s"]
            row["spreads_overlap"] = a["lps_per_s_min"] <= p["lps_per_s_max"] and p["lps_per_s_min"] <= a["lps_per_s_max"]
            row["same_kernels"] = a["kernels"] == p["kernels"]
            result[kind][name] = row
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_dense_free_throughput.json"))
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    if args.child:
        return child(args.repeats, only)
    result = {"repeats": args.repeats, "workloads": {}}
    for name, (M, N_, count) in WORKLOADS.items():
        if only is not None and name not in only:
            continue
        row = figures(M, N_, count, args.repeats)
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) and "lps_per_s" in v else v)
                                for k, v in row.items() if k not in ("gpu_ms", "launches")}), flush=True)
    if args.parent_lib:
        result["against_parent"] = dict(rounds=args.rounds, calls=alternate(args.parent_lib, args.rounds, args.repeats, only))
        for kind, rows in result["against_parent"]["calls"].items():
            for name, row in rows.items():
                print(kind, name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
