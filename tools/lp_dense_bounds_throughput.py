"""What variable bounds cost on the three workloads of tools/lp_dense_throughput.py (4096 x dense-LP(30,30), 2048 x (96,80),
256 x (300,280)), same windowing: per figure the median of `--repeats` timed windows of at least 0.1 s after two warm-up calls,
with min and max, and the kernels' own time per call (HIP events, median) next to it.  Every variable gets a box: a per-LP
lb [B, n] (negative eighths, so that x = lb stays feasible) and a shared ub [n].

  (a) linprog_batch(c, A, b, lb=lb, ub=ub): the bounds shifted and built on the device
  (b) the route a user had, pre-built outside the clock: the identity block concatenated under A_ub, b shifted by torch
      (b - A lb, ub - lb); inside the clock the boundless call, x + lb and objective + c . lb
  (c) the same route with the cat and the shift inside the clock
      -- (b) and (c) with the bytes they materialise, (a) with the bytes of lb and ub
  (d) a boundless duals=False call of this build against the parent commit's library (--parent-lib FILE), alternating: child
      processes of this tool, this build and the parent's library in turn, `--rounds` each, every child the same windows; the
      figure is the median over a side's windows, the spread its min and max.  Skipped without --parent-lib.

Writes profiles/lp_dense_bounds_throughput.json.

    python tools/lp_dense_bounds_throughput.py [--repeats 5] [--rounds 2] [--parent-lib FILE] [--only NAME[,NAME]] [--out FILE]
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

from lp_dense_throughput import WORKLOADS, rate, timed  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import tensors  # noqa: E402


def operands(M, N_, count):
    w, h = N_ + 1, M + 1
    T = np.stack([N.dense_lp(M, N_, 1 + s) for s in range(count)]).reshape(count, h, w)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (T[:, 0, 1:], T[:, 1:, 1:], T[:, 1:, 0]))


def box(N_, count):
    rng = np.random.default_rng([20261108, N_, count])
    lb = -rng.integers(0, 5, (count, N_)).astype(np.float64) / 8.0
    ub = 0.5 + rng.integers(0, 5, N_).astype(np.float64) / 4.0
    return torch.from_numpy(lb).cuda(), torch.from_numpy(ub).cuda()


def figures(M, N_, count, repeats):
    c, A, b = operands(M, N_, count)
    lb, ub = box(N_, count)
    eye = torch.eye(N_, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ms = {"bounded": [], "prebuilt": [], "built_in_clock": []}
    held = {}

    def build():
        A2 = torch.cat([A, eye.expand(count, N_, N_)], dim=1)
        b2 = torch.cat([b - (A @ lb.unsqueeze(2)).squeeze(2), (ub - lb)], dim=1)
        return A2, b2

    def route(key, A2, b2):
        stats = {}
        out = tensors.linprog_batch(c, A2, b2, maximize=True, stats=stats)
        held[key] = (out.x + lb, out.objective + (c * lb).sum(1), out.status, out.pivots)
        ms[key].append(stats["gpu_ms"])

    def bounded():
        stats = {}
        held["bounded"] = tensors.linprog_batch(c, A, b, lb=lb, ub=ub, maximize=True, stats=stats)
        ms["bounded"].append(stats["gpu_ms"])
        held["launches"] = [(k["kernel"], k["class"], k["lps"], k["grid"], k["lds"]) for k in stats["kernels"]]

    A2, b2 = build()
    row = {"lps": count}
    for key, fn in (("bounded", bounded), ("prebuilt", lambda: route("prebuilt", A2, b2)), ("built_in_clock", lambda: route("built_in_clock", *build()))):
        row[key] = rate(count, timed(fn, repeats))
        print("  %dx%d %s: %.0f LPs/s" % (M, N_, key, row[key]["lps_per_s"]), file=sys.stderr, flush=True)
    a, p = held["bounded"], held["prebuilt"]
    # the same tableaux but for the order in which b's shift is summed: the same endings, and objectives that agree to rounding
    same = a.status == p[2]
    optimal = (a.status == 0) & same
    assert float(same.double().mean()) > 0.9, float(same.double().mean())  # (reported as same_status)
    assert bool(torch.allclose(a.objective[optimal], p[1][optimal], rtol=1e-9, atol=1e-7))
    row.update(optimal=int((a.status == 0).sum()), same_status=float(same.double().mean()), pivots_mean=float(a.pivots.double().mean()),
               gpu_ms={k: statistics.median(v[2:]) for k, v in ms.items()}, launches=held["launches"],
               operand_bytes=int(8 * (c.numel() + A.numel() + b.numel())), bound_bytes=int(8 * (lb.numel() + ub.numel())),
               materialised_bytes=int(8 * (A2.numel() + b2.numel())), identity_bytes=int(8 * count * N_ * N_))
    for k in ("prebuilt", "built_in_clock"):
        row["bounded_over_" + k] = row["bounded"]["lps_per_s"] / row[k]["lps_per_s"]
        row["bounded_beats_%s_beyond_spread" % k] = row["bounded"]["lps_per_s_min"] > row[k]["lps_per_s_max"]
    row["kernel_ms_bounded_over_prebuilt"] = row["gpu_ms"]["bounded"] / row["gpu_ms"]["prebuilt"]
    return row


def child(repeats, only):
    """The boundless call on whatever library YALPS_LPDENSE_LIB names: {workload: {"seconds_per_call": [...], "gpu_ms": x}}."""
    if os.environ.get("YALPS_LPDENSE_LIB"):  # (the parent's library has no bounds entries to bind)
        for k in ("validate_bounds", "solve_bounds"):
            N._BATCH_LIBS["yalps_lpdense"][1].pop(k, None)
    out = {}
    for name, (M, N_, count) in WORKLOADS.items():
        if only is not None and name not in only:
            continue
        c, A, b = operands(M, N_, count)
        ms = []

        def fn():
            stats = {}
            tensors.linprog_batch(c, A, b, maximize=True, stats=stats)
            ms.append(stats["gpu_ms"])
            out.setdefault(name, {})["kernels"] = [k["kernel"] for k in stats["kernels"]]

        ts = timed(fn, repeats)
        out[name].update(seconds_per_call=ts, gpu_ms=statistics.median(ms[2:]), lps=count)
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
    for name in sides["this_build"][0]:
        row = {}
        for side, runs in sides.items():
            ts = [t for r in runs for t in r[name]["seconds_per_call"]]
            row[side] = dict(rate(runs[0][name]["lps"], ts), gpu_ms=[r[name]["gpu_ms"] for r in runs], kernels=runs[0][name]["kernels"])
        a, p = row["this_build"], row["parent"]
        row["this_build_over_parent"] = a["lps_per_s"] / p["lps_per_s"]
        row["spreads_overlap"] = a["lps_per_s_min"] <= p["lps_per_s_max"] and p["lps_per_s_min"] <= a["lps_per_s_max"]
        row["same_kernels"] = a["kernels"] == p["kernels"]
        result[name] = row
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_dense_bounds_throughput.json"))
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
        result["boundless_against_parent"] = dict(rounds=args.rounds, workloads=alternate(args.parent_lib, args.rounds, args.repeats, only))
        for name, row in result["boundless_against_parent"]["workloads"].items():
            print("boundless", name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
