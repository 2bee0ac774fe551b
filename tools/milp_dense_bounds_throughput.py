"""What variable bounds cost in milp_batch on the three packing workloads of tools/milp_dense_throughput.py (2048 small trees,
512 x packing(60, 60, 6), 256 x packing(100, 100, 6)), same windowing: per figure the median of `--repeats` timed windows of at
least 0.1 s after two warm-up calls, with min and max, and the kernels' own time per call (HIP events, median) split into root
pass, tree pass and epilogue.  Every integer variable gets a box: a per-MILP lb [B, n] -- negative quarters at the integer
variables, which rule 1 rounds up to -1.0 or -0.0, negative eighths at the others -- and a shared ub [n], read at the integer
variables (`upper` = the integer set).

  (a) milp_batch(c, A, b, lb=lb, ub=ub, upper=integers): the bounds shifted and built on the device
  (b) the only route the parent commit offers, pre-built outside the clock: the identity block of the boxed variables
      concatenated under A_ub, b shifted by torch (b - A l, ub - l, l = ceil(lb) at the integer variables); inside the clock the
      boundless call, x + l and objective + c . l
  (c) the same route with the cat and the shift inside the clock
      -- (b) and (c) with the bytes they materialise, (a) with the bytes of lb and ub
  (d) a boundless call of this build against the parent commit's library (--parent-lib FILE), alternating: child processes of
      this tool, this build and the parent's library in turn, `--rounds` each, every child the same windows; the figure is the
      median over a side's windows, the spread its min and max.  Skipped without --parent-lib.

Writes profiles/milp_dense_bounds_throughput.json.

    python tools/milp_dense_bounds_throughput.py [--repeats 5] [--rounds 2] [--parent-lib FILE] [--only NAME[,NAME]] [--out FILE]
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

torch.cuda.init()

from tests import _np_milp_dense as NM  # noqa: E402
from tools.lp_dense_throughput import timed  # noqa: E402
from tools.milp_dense_throughput import WORKLOADS, rate  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import tensors  # noqa: E402

PARTS = ("root_ms", "tree_ms", "epilogue_ms", "gpu_ms")


def operands(m, n, n_int, seed0, count):
    made = [NM.packing_dense(m, n, n_int, seed0 + s) for s in range(count)]
    c, A, b = (torch.from_numpy(np.stack([lp[k] for lp, _ in made])).cuda() for k in range(3))
    return c, A, b, made[0][1]


def box(n, count, ints):
    rng = np.random.default_rng([20261307, n, count])
    lb = -rng.integers(0, 5, (count, n)).astype(np.float64) / 8.0
    lb[:, ints] = -rng.integers(0, 5, (count, len(ints))).astype(np.float64) / 4.0
    ub = 1.0 + rng.integers(0, 4, n).astype(np.float64)
    return torch.from_numpy(lb).cuda(), torch.from_numpy(ub).cuda()


def figures(m, n, n_int, seed0, count, repeats):
    c, A, b, ints = operands(m, n, n_int, seed0, count)
    lb, ub = box(n, count, ints)
    k = len(ints)
    unit = torch.eye(n, dtype=torch.float64, device="cuda")[ints]
    torch.cuda.synchronize()
    ms = {key: {p: [] for p in PARTS} for key in ("bounded", "prebuilt", "built_in_clock")}
    held = {}

    def note(key, stats):
        for p in PARTS:
            ms[key][p].append(stats[p])

    def build():
        low = lb.clone()
        low[:, ints] = torch.ceil(lb[:, ints])
        A2 = torch.cat([A, unit.expand(count, k, n)], dim=1)
        b2 = torch.cat([b - (A @ low.unsqueeze(2)).squeeze(2), (ub - low)[:, ints]], dim=1)
        return A2, b2, low

    def route(key, A2, b2, low):
        stats = {}
        out = tensors.milp_batch(c, A2, b2, integers=ints, maximize=True, stats=stats)
        held[key] = (out.x + low, out.objective + (c * low).sum(1), out.status, out.nodes)
        note(key, stats)

    def bounded():
        stats = {}
        held["bounded"] = tensors.milp_batch(c, A, b, lb=lb, ub=ub, upper=ints, integers=ints, maximize=True, stats=stats)
        note("bounded", stats)
        held["launches"] = [(q["kernel"], q["class"], q.get("lps", q.get("trees")), q["grid"], q["lds"]) for q in stats["kernels"]]
        held["overflows"] = stats["overflows"]

    A2, b2, low = build()
    row = {"milps": count, "shape": [m, n, n_int], "bound_rows": k}
    for key, fn in (("bounded", bounded), ("prebuilt", lambda: route("prebuilt", A2, b2, low)), ("built_in_clock", lambda: route("built_in_clock", *build()))):
        row[key] = rate(count, timed(fn, repeats))
        print("  %dx%d %s: %.0f MILPs/s" % (m, n, key, row[key]["milps_per_s"]), file=sys.stderr, flush=True)
    a, p = held["bounded"], held["prebuilt"]
    # the same MILPs but for the place of the unit rows and the order in which b's shift is summed: the same endings, and
    # objectives that agree to rounding
    same = a.status == p[2]
    optimal = (a.status == 0) & same
    assert float(same.double().mean()) > 0.9, float(same.double().mean())  # (reported as same_status)
    assert bool(torch.allclose(a.objective[optimal], p[1][optimal], rtol=1e-9, atol=1e-7))
    med = lambda v: statistics.median(v[2:])
    row.update(optimal=int((a.status == 0).sum()), same_status=float(same.double().mean()), nodes_used=int(a.nodes.sum()),
               nodes_used_prebuilt=int(p[3].sum()), longest_tree=int(a.nodes.max()), overflows=int(held["overflows"]),
               gpu_ms={key: {q: med(v) for q, v in parts.items()} for key, parts in ms.items()},
               gpu_ms_spread={key: {q: [min(v[2:]), max(v[2:])] for q, v in parts.items()} for key, parts in ms.items()},
               launches=held["launches"], operand_bytes=int(8 * (c.numel() + A.numel() + b.numel())),
               bound_bytes=int(8 * (lb.numel() + ub.numel())), materialised_bytes=int(8 * (A2.numel() + b2.numel() + low.numel())),
               identity_bytes=int(8 * count * k * n))
    for key in ("prebuilt", "built_in_clock"):
        row["bounded_over_" + key] = row["bounded"]["milps_per_s"] / row[key]["milps_per_s"]
        row["bounded_beats_%s_beyond_spread" % key] = row["bounded"]["milps_per_s_min"] > row[key]["milps_per_s_max"]
        row["bounded_loses_to_%s_beyond_spread" % key] = row["bounded"]["milps_per_s_max"] < row[key]["milps_per_s_min"]
    for q in PARTS:
        row["kernel_%s_bounded_over_prebuilt" % q] = row["gpu_ms"]["bounded"][q] / row["gpu_ms"]["prebuilt"][q]
    return row


def child(repeats, only):
    """The boundless call on whatever library YALPS_MILPDENSE_LIB names: {workload: {"seconds_per_call": [...], parts}}."""
    if os.environ.get("YALPS_MILPDENSE_LIB"):  # (the parent's library has no bounds entries to bind)
        for key in ("validate_bounds", "solve_bounds"):
            N._BATCH_LIBS["yalps_milpdense"][1].pop(key, None)
    out = {}
    for name, spec in WORKLOADS.items():
        if only is not None and name not in only:
            continue
        c, A, b, ints = operands(*spec)
        ms = {p: [] for p in PARTS}

        def fn():
            stats = {}
            tensors.milp_batch(c, A, b, integers=ints, maximize=True, stats=stats)
            for p in PARTS:
                ms[p].append(stats[p])
            out.setdefault(name, {})["kernels"] = [q["kernel"] for q in stats["kernels"]]

        ts = timed(fn, repeats)
        out[name].update(seconds_per_call=ts, milps=spec[-1], **{p: statistics.median(v[2:]) for p, v in ms.items()})
    print("CHILD " + json.dumps(out), flush=True)


def alternate(parent_lib, rounds, repeats, only):
    sides = {"this_build": [], "parent": []}
    for _ in range(rounds):
        for side in ("this_build", "parent"):
            env = dict(os.environ)
            env.pop("YALPS_MILPDENSE_LIB", None)
            if side == "parent":
                env["YALPS_MILPDENSE_LIB"] = os.path.abspath(parent_lib)
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
            row[side] = dict(rate(runs[0][name]["milps"], ts), kernels=runs[0][name]["kernels"], **{p: [r[name][p] for r in runs] for p in PARTS})
        a, p = row["this_build"], row["parent"]
        row["this_build_over_parent"] = a["milps_per_s"] / p["milps_per_s"]
        row["spreads_overlap"] = a["milps_per_s_min"] <= p["milps_per_s_max"] and p["milps_per_s_min"] <= a["milps_per_s_max"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "milp_dense_bounds_throughput.json"))
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    if args.child:
        return child(args.repeats, only)
    result = {"tool": "tools/milp_dense_bounds_throughput.py", "repeats": args.repeats, "workloads": {}}

    def write():
        with open(args.out, "w") as f:  # (after every step: a run that is cut short leaves what it measured)
            json.dump(result, f, indent=1)
            f.write("\n")

    for name, spec in WORKLOADS.items():
        if only is not None and name not in only:
            continue
        row = figures(*spec, args.repeats)
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["milps_per_s"]) if isinstance(v, dict) and "milps_per_s" in v else v)
                                for k, v in row.items() if k not in ("gpu_ms_spread", "launches")}), flush=True)
        write()
    if args.parent_lib:
        result["boundless_against_parent"] = dict(rounds=args.rounds, workloads=alternate(args.parent_lib, args.rounds, args.repeats, only))
        for name, row in result["boundless_against_parent"]["workloads"].items():
            print("boundless", name, json.dumps({k: (round(v["milps_per_s"]) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
        write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
