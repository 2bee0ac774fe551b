"""What the dual solution costs on the three workloads of tools/lp_dense_throughput.py (4096 x dense-LP(30,30), 2048 x (96,80),
256 x (300,280)), same windowing: per figure the median of `--repeats` timed windows of at least 0.1 s after two warm-up calls,
with min and max, and the kernels' own time per call (HIP events, median) next to it.

  (a) linprog_batch(duals=False) on this build, next to the parent commit's figure in profiles/lp_dense_throughput.json: the
      "nothing changed" check (the spreads overlap, or the distance is reported)
  (b) linprog_batch(duals=True)
  (c) what a tensor user paid for duals before: sensitivity_many on the equivalent models of the first 512 LPs (the copy of the
      tensors to the host not counted)
  (d) one linprog_objective forward plus backward with all five operands requiring grad (the LPs have no equalities: A_eq and
      b_eq are given with one row 0 . x = 0 so that they take part)

Writes profiles/lp_dense_duals_throughput.json.

    python tools/lp_dense_duals_throughput.py [--repeats 5] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
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
from yalps_amd.sensitivity import sensitivity_many  # noqa: E402

SENS_LPS = 512
PARENT = os.path.join(ROOT, "profiles", "lp_dense_throughput.json")


def equivalent_model(c, A, b):
    """The maximising model of one LP without equalities: constraints u0.. {"max"}, every variable listing every coefficient."""
    m, n = A.shape
    return {"direction": "maximize", "objective": "obj", "constraints": {"u%d" % i: {"max": float(b[i])} for i in range(m)},
            "variables": {"x%d" % j: {"obj": float(c[j]), **{"u%d" % i: float(A[i, j]) for i in range(m)}} for j in range(n)}}


def figures(M, N_, count, repeats, parent):
    w, h = N_ + 1, M + 1
    T = np.stack([N.dense_lp(M, N_, 1 + s) for s in range(count)]).reshape(count, h, w)
    host = [np.ascontiguousarray(a) for a in (T[:, 0, 1:], T[:, 1:, 1:], T[:, 1:, 0])]
    c, A, b = (torch.from_numpy(a).cuda() for a in host)
    models = [equivalent_model(host[0][i], host[1][i], host[2][i]) for i in range(min(count, SENS_LPS))]
    leaves = [t.clone().requires_grad_() for t in (c, A, b)]
    leaves += [torch.zeros((count, 1, N_), dtype=torch.float64, device="cuda", requires_grad=True),
               torch.zeros((count, 1), dtype=torch.float64, device="cuda", requires_grad=True)]
    ones = torch.ones((count,), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ms = {"off": [], "on": []}
    held = {}

    def off():
        stats = {}
        held["off"] = tensors.linprog_batch(c, A, b, maximize=True, stats=stats)
        ms["off"].append(stats["gpu_ms"])

    def on():
        stats = {}
        held["on"] = tensors.linprog_batch(c, A, b, maximize=True, stats=stats, duals=True)
        ms["on"].append(stats["gpu_ms"])

    def sens():
        held["sens"] = sensitivity_many(models)

    def grad():
        for t in leaves:
            t.grad = None
        objective, held["grad"] = tensors.linprog_objective(*leaves, maximize=True)
        objective.backward(ones)
        torch.cuda.synchronize()

    row = {"lps": count}
    for key, fn, lps in (("duals_off", off, count), ("duals_on", on, count), ("objective_forward_backward", grad, count),
                         ("sensitivity_many", sens, len(models))):
        row[key] = rate(lps, timed(fn, repeats))
        print("  %dx%d %s: %.0f LPs/s" % (M, N_, key, row[key]["lps_per_s"]), file=sys.stderr, flush=True)
    a, d = held["off"], held["on"]
    assert all(torch.equal(p, q) for p, q in zip(a, d[:4]))
    optimal = d.status == 0
    gap = (d.objective - (d.ineqlin * b).sum(1)).abs()[optimal]
    assert bool((gap <= 1e-8 + 1e-12 * (d.ineqlin * b).abs().sum(1)[optimal]).all())
    for i, s in enumerate(held["sens"][:8]):  # the old route's duals are the new route's
        if s["status"] == "optimal":
            assert [v["dual"] for _, v in s["sensitivity"]["constraints"]] == d.ineqlin[i].tolist()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in leaves)
    row.update(optimal=int(optimal.sum()), gpu_ms={k: statistics.median(v[2:]) for k, v in ms.items()})
    row["gpu_ms_on_over_off"] = row["gpu_ms"]["on"] / row["gpu_ms"]["off"]
    row["duals_on_over_off"] = row["duals_on"]["lps_per_s"] / row["duals_off"]["lps_per_s"]
    row["duals_on_over_sensitivity_many"] = row["duals_on"]["lps_per_s"] / row["sensitivity_many"]["lps_per_s"]
    if parent is not None:
        p, q = parent["linprog_batch"], row["duals_off"]
        row["parent_linprog_batch"] = {k: p[k] for k in ("lps_per_s", "lps_per_s_min", "lps_per_s_max")}
        row["parent_gpu_ms"] = parent["gpu_ms"]["linprog_batch"]
        row["duals_off_over_parent"] = q["lps_per_s"] / p["lps_per_s"]
        row["spreads_overlap"] = q["lps_per_s_min"] <= p["lps_per_s_max"] and p["lps_per_s_min"] <= q["lps_per_s_max"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lp_dense_duals_throughput.json"))
    args = ap.parse_args()
    parent = json.load(open(PARENT))["workloads"] if os.path.exists(PARENT) else {}
    result = {"repeats": args.repeats, "sensitivity_many_lps": SENS_LPS, "workloads": {}}
    for name, (M, N_, count) in WORKLOADS.items():
        if args.only is not None and name not in args.only.split(","):
            continue
        row = figures(M, N_, count, args.repeats, parent.get(name))
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["lps_per_s"]) if isinstance(v, dict) and "lps_per_s" in v else v) for k, v in row.items()}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
