"""The insulated singular solve (mg_pcg with the null-space projections) beside the solve with one Dirichlet face on one
MI355X: wall clock with the handle's stream synchronised, the same log-normal kappa, every level above the coarsest
matrix-free, Jacobi V(2,2), P1 transfers, rtol 1e-10 from a zero start.  The two handles take turns, --reps times each after
one untimed call (measuring-on-mi355x: compare in one call, alternating):
  solves      iterations, milliseconds per solve (median, spread) and per iteration
  projection  one Euclidean mean removal of a top-level vector (mg_remove_mean: ns_partial, fcg_fold, ns_subtract, the mean's
              download and the synchronisation) -- what every iteration of the singular solve adds -- in milliseconds, as a
              share of an iteration, and the 24 bytes per row it moves per second beside the 8 TB/s of the HBM

    python tools/time_insulated.py [--json profiles/diffusion_insulated_time.json] [--elements 256] [--levels 6]
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


def summary(ms):
    return {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=256)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "diffusion_insulated_time.json"))
    args = ap.parse_args()
    from multigrid_dolfinx_amd import poisson
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy, _DeviceArray
    N, top = args.elements, args.levels - 1
    n = (N + 1) ** 3
    rng = np.random.default_rng(3)
    kappa = np.exp(rng.standard_normal(N ** 3))
    f = rng.standard_normal(n) + 0.25
    handles = {}
    for name in ("insulated", "x-"):
        h = DeviceHierarchy(3, 0, top, c=N >> top)
        h.set_prolongation("p1")
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        if name == "insulated":
            h.set_diffusion_insulated()
        else:
            h.set_diffusion_faces(("x-",))
        h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0)
        handles[name] = (h, f if name == "insulated" else np.where(poisson.dirichlet_mask(N, ("x-",)), 0.0, f))
    report = {"nodes": "%d^3" % (N + 1), "levels": args.levels, "rtol": args.rtol, "reps": args.reps, "solves": {}}
    ms = {name: [] for name in handles}
    its = {}
    for rep in range(args.reps + 1):                # (the first call allocates, captures and factorises: not timed)
        for name, (h, rhs) in handles.items():
            h.set_vector(top, "f", rhs)
            h.zero_vector(top, "v")
            h.sync()
            t0 = time.perf_counter()
            hist = h.pcg(rtol=args.rtol, max_iter=200, level=top)
            if rep:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            its[name] = len(hist)
    for name in handles:
        report["solves"][name] = dict(summary(ms[name]), iterations=its[name], ms_per_iteration=statistics.median(ms[name]) / max(1, its[name]),
                                      singular=handles[name][0].diffusion_nullspace(top))
        print(name, report["solves"][name], file=sys.stderr, flush=True)
    h = handles["insulated"][0]
    x = _DeviceArray(h._lib, h.device, n, f)
    h.remove_mean(x.ptr.value, n)
    t = []
    for _ in range(4 * args.reps):
        t0 = time.perf_counter()
        h.remove_mean(x.ptr.value, n)
        t.append((time.perf_counter() - t0) * 1e3)
    x.free()
    per_it = report["solves"]["insulated"]["ms_per_iteration"]
    report["projection"] = dict(summary(t), bytes=24 * n, tb_per_s=24 * n / (statistics.median(t) * 1e-3) / 1e12,
                                share_of_an_iteration=statistics.median(t) / per_it)
    print("projection", report["projection"], file=sys.stderr, flush=True)
    for h, _ in handles.values():
        h.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
