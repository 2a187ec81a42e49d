"""mg_eigs (smallest eigenpairs by multigrid LOBPCG) and its two block kernels on one MI355X, wall clock with the handle's
stream synchronised, log-normal kappa, every level above the coarsest matrix-free, Jacobi V(2,2), P1 transfers:
  eigs     k = 4 with a block of 6, rtol 1e-8, from a cold start: iterations, restarts, the residuals, milliseconds per call
           (median of --reps, spread) and per iteration, and the work vectors' bytes, at 65^3, 129^3 and 257^3 nodes
  kernels  mg_block_gram 4 x 4 (weighted and not) and 1 x 1, mg_block_combine (18, 6) and (12, 6) on the finest level: the
           milliseconds of one call (launch, fold, the download or the synchronisation) and the bytes the kernel moves per
           second, 8 (NA + NB (+ 1)) and 8 (NS + NO) per row, beside the 8 TB/s of the HBM

    python tools/time_eigs.py [--json profiles/diffusion_eigs_time.json] [--elements 64 128 256]
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
    ap.add_argument("--elements", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "diffusion_eigs_time.json"))
    args = ap.parse_args()
    from multigrid_dolfinx_amd import _capi
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy, _DeviceArray
    report = {"k": 4, "block": 6, "rtol": 1e-8, "reps": args.reps, "sizes": {}}
    for N in args.elements:
        levels = int(np.log2(N)) - 1            # coarsest level: 4 cells per dimension
        top = levels - 1
        n = (N + 1) ** 3
        kappa = np.exp(np.random.default_rng(3).standard_normal(N ** 3))
        h = DeviceHierarchy(3, 0, top, c=N >> top)
        h.set_prolongation("p1")
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0)
        xs = [_DeviceArray(h._lib, h.device, n) for _ in range(24)]
        ptrs = [a.ptr.value for a in xs]
        out = report["sizes"]["%d^3" % (N + 1)] = {"levels": levels}
        ms = []
        try:
            for rep in range(args.reps + 1):        # (the first call allocates: not timed)
                t0 = time.perf_counter()
                res = h.eigs(4, 6, x_ptrs=ptrs[:6], rtol=1e-8, max_iter=100)
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
        except _capi.MgError as e:                  # (a size the iteration does not survive is a result too)
            out["eigs"] = {"error": str(e)}
            print(N + 1, out["eigs"], file=sys.stderr, flush=True)
            h.close()
            continue
        out["eigs"] = dict(summary(ms), iterations=res["iterations"], restarts=res["restarts"], resid=[float(r) for r in res["resid"]],
                           ms_per_iteration=statistics.median(ms) / max(1, res["iterations"]),
                           **{"lambda": [float(v) for v in res["lambda"]]}, work_bytes=h.eigs_info()["bytes"], lane_bytes=h.batch_info()["bytes"])
        print(N + 1, out["eigs"], file=sys.stderr, flush=True)
        # the kernels: the Ritz vectors are as good an operand as any (18 more vectors from combinations of them)
        coeff = np.random.default_rng(1).standard_normal((6, 6))
        for q in (6, 12, 18):
            h.block_combine(ptrs[:6], coeff, ptrs[q:q + 6])
        kernels = out["kernels"] = {}
        calls = {
            "gram_1x1": (lambda: h.block_gram(ptrs[:1], ptrs[1:2]), 2),
            "gram_4x4": (lambda: h.block_gram(ptrs[:4], ptrs[4:8]), 8),
            "gram_4x4_weighted": (lambda: h.block_gram(ptrs[:4], ptrs[4:8], ptrs[8]), 9),
            "combine_12_6": (lambda: h.block_combine(ptrs[:12], np.ones((12, 6)) / 12, ptrs[18:24]), 18),
            "combine_18_6": (lambda: h.block_combine(ptrs[:18], np.ones((18, 6)) / 18, ptrs[18:24]), 24),
        }
        for name, (call, streams) in calls.items():
            call()
            t = []
            for _ in range(4 * args.reps):
                t0 = time.perf_counter()
                call()
                t.append((time.perf_counter() - t0) * 1e3)
            kernels[name] = dict(summary(t), bytes=8 * streams * n, tb_per_s=8 * streams * n / (statistics.median(t) * 1e-3) / 1e12)
        print(N + 1, {k: round(v["tb_per_s"], 2) for k, v in kernels.items()}, file=sys.stderr, flush=True)
        for a in xs:
            a.free()
        h.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
