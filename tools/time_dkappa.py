"""mg_diffusion_dkappa (mg_diffusion_adj.hip.h) on 257^3 and 1025^3 nodes, N_l = 8 * 2^l:
  kernels  "dkappa" (the plane march) and "dkappa_gather" (one thread per cell) through mg_time_kernel, two repetitions of
           --reps launches each (their distance is the run-to-run spread): ms per launch and the fraction of 8 TB/s on the model
           of 8 + 8 B per node read and 8 B per cell written (24 B per cell)
  solve    one forward + backward through torch_diffusion.DiffusionSolver at 257^3, log-normal kappa (sigma 1, seed 0),
           J = 1/2 ||u - d||^2: seconds and mg_pcg iterations of each solve, stored and matrix-free

    python tools/time_dkappa.py [--levels 5,7] [--json profiles/diffusion_dkappa_time.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("dkappa", "dkappa_gather")


def kernel_times(hi, reps):
    import torch
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 8 << hi
    rep = {"cells": N ** 3, "nodes": (N + 1) ** 3, "reps": reps, "model_bytes": 24 * N ** 3}
    with DeviceHierarchy(3, 2, hi) as h:
        h.gen_poisson_level(hi)         # (the kernel reads the grid's dimensions only: any 3-D level will do)
        gen = torch.Generator(device="cuda").manual_seed(4)
        for which in ("v", "f"):
            x = torch.randn(h.n_dofs(hi), dtype=torch.float64, device="cuda", generator=gen)
            torch.cuda.synchronize()
            h.set_vector_device(hi, which, x.data_ptr())
            del x
        for k in KERNELS:
            ms = [h.time_kernel(k, hi, reps) for _ in range(2)]
            rep[k] = {"ms": ms, "fraction_of_8TBs": rep["model_bytes"] / (min(ms) * 1e-3) / 8e12}
            print(N + 1, k, rep[k], flush=True)
    rep["march_over_gather"] = min(rep["dkappa_gather"]["ms"]) / min(rep["dkappa"]["ms"])
    return rep


def solve_times(hi, n_levels):
    import numpy as np
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 8 << hi
    kappa = np.exp(np.random.default_rng(0).standard_normal(N ** 3))
    gen = torch.Generator(device="cuda").manual_seed(5)
    f = torch.randn((N + 1) ** 3, dtype=torch.float64, device="cuda", generator=gen)
    d = torch.randn((N + 1) ** 3, dtype=torch.float64, device="cuda", generator=gen)
    # rtol 1e-6: the adjoint right-hand side u - d is dominated by smooth modes (||lambda|| / ||u - d|| = 1.4e5 here), and the
    # residual cannot fall below about eps ||A|| ||lambda|| = 0.8 in fp64, 7e-7 of ||u - d||; at 1e-10 the adjoint solve stalls there
    out = {"N": N, "levels": n_levels, "rtol": 1e-6}
    for label, min_rows in (("stored", None), ("matrix_free", 1 << 22)):
        with DiffusionSolver(N, n_levels, rtol=out["rtol"], matrix_free_min_rows=min_rows) as solver:
            r = {}
            for attempt in ("warm_up", "timed"):
                k = torch.tensor(kappa, requires_grad=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                J = 0.5 * torch.sum((solver.solve(k, f) - d) ** 2)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                J.backward()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                r = {"forward_s": t1 - t0, "backward_s": t2 - t1, "iterations": dict(solver.last_iterations), "J": float(J),
                     "grad_kappa_l2": float(k.grad.norm())}
            out[label] = r          # (the second pass: set-up work vectors and captured cycles exist)
            print(label, r, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="5,7")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-solve", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    report = {"kernels": {}}
    for hi in (int(x) for x in args.levels.split(",")):
        report["kernels"][str((8 << hi) + 1)] = kernel_times(hi, args.reps)
    if not args.no_solve:
        report["solve_257"] = solve_times(5, 6)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
