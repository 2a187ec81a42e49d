"""mg_diffusion_apply_dkappa (diffusion_mf<SpMV, tangent>, mg_diffusion_mf.hip.h) on 257^3 and 1025^3 nodes, N_l = 8 * 2^l:
  kernels  "apply_dkappa" beside "diffusion_mf:spmv" on the same matrix-free level in the same session, through mg_time_kernel,
           two repetitions of --reps launches each (their distance is the run-to-run spread): ms per launch and the fraction
           of 8 TB/s on the model both share, 8 (x) + 8 (kappa / dkappa) + 8 (out) = 24 B per row
  hvp      one Hessian-vector product through torch_diffusion.DiffusionSolver at 257^3 (six levels, every level above 0
           matrix-free, log-normal kappa (sigma 1, seed 0), J = 1/2 ||u - d||^2, rtol 1e-6 as in tools/time_dkappa.py) beside one
           forward + backward: seconds, mg_pcg calls and iterations; both with the default tuning (captured V-cycles)

    python tools/time_tangent.py [--levels 5,7] [--json profiles/diffusion_tangent_time.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("diffusion_mf:spmv", "apply_dkappa")


def kernel_times(hi, reps):
    import torch
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 8 << hi
    rep = {"cells": N ** 3, "nodes": (N + 1) ** 3, "reps": reps, "model_bytes": 24 * (N + 1) ** 3}
    with DeviceHierarchy(3, hi - 1, hi) as h:
        gen = torch.Generator(device="cuda").manual_seed(4)
        kappa = torch.exp(torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
        torch.cuda.synchronize()
        h.gen_diffusion_hierarchy(kappa.data_ptr(), matrix_free_min_rows=0)     # kappa never leaves the device
        assert h.level_matrix_free(hi)
        del kappa
        for which in ("v", "f"):        # x, and a sign-indefinite direction in the first N^3 entries of F
            x = torch.randn(h.n_dofs(hi), dtype=torch.float64, device="cuda", generator=gen)
            torch.cuda.synchronize()
            h.set_vector_device(hi, which, x.data_ptr())
            del x
        for k in KERNELS:
            ms = [h.time_kernel(k, hi, reps) for _ in range(2)]
            rep[k] = {"ms": ms, "fraction_of_8TBs": rep["model_bytes"] / (min(ms) * 1e-3) / 8e12}
            print(N + 1, k, rep[k], flush=True)
    rep["tangent_over_spmv"] = min(rep["apply_dkappa"]["ms"]) / min(rep["diffusion_mf:spmv"]["ms"])
    return rep


def hvp_times(hi, n_levels):
    import numpy as np
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver, NotConverged
    N = 8 << hi
    kappa = np.exp(np.random.default_rng(0).standard_normal(N ** 3))
    gen = torch.Generator(device="cuda").manual_seed(5)
    f = torch.randn((N + 1) ** 3, dtype=torch.float64, device="cuda", generator=gen)
    d = torch.randn((N + 1) ** 3, dtype=torch.float64, device="cuda", generator=gen)
    v = torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen)
    out = {"N": N, "levels": n_levels, "rtol": 1e-6, "matrix_free_min_rows": 0}
    with DiffusionSolver(N, n_levels, rtol=out["rtol"], matrix_free_min_rows=0) as solver:
        out["graph"] = 1                            # captured V-cycles, the default
        for attempt in ("warm_up", "timed"):        # (the second pass: set-up work vectors and captured cycles exist)
            # kappa on the device: after the first pass the hierarchy is refreshed in place, and the times are the solves'
            k = torch.tensor(kappa, device="cuda", requires_grad=True)
            torch.cuda.synchronize()
            n0, t0 = solver.n_solves, time.perf_counter()
            J = 0.5 * torch.sum((solver.solve(k, f) - d) ** 2)
            J.backward()
            torch.cuda.synchronize()
            n1, t1 = solver.n_solves, time.perf_counter()
            first = {"seconds": t1 - t0, "solves": n1 - n0, "iterations": dict(solver.last_iterations), "J": float(J.detach()),
                     "grad_kappa_l2": float(k.grad.norm())}
            k = torch.tensor(kappa, device="cuda", requires_grad=True)
            torch.cuda.synchronize()
            n0, t0 = solver.n_solves, time.perf_counter()
            J = 0.5 * torch.sum((solver.solve(k, f) - d) ** 2)
            (g,) = torch.autograd.grad(J, k, create_graph=True)
            try:
                (hv,) = torch.autograd.grad(torch.sum(g * v), k)
            except NotConverged as exc:         # reported, not hidden: there is no figure then
                second = {"not_converged": str(exc), "solves": solver.n_solves - n0, "iterations": dict(solver.last_iterations),
                          "residuals": dict(solver.last_residual)}
                break
            torch.cuda.synchronize()
            n1, t1 = solver.n_solves, time.perf_counter()
            second = {"seconds": t1 - t0, "solves": n1 - n0, "iterations": dict(solver.last_iterations), "hv_l2": float(hv.norm())}
            del g, hv
        out["forward_backward"], out["hessian_vector"] = first, second
        if "seconds" in second:
            out["hvp_over_forward_backward"] = second["seconds"] / first["seconds"]
        out["levels_matrix_free"] = [bool(solver.hierarchy.level_matrix_free(l)) for l in range(n_levels)]
        print(out, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="5,7")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-hvp", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    report = {"kernels": {}}
    for hi in (int(x) for x in args.levels.split(",")):
        report["kernels"][str((8 << hi) + 1)] = kernel_times(hi, args.reps)
    if not args.no_hvp:
        report["hvp_257"] = hvp_times(5, 6)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
