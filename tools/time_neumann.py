"""No-flux faces (mg_set_diffusion_faces) beside the default set on 257^3 nodes, in one session, as interleaved repetitions:
  jacobi    one-step Jacobi launches of the matrix-free finest level through mg_time_kernel (events around --launches
            launches): diffusion_mf with the default set, diffusion_mf_faces with the set x- | x+
  gradient  a full DiffusionSolver gradient, forward solve plus backward (two mg_pcg, one sensitivity kernel, the lift and
            its derivative), kappa on the device, wall clock with a device synchronisation, for both sets
Every figure is the median over --reps repetitions, default and face set taking turns, with the spread (max - min) and the
ratio of the medians.  --default-only measures the default set alone and --lib loads another build of the library (one
without the entry: the parent commit's), so that the default-set times of two builds can be laid side by side; the cost of
the variant relative to the default kernel is reported, not gated.

    python tools/time_neumann.py [--json profiles/diffusion_neumann_time.json] [--default-only] [--lib other/libmg_hip.so]
(--json: where the report is written; without --default-only the default is profiles/diffusion_neumann_time.json)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FACES = ("x-", "x+")


def summary(ms):
    return {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=256)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.json is None and not args.default_only:     # (a --default-only run is a side measurement: written only where asked)
        args.json = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "diffusion_neumann_time.json")
    import torch  # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    from multigrid_dolfinx_amd import _capi
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    if args.default_only:       # (a build without the entry loads too)
        for name in ("mg_set_diffusion_faces", "mg_diffusion_faces"):
            _capi.SIGNATURES.pop(name, None)
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, top = args.elements, args.levels - 1
    sets = {"default": None} if args.default_only else {"default": None, "x-|x+": FACES}
    report = {"nodes": (N + 1) ** 3, "levels": args.levels, "reps": args.reps, "launches": args.launches,
              "library": args.lib or "in-tree", "jacobi": {}, "gradient": {}}
    gen = torch.Generator(device="cuda").manual_seed(4)
    kappa = torch.exp(torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
    n = (N + 1) ** 3
    f, d, g = (torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(3))
    torch.cuda.synchronize()

    # ---- the one-step Jacobi launch ----
    handles = {}
    for name, faces in sets.items():
        h = DeviceHierarchy(3, 0, top, c=N >> top)
        if faces is not None:
            h.set_diffusion_faces(faces)
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        h.gen_diffusion_hierarchy(kappa.data_ptr(), matrix_free_min_rows=0)
        h.set_vector_device(top, "v", f.data_ptr())
        h.time_kernel("diffusion_mf", top, args.launches)      # warm-up
        handles[name] = h
    ms = {name: [] for name in sets}
    for _ in range(args.reps):
        for name, h in handles.items():
            ms[name].append(h.time_kernel("diffusion_mf", top, args.launches))
    for h in handles.values():
        h.close()
    report["jacobi"] = {name: summary(v) for name, v in ms.items()}

    # ---- the gradient ----
    solvers = {}
    for name, faces in sets.items():
        extra = {} if faces is None else {"dirichlet_faces": faces}
        solvers[name] = DiffusionSolver(N, args.levels, matrix_free_min_rows=0, **extra)

    def gradient(solver):
        k, ft, gt = kappa.clone().requires_grad_(), f.clone().requires_grad_(), g.clone().requires_grad_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        J = 0.5 * torch.sum((solver.solve(k, ft, gt) - d) ** 2)
        J.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for solver in solvers.values():
        gradient(solver)        # warm-up: the first generation, the first captures
    ms = {name: [] for name in sets}
    for _ in range(args.reps):
        for name, solver in solvers.items():
            ms[name].append(gradient(solver))
    report["gradient"] = {name: summary(v) for name, v in ms.items()}
    report["gradient_iterations"] = {name: dict(s.last_iterations) for name, s in solvers.items()}
    for solver in solvers.values():
        solver.close()
    if not args.default_only:
        for what in ("jacobi", "gradient"):
            report[what]["ratio_of_medians"] = report[what]["x-|x+"]["median_ms"] / report[what]["default"]["median_ms"]
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
