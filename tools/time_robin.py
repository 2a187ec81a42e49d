"""Robin faces (mg_set_diffusion_robin) on 257^3 nodes, in one session, as interleaved repetitions:
  jacobi    one-step Jacobi launches of the matrix-free finest level through mg_time_kernel (events around --launches
            launches), Dirichlet data on z- only:
              faces        no field                                    diffusion_mf_faces   32 B per row
              robin        fields on z+ and x-, no reaction term       diffusion_mf_react   40 B per row: the nodal vector holds B
              react        a reaction field, no Robin field            diffusion_mf_react   40 B per row
              react_robin  both: the nodal vector holds R + B          diffusion_mf_react   40 B per row
            (the record of the rejected march that formed B from the face fields, 32 B per row, measured by this tool when
            "robin" launched it: profiles/diffusion_robin_onthefly_time.json)
            default        all six faces Dirichlet, no field           diffusion_mf         (the no-regression figure)
  gradient  a full DiffusionSolver gradient, forward solve plus backward, every field on the device, wall clock with a device
            synchronisation: default, faces, robin, and the mg_pcg iteration counts
  kernels   the sensitivity kernels of face z+ on the finest level: drobin and apply_drobin
Every figure is the median over --reps repetitions, the variants taking turns, with the spread (max - min).  --default-only
measures the handles without a field alone (default, faces) and --lib loads another build of the library (one without the
entries: the parent commit's), so that the default times of two builds can be laid side by side.

    python tools/time_robin.py [--json profiles/diffusion_robin_time.json] [--default-only] [--lib other/libmg_hip.so]
(--json: where the report is written; without --default-only the default is profiles/diffusion_robin_time.json)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW_ENTRIES = ("mg_set_diffusion_robin", "mg_set_diffusion_robin_device", "mg_diffusion_robin", "mg_level_robin",
               "mg_diffusion_drobin", "mg_diffusion_apply_drobin")
DIRICHLET = 16                  # z-
FIELD_FACES = (32, 1)           # z+ (N^2 rows in two planes' worth of tiles), x- (one row per line of every plane)


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
        args.json = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "diffusion_robin_time.json")
    import torch  # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    from multigrid_dolfinx_amd import _capi
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    if args.default_only:       # (a build without the entries loads too)
        for name in NEW_ENTRIES:
            _capi.SIGNATURES.pop(name, None)
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, top = args.elements, args.levels - 1
    variants = ("default", "faces") if args.default_only else ("default", "faces", "robin", "react", "react_robin")
    report = {"nodes": (N + 1) ** 3, "levels": args.levels, "reps": args.reps, "launches": args.launches,
              "library": args.lib or "in-tree", "dirichlet_faces": DIRICHLET, "field_faces": list(FIELD_FACES), "jacobi": {}, "gradient": {}}
    gen = torch.Generator(device="cuda").manual_seed(4)
    kappa = torch.exp(torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
    sigma = float(N) ** 2 * 10.0 ** (-3.0 + 3.0 * torch.rand(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
    # alpha h between 1e-4 and 1e2: insulated patches beside nearly clamped ones
    alpha = {face: float(N) * 10.0 ** (-4.0 + 6.0 * torch.rand(N ** 2, dtype=torch.float64, device="cuda", generator=gen)) for face in FIELD_FACES}
    n = (N + 1) ** 3
    f, d, g = (torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(3))
    torch.cuda.synchronize()

    # ---- the one-step Jacobi launch, and the sensitivity kernels ----
    handles = {}
    for name in variants:
        h = DeviceHierarchy(3, 0, top, c=N >> top)
        if name != "default":
            h.set_diffusion_faces(DIRICHLET)
        if name in ("react", "react_robin"):
            h.set_diffusion_reaction(sigma.data_ptr(), N=N)
        if name in ("robin", "react_robin"):
            for face in FIELD_FACES:
                h.set_diffusion_robin(face, alpha[face].data_ptr(), N=N)
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        h.gen_diffusion_hierarchy(kappa.data_ptr(), matrix_free_min_rows=0)
        h.set_vector_device(top, "v", f.data_ptr())
        h.time_kernel("diffusion_mf", top, args.launches)      # warm-up
        handles[name] = h
    ms = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, h in handles.items():
            ms[name].append(h.time_kernel("diffusion_mf", top, args.launches))
    report["jacobi"] = {name: summary(v) for name, v in ms.items()}
    if not args.default_only:
        h = handles["robin"]
        keys = ("drobin", "apply_drobin")
        for key in keys:
            h.time_kernel(key, top, 5)
        ms = {key: [] for key in keys}
        for _ in range(args.reps):
            for key in keys:
                ms[key].append(h.time_kernel(key, top, args.launches))
        report["kernels"] = {key: summary(v) for key, v in ms.items()}
    for h in handles.values():
        h.close()

    # ---- the gradient ----
    grad_variants = ("default", "faces") if args.default_only else ("default", "faces", "robin")
    solvers = {name: DiffusionSolver(N, args.levels, matrix_free_min_rows=0, dirichlet_faces=None if name == "default" else DIRICHLET)
               for name in grad_variants}

    def gradient(name, solver):
        k, ft, gt = kappa.clone().requires_grad_(), f.clone().requires_grad_(), g.clone().requires_grad_()
        extra = {"robin": {face: a.clone().requires_grad_() for face, a in alpha.items()}} if name == "robin" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        J = 0.5 * torch.sum((solver.solve(k, ft, gt, **extra) - d) ** 2)
        J.backward()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, solver in solvers.items():
        gradient(name, solver)  # warm-up: the first generation, the first captures
    ms = {name: [] for name in grad_variants}
    for _ in range(args.reps):
        for name, solver in solvers.items():
            ms[name].append(gradient(name, solver))
    report["gradient"] = {name: summary(v) for name, v in ms.items()}
    report["gradient_iterations"] = {name: dict(s.last_iterations) for name, s in solvers.items()}
    for solver in solvers.values():
        solver.close()
    if not args.default_only:
        j = report["jacobi"]
        j["robin_over_faces"] = j["robin"]["median_ms"] / j["faces"]["median_ms"]
        j["react_over_faces"] = j["react"]["median_ms"] / j["faces"]["median_ms"]
        j["react_minus_robin_ms"] = j["react"]["median_ms"] - j["robin"]["median_ms"]
        report["gradient"]["robin_over_faces"] = report["gradient"]["robin"]["median_ms"] / report["gradient"]["faces"]["median_ms"]
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
