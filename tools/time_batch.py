"""Batched solves (mg_apply_batch, mg_pcg_batch, DiffusionSolver.solve_many) beside one solve per right-hand side, on 257^3 nodes
with six levels, every level above the coarsest matrix-free, in one session, as interleaved repetitions, for the default
hierarchy and for one with a reaction field and the face set 18:
  kernels   diffusion_mf_batch<NV>:jacobi|residual|spmv for NV = 2, 3, 4 beside the one-vector kernel, through mg_time_kernel
            (events around --launches launches), on the finest (257^3) and the next (129^3) level; per_vector = the fused time
            over NV one-vector launches
  bits      at the sizes timed: mg_apply_batch of four lanes on the finest level against the handle's own one-vector calls
  gradient  a gradient of a misfit summed over B = 4 and 8 sources, forward plus backward, wall clock with a device
            synchronisation: solve_many + backward ("many"), the same with "mf_batch" 0 ("many_unfused": one generation, the
            lanes in lockstep, no fused launch) and B calls of solve + backward ("loop": the only way without solve_many; the
            calls after the first with same_operator=True, so the loop generates once as well)
Every figure is the median over --reps repetitions, the variants taking turns, with the spread (max - min).  --loop-only
measures the loop alone and --lib loads another build of the library (one without the entries: the parent commit's), so that
the loop's times of two builds can be laid side by side; --parent-report takes the report of such a run (made in the same
session) into this one's, under "loop_on_parent_build".

    python tools/time_batch.py --loop-only --lib other/libmg_hip.so --json parent_loop.json
    python tools/time_batch.py [--json profiles/diffusion_batch_time.json] [--parent-report parent_loop.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW_ENTRIES = ("mg_apply_batch", "mg_pcg_batch", "mg_batch_info", "mg_release_batch")
OPS = ("jacobi", "residual", "spmv")


def summary(ms):
    return {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=256)
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sources", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--parent-report", default=None)
    args = ap.parse_args()
    if args.json is None and not args.loop_only:        # (a --loop-only run is a side measurement: written only where asked)
        args.json = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "diffusion_batch_time.json")
    import torch  # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    from multigrid_dolfinx_amd import _capi
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    if args.loop_only:          # (a build without the entries loads too)
        for name in NEW_ENTRIES:
            _capi.SIGNATURES.pop(name, None)
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, top = args.elements, args.levels - 1
    n = (N + 1) ** 3
    report = {"nodes": n, "levels": args.levels, "reps": args.reps, "launches": args.launches, "library": args.lib or "in-tree",
              "hierarchies": {}}
    gen = torch.Generator(device="cuda").manual_seed(4)
    kappa = torch.exp(torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
    sigma = float(N) ** 2 * 10.0 ** (-3.0 + 3.0 * torch.rand(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
    Bmax = max(args.sources)
    F = torch.zeros(Bmax, n, dtype=torch.float64, device="cuda")
    for b in range(Bmax):       # point sources inside the cube
        i, j, k = (torch.randint(N // 8, N - N // 8, (3,), generator=torch.Generator().manual_seed(b))).tolist()
        F[b, (k * (N + 1) + j) * (N + 1) + i] = 1.0
    D = 1e-3 * torch.randn(Bmax, n, dtype=torch.float64, device="cuda", generator=gen)
    torch.cuda.synchronize()

    for name, faces, react in (("default", 63, False), ("sigma_faces18", 18, True)):
        out = report["hierarchies"][name] = {"dirichlet_faces": faces, "reaction": react}
        if not args.loop_only:
            h = DeviceHierarchy(3, 0, top, c=N >> top)
            h.set_diffusion_faces(faces)
            if react:
                h.set_diffusion_reaction(sigma.data_ptr(), N=N)
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
            h.set_prolongation("p1")
            h.gen_diffusion_hierarchy(kappa.data_ptr(), matrix_free_min_rows=0)
            # ---- the bits, at the size timed ----
            x = torch.randn(4, n, dtype=torch.float64, device="cuda", generator=gen)
            f = torch.randn(4, n, dtype=torch.float64, device="cuda", generator=gen)
            got, want = torch.empty_like(x), torch.empty_like(x)
            torch.cuda.synchronize()
            ptrs = lambda t: [t[b].data_ptr() for b in range(t.shape[0])]
            same = {}
            for op in OPS:
                dots = h.apply_batch(op, ptrs(x), ptrs(f), ptrs(got), level=top, dots=op == "spmv")
                single_dots = []
                for b in range(4):
                    h.set_vector_device(top, "v", x[b].data_ptr())
                    h.set_vector_device(top, "f", f[b].data_ptr())
                    if op == "jacobi":
                        h.smooth(top, 1)
                    elif op == "residual":
                        h.residual(top)
                    else:
                        single_dots.append(h.quadratic_form(top, "v"))
                    h.get_vector_device(top, "v" if op == "jacobi" else "r", want[b].data_ptr())
                same[op] = bool(torch.equal(got, want)) and (op != "spmv" or list(dots) == single_dots)
            out["bits_equal_at_%d" % (N + 1)] = same
            h.release_batch()
            del x, f, got, want
            # ---- the kernels ----
            kernels = out["kernels"] = {}
            for level in (top, top - 1):
                rng = torch.randn(h.n_dofs(level), dtype=torch.float64, device="cuda", generator=gen)
                torch.cuda.synchronize()
                h.set_vector_device(level, "v", rng.data_ptr())
                h.set_vector_device(level, "f", rng.data_ptr())
                keys = ["diffusion_mf:" + op for op in OPS] + ["diffusion_mf_batch%d:%s" % (nv, op) for nv in (2, 3, 4) for op in OPS]
                for key in keys:
                    h.time_kernel(key, level, 3)        # warm-up
                ms = {key: [] for key in keys}
                for _ in range(args.reps):
                    for key in keys:
                        ms[key].append(h.time_kernel(key, level, args.launches))
                side = (N >> (top - level)) + 1
                lv = kernels["%d^3" % side] = {key: summary(v) for key, v in ms.items()}
                for nv in (2, 3, 4):
                    for op in OPS:
                        lv["diffusion_mf_batch%d:%s" % (nv, op)]["per_vector"] = (
                            lv["diffusion_mf_batch%d:%s" % (nv, op)]["median_ms"] / (nv * lv["diffusion_mf:" + op]["median_ms"]))
            h.close()

        # ---- the gradient over B sources ----
        kinds = ("loop",) if args.loop_only else ("many", "many_unfused", "loop")
        solvers = {kind: DiffusionSolver(N, args.levels, matrix_free_min_rows=0, dirichlet_faces=faces) for kind in kinds}
        if "many_unfused" in solvers:
            solvers["many_unfused"].hierarchy.set_tuning("mf_batch", 0)

        def gradient(kind, solver, B):
            k = kappa.clone().requires_grad_()
            extra = {"sigma": sigma.clone().requires_grad_()} if react else {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "loop":
                for b in range(B):
                    J = 0.5 * torch.sum((solver.solve(k, F[b], same_operator=b > 0, **extra) - D[b]) ** 2)
                    J.backward()
            else:
                J = 0.5 * torch.sum((solver.solve_many(k, F[:B], **extra) - D[:B]) ** 2)
                J.backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, k.grad

        grads = out["gradient"] = {}
        for B in args.sources:
            first = {kind: gradient(kind, solver, B)[1] for kind, solver in solvers.items()}     # warm-up: generations, lanes, captures
            ms = {kind: [] for kind in kinds}
            for rep in range(args.reps):
                for kind, solver in solvers.items():
                    ms[kind].append(gradient(kind, solver, B)[0])
                print(name, "B =", B, "repetition", rep, file=sys.stderr, flush=True)
            g = grads["B=%d" % B] = {kind: summary(v) for kind, v in ms.items()}
            print(name, "B =", B, {kind: round(g[kind]["median_ms"], 1) for kind in kinds}, file=sys.stderr, flush=True)
            g["iterations"] = {kind: (dict(s.last_lane_iterations) if kind != "loop" else dict(s.last_iterations)) for kind, s in solvers.items()}
            if not args.loop_only:
                g["many_over_loop"] = g["many"]["median_ms"] / g["loop"]["median_ms"]
                g["many_unfused_over_loop"] = g["many_unfused"]["median_ms"] / g["loop"]["median_ms"]
                scale = float(first["loop"].abs().max())
                g["grad_kappa_many_equals_unfused"] = bool(torch.equal(first["many"], first["many_unfused"]))
                g["grad_kappa_many_minus_loop_over_max"] = float((first["many"] - first["loop"]).abs().max()) / scale
            del first
        for solver in solvers.values():
            solver.close()
    if args.parent_report:
        with open(args.parent_report) as fh:
            parent = json.load(fh)
        report["loop_on_parent_build"] = {name: {B: g["loop"] for B, g in h["gradient"].items()} for name, h in parent["hierarchies"].items()}
        for name, by_b in report["loop_on_parent_build"].items():
            for B, loop in by_b.items():
                g = report["hierarchies"][name]["gradient"][B]
                if "many" in g:
                    g["many_over_parent_loop"] = g["many"]["median_ms"] / loop["median_ms"]
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
