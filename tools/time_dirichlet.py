"""The sensitivity operators with a node set per side (mg_diffusion_apply_dkappa_ex, mg_diffusion_dkappa_ex) beside the two
entries without node sets on 513^3 nodes, N_l = 8 * 2^l, in one session:
  entries  each of the four (rows, cols) pairs of T and the four (a_nodes, b_nodes) pairs of D through its entry by device
           pointer, beside mg_diffusion_apply_dkappa and mg_diffusion_dkappa: wall-clock ms per call over --reps calls after a
           warm-up call, twice (their distance is the run-to-run spread).  A call synchronises the handle's stream, so a figure is
           the kernel plus one launch and one synchronisation.
  kernels  "apply_dkappa", "apply_dkappa:all", "dkappa", "dkappa:all" through mg_time_kernel (events around --reps launches).

    python tools/time_dirichlet.py [--level 6] [--json profiles/diffusion_dirichlet_time.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = ("interior", "all")
KERNELS = ("apply_dkappa", "apply_dkappa:all", "dkappa", "dkappa:all")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch  # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    hi, reps = args.level, args.reps
    N = 8 << hi
    report = {"cells": N ** 3, "nodes": (N + 1) ** 3, "reps": reps, "entries_ms": {}, "kernels_ms": {}}
    with DeviceHierarchy(3, hi - 1, hi) as h:
        gen = torch.Generator(device="cuda").manual_seed(4)
        kappa = torch.exp(torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
        torch.cuda.synchronize()
        h.gen_diffusion_hierarchy(kappa.data_ptr(), matrix_free_min_rows=0)
        del kappa
        n = h.n_dofs(hi)
        w = torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen)
        x, a = (torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(2))
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def timed(call):
            call()
            ms = []
            for _ in range(2):
                t0 = time.perf_counter()
                for _ in range(reps):
                    call()
                ms.append((time.perf_counter() - t0) * 1e3 / reps)
            return ms

        import ctypes as C
        from multigrid_dolfinx_amd._capi import check
        ptr = lambda t: C.c_void_p(t.data_ptr())
        T = lambda: h.diffusion_apply_dkappa(hi, w.data_ptr(), x.data_ptr(), out.data_ptr())
        D = lambda: h.diffusion_dkappa(hi, a.data_ptr(), x.data_ptr(), out.data_ptr())
        T_ex = lambda rows, cols: check(h._lib.mg_diffusion_apply_dkappa_ex(h._h, h._idx(hi), ptr(w), ptr(x), rows, cols, ptr(out)))
        D_ex = lambda an, bn: check(h._lib.mg_diffusion_dkappa_ex(h._h, h._idx(hi), ptr(a), an, ptr(x), bn, ptr(out)))
        report["entries_ms"]["mg_diffusion_apply_dkappa"] = timed(T)
        for rows in (0, 1):
            for cols in (0, 1):
                report["entries_ms"][f"T_ex {SETS[rows]} {SETS[cols]}"] = timed(lambda: T_ex(rows, cols))
        report["entries_ms"]["mg_diffusion_dkappa"] = timed(D)
        for an in (0, 1):
            for bn in (0, 1):
                report["entries_ms"][f"D_ex {SETS[an]} {SETS[bn]}"] = timed(lambda: D_ex(an, bn))
        for name, ms in report["entries_ms"].items():
            print(N + 1, name, ms, flush=True)
        h.set_vector_device(hi, "v", x.data_ptr())
        h.set_vector_device(hi, "f", a.data_ptr())
        for k in KERNELS:
            report["kernels_ms"][k] = [h.time_kernel(k, hi, reps) for _ in range(2)]
            print(N + 1, k, report["kernels_ms"][k], flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
