"""Variable-coefficient diffusion levels (mg_gen_diffusion_level / mg_gen_diffusion_hierarchy) on BASELINE configs C3
(257^3) and C4 (1025^3), N_l = 8 * 2^l:
  setup    wall clock of the whole entry on the finest level next to mg_gen_poisson_level's, and the host -> device copy of
           the kappa bytes on its own (torch), all after a warm-up call
  levels   per field (planar 1:1000 jump at x = 1/2, log-normal sigma = 1 seeded): distinct rows, row classes and escape
           rows per level
  cycles   V(50,50) cycles/s of the jump hierarchy against the Poisson hierarchy in the same run, with the per-path
           smoother launch counts of one cycle
  solve    mg_pcg to ||r|| <= 1e-10 ||f|| from zero, V(2,2), P1 + P^T, Jacobi against Chebyshev, arithmetic / harmonic /
           Galerkin coarse levels: iterations and seconds
  --matrix-free   instead of the above: the log-normal finest level stored and matrix-free (mg_gen_diffusion_level_mf) side
           by side -- ms per Jacobi sweep, residual, SpMV and Chebyshev step of the stored one-step kernel (two repetitions:
           their distance is the run-to-run spread) and of diffusion_mf, the byte model and its fraction of 8 TB/s, device
           memory of both levels and both hierarchies, mg_pcg to 1e-10 with V(2,2) Jacobi and Chebyshev on both
The gen_diffusion kernel itself is timed from a kernel trace:
    rocprofv3 --kernel-trace --stats -d profiles/diffusion_trace -o run -- python tools/time_diffusion.py --gen-only

    python tools/time_diffusion.py [--configs c3,c4] [--json profiles/diffusion_time.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"c3": (3, 2, 5), "c4": (3, 2, 7)}


def fields(N, dim):
    from tests.diffusion_workers import jump_kappa, lognormal_kappa
    return {"jump": jump_kappa(N, dim), "lognormal": lognormal_kappa(N, dim, seed=0)}


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def setup_times(dim, lo, hi, kappa):
    import torch
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    out = {}
    with DeviceHierarchy(dim, lo, hi) as h:
        h.gen_diffusion_level(hi, kappa)
        h.sync()
        out["gen_diffusion_level_s"] = timed(lambda: (h.gen_diffusion_level(hi, kappa), h.sync()))
        h.gen_poisson_level(hi)
        out["gen_poisson_level_s"] = timed(lambda: (h.gen_poisson_level(hi), h.sync()))
    t = torch.from_numpy(kappa)
    t.to("cuda")
    torch.cuda.synchronize()
    out["kappa_upload_s"] = timed(lambda: (t.to("cuda"), torch.cuda.synchronize()))
    out["kappa_bytes"] = int(kappa.nbytes)
    return out


def level_report(h, lo, hi):
    rows = {}
    for l in range(lo, hi + 1):
        s, i = h.level_storage(l), h.level_info(l)
        rows[l] = {"distinct_rows": s["distinct_rows"], "row_classes": i["row_classes"], "escape_rows": s["escape_rows"]}
    return rows


def cycles_per_s(h, hi, n=5):
    import numpy as np
    h.zero_vector(hi, "v")
    h.set_vector(hi, "f", np.ones(h.n_dofs(hi)))
    h.vcycle(hi, 1)
    h.sync()
    return n / timed(lambda: (h.vcycle(hi, n), h.sync()))


def launches(h, lo, hi):
    """Per-path smoother launches of one V-cycle on a fresh hierarchy (before any cycle is captured and replayed)."""
    import numpy as np
    h.zero_vector(hi, "v")
    h.set_vector(hi, "f", np.ones(h.n_dofs(hi)))
    h.prepare_cycle(hi)
    h.reset_smoother_launches()
    h.vcycle(hi, 1)
    return {l: h.smoother_launches(l) for l in range(lo + 1, hi + 1)}


# bytes per row and launch: (stored symmetric diagonals, matrix-free)
MF_BYTES = {"jacobi": (56, 32), "residual": (56, 32), "spmv": (48, 24), "chebyshev": (64, 40)}


def matrix_free_report(dim, lo, hi, kappa, reps, min_rows, solve=True):
    import numpy as np
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    rows = ((8 << hi) + 1) ** dim
    rng = np.random.default_rng(4)
    v, f = rng.standard_normal(rows), rng.standard_normal(rows)
    rep = {"rows": rows, "reps": reps, "kernels": {}}

    def level_times(h, names):
        h.set_chebyshev_bounds(hi, 0.3, 2.2)
        h.set_vector(hi, "v", v)
        h.set_vector(hi, "f", f)
        return {k: h.time_kernel(name, hi, reps) for k, name in names.items()}

    with DeviceHierarchy(dim, lo, hi) as s:
        s.gen_diffusion_level(hi, kappa)
        rep["stored_level_bytes"] = s.memory_bytes()
        names = {k: k for k in MF_BYTES}
        stored = [level_times(s, names), level_times(s, names)]
    with DeviceHierarchy(dim, lo, hi) as m:
        m.gen_diffusion_level(hi, kappa, matrix_free=True)
        rep["matrix_free_level_bytes"] = m.memory_bytes()
        free = [level_times(m, {k: "diffusion_mf:" + k for k in MF_BYTES}) for _ in range(2)]
    for k, (bs, bm) in MF_BYTES.items():
        s_ms, m_ms = min(x[k] for x in stored), min(x[k] for x in free)
        rep["kernels"][k] = {
            "stored_ms": [x[k] for x in stored], "matrix_free_ms": [x[k] for x in free],
            "speedup": s_ms / m_ms, "model_speedup": bs / bm,
            "stored_fraction_of_8TBs": bs * rows / (s_ms * 1e-3) / 8e12,
            "matrix_free_fraction_of_8TBs": bm * rows / (m_ms * 1e-3) / 8e12}
        print(k, rep["kernels"][k], flush=True)
    if not solve:
        return rep
    for sm in ("jacobi", "chebyshev"):
        for label, mr in (("stored", None), ("matrix_free", min_rows)):
            with DeviceHierarchy.synthetic_diffusion(dim, lo, hi, kappa, smoother=sm, matrix_free_min_rows=mr) as h:
                h.zero_vector(hi, "v")
                h.set_vector(hi, "f", f)
                h.prepare_cycle(hi)
                h.sync()
                t = time.perf_counter()
                hist = h.pcg(rtol=1e-10, max_iter=200)
                h.sync()
                rep[f"pcg_{sm}_{label}"] = {"iterations": len(hist), "seconds": time.perf_counter() - t,
                                            "final_rel": float(hist[-1] / np.linalg.norm(f)),
                                            "hierarchy_bytes": h.memory_bytes(),
                                            "matrix_free_levels": [l for l in range(lo, hi + 1) if h.level_matrix_free(l)]}
            print(f"pcg_{sm}_{label}", rep[f"pcg_{sm}_{label}"], flush=True)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--json", default=None)
    ap.add_argument("--gen-only", action="store_true")
    ap.add_argument("--matrix-free", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mf-min-rows", type=int, default=1 << 22)
    ap.add_argument("--no-solve", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    report = {}
    for name in args.configs.split(","):
        dim, lo, hi = CONFIGS[name]
        N = 8 << hi
        if args.matrix_free:
            # (the log-normal field of fields(): sigma 1, seed 0)
            kappa = np.exp(np.random.default_rng(0).standard_normal(N ** dim))
            report[name] = matrix_free_report(dim, lo, hi, kappa, args.reps, args.mf_min_rows, solve=not args.no_solve)
            continue
        fs = fields(N, dim)
        if args.gen_only:
            with DeviceHierarchy(dim, lo, hi) as h:
                for k in fs.values():
                    h.gen_diffusion_level(hi, k)
                h.gen_poisson_level(hi)
            continue
        rep = {"setup": setup_times(dim, lo, hi, fs["jump"])}
        print(name, "setup", rep["setup"], flush=True)
        with DeviceHierarchy.synthetic(dim, lo, hi, mu1=50, mu2=50) as p:
            p.set_params(50, 50, 2.0 / 3.0, restriction="p1_transpose")
            p.set_prolongation("p1")
            rep["poisson_levels"] = level_report(p, lo, hi)
            rep["poisson_launches"] = launches(p, lo, hi)
            rep["poisson_v50_cycles_per_s"] = cycles_per_s(p, hi)
        for fname, kappa in fs.items():
            fr = {}
            with DeviceHierarchy.synthetic_diffusion(dim, lo, hi, kappa, mu1=50, mu2=50) as h:
                fr["levels"] = level_report(h, lo, hi)
                fr["launches"] = launches(h, lo, hi)
                fr["v50_cycles_per_s"] = cycles_per_s(h, hi)
            f = np.random.default_rng(4).standard_normal((N + 1) ** dim)
            for coarse in ("arithmetic", "harmonic", "galerkin"):
                for sm in ("jacobi", "chebyshev"):
                    key = f"pcg_{coarse}_{sm}"
                    try:
                        with DeviceHierarchy.synthetic_diffusion(dim, lo, hi, kappa, coarse=coarse, smoother=sm) as h:
                            h.zero_vector(hi, "v")
                            h.set_vector(hi, "f", f)
                            h.prepare_cycle(hi)
                            h.sync()
                            t = time.perf_counter()
                            hist = h.pcg(rtol=1e-10, max_iter=200)
                            h.sync()
                            fr[key] = {"iterations": len(hist), "seconds": time.perf_counter() - t,
                                       "final_rel": float(hist[-1] / np.linalg.norm(f))}
                    except Exception as exc:          # recorded as measured: e.g. an estimate refused on a level
                        fr[key] = {"error": str(exc)}
                    print(name, fname, key, fr[key], flush=True)
            rep[fname] = fr
            print(name, fname, json.dumps({k: v for k, v in fr.items() if not k.startswith("pcg")}), flush=True)
        report[name] = rep
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1, default=str)
    print(json.dumps(report, default=str))


if __name__ == "__main__":
    main()
