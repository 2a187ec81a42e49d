"""The Chebyshev smoother (MG_SMOOTH_CHEBYSHEV) against weighted Jacobi, on the device-generated hierarchies of BASELINE
configs 1-4 with the P1 embedding and R = P^T:
  --study    the NumPy cycle study that fixed the default lower_ratio (tests/cheb_reference.py; no GPU): contraction per
             V(m, m) cycle from zero on 65^2 and 33^3 Poisson hierarchies, Jacobi 2/3 against Chebyshev for several ratios,
             and on the 1 : 1000 coefficient jump with Galerkin coarse levels
  kernels    per-step time of the one-step Chebyshev kernel ("chebyshev") next to the Jacobi one-sweep kernel ("jacobi")
             on every level of the config (mg_time_kernel), with the bytes per row of the class-coded formats
  estimate   wall clock of the Lanczos estimate per level (the first mg_chebyshev_bounds call on a fresh handle) and the
             device bytes it held
  solve      finest-level cycles and seconds to ||r||_2 <= rtol ||f||_2 from zero for a loop of mg_vcycle, mg_pcg and FMG
             (mu0 = 2, then cycles on the finest level), V(mu, mu) with either smoother

    python tools/time_chebyshev.py --study
    python tools/time_chebyshev.py [--configs c1,c2,c3,c4] [--mus 2] [--rtol 1e-10] [--max 400] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"c1": (2, 1, 3), "c2": (2, 4, 8), "c3": (3, 2, 5), "c4": (3, 2, 7)}      # (dim, lo, hi), N_l = 8 * 2^l


def study():
    import numpy as np
    from tests import cheb_reference as ref
    rng = np.random.default_rng(0)
    rows = []
    cases = [("poisson", 2, 4, 5), ("poisson", 3, 4, 4), ("jump_galerkin", 2, 4, 5), ("jump_galerkin", 3, 4, 4)]
    for kind, dim, N0, nlev in cases:
        if kind == "poisson":
            As = ref.poisson_matrices(dim, N0, nlev)
        else:
            As = ref.galerkin_matrices(ref.kuhn_diffusion(N0 << (nlev - 1), dim), dim, N0, nlev)
        f = rng.standard_normal(As[-1].shape[0])
        n = (N0 << (nlev - 1)) + 1
        for m in (2, 4):
            row = {"case": kind, "grid": f"{n}^{dim}", "degree": m,
                   "jacobi": ref.contraction(ref.Cycle(As, dim, N0, mu1=m, mu2=m, smoother="jacobi").history(f, 10))}
            for ratio in (3, 4, 6, 8, 11, 30):
                row[f"cheb_{ratio}"] = ref.contraction(ref.Cycle(As, dim, N0, mu1=m, mu2=m, lower_ratio=ratio).history(f, 10))
            rows.append(row)
            print(" ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
    return rows


def timed(h, fn):
    h.sync()
    t0 = time.perf_counter()
    out = fn()
    h.sync()
    return time.perf_counter() - t0, out


def make(cfg, smoother, mu):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    dim, lo, hi = CONFIGS[cfg]
    h = DeviceHierarchy.synthetic(dim, lo, hi, c=8, mu1=mu, mu2=mu)
    h.set_params(mu, mu, 2.0 / 3.0, restriction="p1_transpose", smoother=smoother)
    h.set_prolongation("p1")
    return h


def kernels_and_estimate(cfg, reps):
    dim, lo, hi = CONFIGS[cfg]
    out = []
    with make(cfg, "chebyshev", 2) as h:
        for l in range(lo + 1, hi + 1):
            dt, b = timed(h, lambda: h.chebyshev_bounds(l))
            row = {"config": cfg, "level": l, "rows": h.n_dofs(l), "estimate_s": dt, "estimate_bytes": h.chebyshev_estimate_bytes(),
                   "bounds": b, "row_classes": h.level_info(l)["row_classes"]}
            for k in ("jacobi", "chebyshev"):
                h.time_kernel(k, l, 3)
                row[k + "_ms"] = h.time_kernel(k, l, reps)
            n = h.n_dofs(l)
            # class-coded rows: x 8 + f 8 + out 8 + class byte 1; Chebyshev also reads x_{k-1} 8
            row["cheb_TB_s_at_33B"] = 33.0 * n / row["chebyshev_ms"] / 1e9
            row["jacobi_TB_s_at_25B"] = 25.0 * n / row["jacobi_ms"] / 1e9
            out.append(row)
            print(f"{cfg} level {l} ({n} rows): estimate {dt * 1e3:8.2f} ms, {row['estimate_bytes'] / 1e9:.2f} GB held; "
                  f"jacobi {row['jacobi_ms'] * 1e3:9.1f} us, chebyshev {row['chebyshev_ms'] * 1e3:9.1f} us "
                  f"({row['cheb_TB_s_at_33B']:.2f} TB/s at 33 B/row = {row['cheb_TB_s_at_33B'] / 8:.2f} of 8 TB/s)", flush=True)
    return out


def solve(cfg, smoother, mu, rtol, max_it):
    dim, lo, hi = CONFIGS[cfg]
    row = {"config": cfg, "smoother": smoother, "mu": mu, "rtol": rtol}
    with make(cfg, smoother, mu) as h:
        bn = h.norm2(hi, "f")
        h.zero_vector(hi, "v")
        h.vcycle(hi, 2)                       # warm-up: estimates, graphs, the direct coarsest solve, PCG work vectors
        h.zero_vector(hi, "v")
        h.pcg(rtol=0.0, max_iter=2)

        def plain():
            for k in range(max_it):
                if h.vcycle(hi, 1, residuals=True)[0] <= rtol * bn:
                    return k + 1, True
            return max_it, False
        h.zero_vector(hi, "v")
        dt, (n, ok) = timed(h, plain)
        row["vcycle_loop"] = {"s": dt, "cycles": n, "reached": ok}
        h.zero_vector(hi, "v")
        dt, hist = timed(h, lambda: h.pcg(rtol=rtol, max_iter=max_it))
        row["pcg"] = {"s": dt, "cycles": len(hist), "reached": bool(len(hist) and hist[-1] <= rtol * bn)}
        dt, fh = timed(h, lambda: h.fmg(2, tol=rtol * bn, max_cycles=max_it, top_level=hi))
        row["fmg"] = {"s": dt, "cycles": len(fh), "reached": bool(len(fh) and fh[-1] <= rtol * bn)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--study", action="store_true")
    ap.add_argument("--configs", default="c1,c2,c3,c4")
    ap.add_argument("--mus", default="2")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--max", type=int, default=400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    result = {}
    if args.study:
        result["study"] = study()
    configs = [c for c in args.configs.split(",") if c in CONFIGS] if not args.study else []
    result["kernels"] = [r for cfg in configs for r in kernels_and_estimate(cfg, args.reps)]
    result["solve"] = []
    for cfg in configs:
        for mu in [int(m) for m in args.mus.split(",")]:
            for smoother in ("jacobi", "chebyshev"):
                r = solve(cfg, smoother, mu, args.rtol, args.max)
                result["solve"].append(r)
                f = lambda d: f"{d['cycles']:4d}{'' if d['reached'] else '+'} {d['s']:7.3f} s"
                print(f"{cfg} V({mu},{mu}) {smoother:9s} vcycle {f(r['vcycle_loop'])} | pcg {f(r['pcg'])} | "
                      f"fmg {f(r['fmg'])}", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1, default=str)


if __name__ == "__main__":
    main()
