"""Solve to a tolerance three ways on the device-generated hierarchies of BASELINE configs 1-4: flexible CG preconditioned
by one V-cycle (`mg_pcg`), a loop of `mg_vcycle` with the residual after every cycle, and FMG (`mg_fmg`, mu0 = 2, then
cycles on the finest level until the tolerance).  Reports seconds and V-cycles (finest-level cycles) to ||r||_2 <= rtol ||f||_2,
the time of one V-cycle alone, and the time of one PCG iteration minus that (SpMV, three step kernels, folds, one 8-byte
read).

    python tools/time_pcg.py [--configs c1,c2,c3,c4] [--mus 50,2] [--rtol 1e-10] [--max 400] [--json out.json]
    python tools/time_pcg.py --configs c4 --mus 2 --profile-iters 4     # a few PCG iterations only (rocprofv3)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy          # noqa: E402

CONFIGS = {"c1": (2, 1, 3), "c2": (2, 4, 8), "c3": (3, 2, 5), "c4": (3, 2, 7)}      # (dim, lo, hi), N_l = 8 * 2^l


def timed(h, fn):
    h.sync()
    t0 = time.perf_counter()
    out = fn()
    h.sync()
    return time.perf_counter() - t0, out


def run(cfg, mu, rtol, max_it, cycle_reps):
    dim, lo, hi = CONFIGS[cfg]
    row = {"config": cfg, "mu": mu, "rtol": rtol}
    with DeviceHierarchy.synthetic(dim, lo, hi, c=8, mu1=mu, mu2=mu) as h:
        bn = h.norm2(hi, "f")
        h.zero_vector(hi, "v")
        h.vcycle(hi, 2)                       # warm-up: graphs of both ping-pong states, the direct coarsest solve
        h.zero_vector(hi, "v")
        h.pcg(rtol=0.0, max_iter=2)           # ... and the PCG work vectors
        h.zero_vector(hi, "v")
        dt, _ = timed(h, lambda: h.vcycle(hi, cycle_reps))
        row["ms_per_vcycle"] = 1e3 * dt / cycle_reps

        h.zero_vector(hi, "v")
        dt, hist = timed(h, lambda: h.pcg(rtol=rtol, max_iter=max_it))
        row["pcg"] = {"s": dt, "cycles": len(hist), "reached": bool(len(hist) and hist[-1] <= rtol * bn),
                      "true_rel": h.norm2(hi, "r") / bn}
        row["ms_per_pcg_iter_minus_vcycle"] = 1e3 * dt / max(1, len(hist)) - row["ms_per_vcycle"]

        def plain():
            for k in range(max_it):
                if h.vcycle(hi, 1, residuals=True)[0] <= rtol * bn:
                    return k + 1, True
            return max_it, False
        h.zero_vector(hi, "v")
        dt, (n, ok) = timed(h, plain)
        row["vcycle_loop"] = {"s": dt, "cycles": n, "reached": ok}

        dt, fh = timed(h, lambda: h.fmg(2, tol=rtol * bn, max_cycles=max_it, top_level=hi))
        row["fmg"] = {"s": dt, "cycles": len(fh), "reached": bool(len(fh) and fh[-1] <= rtol * bn)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c2,c3,c4")
    ap.add_argument("--mus", default="50,2")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--max", type=int, default=400)
    ap.add_argument("--cycle-reps", type=int, default=5)
    ap.add_argument("--profile-iters", type=int, default=0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.profile_iters:
        for cfg in args.configs.split(","):
            dim, lo, hi = CONFIGS[cfg]
            for mu in (int(m) for m in args.mus.split(",")):
                with DeviceHierarchy.synthetic(dim, lo, hi, c=8, mu1=mu, mu2=mu) as h:
                    h.zero_vector(hi, "v")
                    dt, hist = timed(h, lambda: h.pcg(rtol=0.0, max_iter=args.profile_iters))
                    print(f"{cfg} V({mu},{mu}): {len(hist)} PCG iterations in {dt:.3f} s, {h.memory_bytes() / 2**30:.1f} GiB on the device",
                          flush=True)
        return
    rows = []
    for cfg in args.configs.split(","):
        for mu in (int(m) for m in args.mus.split(",")):
            r = run(cfg, mu, args.rtol, args.max, args.cycle_reps)
            rows.append(r)
            fmt = lambda d: f"{d['s']:8.3f} s {d['cycles']:4d}{'' if d['reached'] else '+'}"     # noqa: E731
            print(f"{cfg} V({mu},{mu}) to {args.rtol:g}: pcg {fmt(r['pcg'])} | vcycle loop {fmt(r['vcycle_loop'])} | "
                  f"fmg {fmt(r['fmg'])} | {r['ms_per_vcycle']:.3f} ms per V-cycle, PCG iteration +"
                  f"{r['ms_per_pcg_iter_minus_vcycle']:.3f} ms (true residual {r['pcg']['true_rel']:.2e})", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
