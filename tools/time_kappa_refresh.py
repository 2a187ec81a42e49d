"""kappa from device memory (mg_gen_diffusion_hierarchy_device, mg_refresh_diffusion_hierarchy, kappa_ingest of
mg_diffusion_kappa.hip.h) against the host hand-off, N_l = 8 * 2^l, levels 2 .. top, log-normal kappa (sigma 1):
  hierarchy  wall seconds of gen_diffusion_hierarchy from a host array (the entry that existed before the device entries:
             upload, check, every level freed, reallocated and rebuilt), of the same call from a device address, and of
             refresh_diffusion_hierarchy, each on a handle that holds a hierarchy already (what a loop over kappa pays), two
             repetitions after a first call that is reported by itself; every call returns with the stream synchronised
  kernel     "kappa_ingest" through mg_time_kernel on the matrix-free top level, two repetitions of --reps launches: ms per
             launch and the fraction of 8 TB/s on the model of 17 B per fine cell
  solve      forward solves through torch_diffusion.DiffusionSolver at 257^3 with kappa on the device, stored and matrix-free:
             (levels of at least 2^22 rows, and all levels above the coarsest): the first solve (generates), two refreshed solves, with the seconds spent putting kappa into the hierarchy and in
             mg_pcg, and one more mg_pcg on the hierarchy as it stands (no factorisation, no capture: the solve alone)

    python tools/time_kappa_refresh.py [--tops 5,7] [--json profiles/diffusion_refresh_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MF_MIN_ROWS = 1 << 22


def _wall(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def hierarchy_times(top, reps):
    import torch
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 8 << top
    gen = torch.Generator(device="cuda").manual_seed(0)
    kd = torch.exp(torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen))
    kh = kd.cpu().numpy()
    torch.cuda.synchronize()
    rep = {"cells": N ** 3, "rows": (N + 1) ** 3, "kappa_bytes": 8 * N ** 3, "matrix_free_min_rows": MF_MIN_ROWS}
    with DeviceHierarchy(3, 2, top) as h:
        calls = (("host", lambda: h.gen_diffusion_hierarchy(kh, matrix_free_min_rows=MF_MIN_ROWS)),
                 ("device", lambda: h.gen_diffusion_hierarchy(kd.data_ptr(), matrix_free_min_rows=MF_MIN_ROWS)),
                 ("refresh", lambda: h.refresh_diffusion_hierarchy(kd.data_ptr())))
        for name, call in calls:
            first = _wall(call)
            rep[name] = {"first_s": first, "s": [_wall(call) for _ in range(2)], "rhs_norm": h.norm2(top, "f"),
                         "hierarchy_bytes": h.memory_bytes()}
            print(N + 1, name, rep[name], flush=True)
        rep["matrix_free_levels"] = [l for l in range(2, top + 1) if h.level_matrix_free(l)]
        ms = [h.time_kernel("kappa_ingest", top, reps) for _ in range(2)]
        rep["kappa_ingest"] = {"reps": reps, "ms": ms, "model_bytes": 17 * N ** 3,
                               "fraction_of_8TBs": 17 * N ** 3 / (min(ms) * 1e-3) / 8e12}
        print(N + 1, "kappa_ingest", rep["kappa_ingest"], flush=True)
    for name in ("device", "refresh"):
        rep[name]["speedup_over_host"] = min(rep["host"]["s"]) / min(rep[name]["s"])
    return rep


def solve_times(top, n_levels):
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 8 << top
    gen = torch.Generator(device="cuda").manual_seed(5)
    logk = torch.randn(N ** 3, dtype=torch.float64, device="cuda", generator=gen)
    f = torch.randn((N + 1) ** 3, dtype=torch.float64, device="cuda", generator=gen)
    out = {"N": N, "levels": n_levels, "rtol": 1e-10}
    # (matrix_free_all: every level above the coarsest keeps kappa only, so a refresh rebuilds the 9^3 level and nothing else)
    for label, min_rows in (("stored", None), ("matrix_free", MF_MIN_ROWS), ("matrix_free_all", 0)):
        with DiffusionSolver(N, n_levels, rtol=out["rtol"], matrix_free_min_rows=min_rows) as solver:
            phases = {}
            generate, pcg = solver._generate, solver._pcg

            def timed(name, call):
                def run(*a):
                    t0 = time.perf_counter()
                    r = call(*a)
                    phases[name] = time.perf_counter() - t0
                    return r
                return run
            solver._generate, solver._pcg = timed("kappa_s", generate), timed("pcg_s", pcg)
            runs = []
            for step in range(3):           # kappa moves a little each time, as in an optimisation loop
                k = torch.exp(logk + 0.01 * step)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                solver.solve(k, f)
                torch.cuda.synchronize()
                runs.append({"forward_s": time.perf_counter() - t0, "how": solver.last_generate, **phases,
                             "iterations": solver.last_iterations["forward"]})
                print(label, runs[-1], flush=True)
            again = _wall(lambda: pcg(f, "forward"))
            out[label] = {"solves": runs, "pcg_alone_s": again, "pcg_alone_iterations": solver.last_iterations["forward"]}
            print(label, "mg_pcg alone", again, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tops", default="5,7")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--commit", default=None, help="what to record as the commit where git is not at hand")
    args = ap.parse_args()
    import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                           text=True).stdout.strip()
    with DeviceHierarchy(3, 0, 1) as h:
        machine = h.device_info()
    report = {"note": "tools/time_kappa_refresh.py: wall seconds per call, every call returning with the handle's stream synchronised; "
                      "'host' is gen_diffusion_hierarchy from a host array (uploaded, then the walk over the levels the device entry runs); "
                      "levels with at least 2^22 rows matrix-free; log-normal kappa (sigma 1); two repetitions per figure",
              "machine": machine, "torch": torch.__version__, "commit": commit or "working tree (no git at run time)",
              "hierarchy": {}}
    for top in (int(x) for x in args.tops.split(",")):
        report["hierarchy"][str((8 << top) + 1)] = hierarchy_times(top, args.reps)
    if not args.no_solve:
        report["solve_257"] = solve_times(5, 6)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
