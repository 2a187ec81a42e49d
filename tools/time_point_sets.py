"""Located point sets (mg_points_*; mg_diffusion_points.hip.h) on 257^3 nodes with M = 10^4 and 10^6 uniformly random points
and B = 1, 4, 8 lanes, by the method of tools/time_points.py: --rounds interleaved rounds of --reps synchronous calls each,
median and spread ((max - min) / median) of the ms per call.
  loop     B calls of mg_diffusion_point_sample / _load / _gradient / _gradient_t, one per lane (check kernel, and for the
           transposes the temporaries, the sort and the run sums, every time)
  set      one call of mg_points_sample / _load / _gradient / _gradient_t for the B lanes on a set made beforehand
  create   mg_points_create + mg_points_destroy on its own
  groups   the set calls at the largest B with 1, 2, 4 and 8 lanes per launch (MG_POINT_GROUP), ms per lane relative to 4
Recorded, not gated.

    python tools/time_point_sets.py [--N 256] [--points 10000,1000000] [--lanes 1,4,8] [--json profiles/diffusion_point_sets_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENTRIES = ("sample", "load", "gradient", "gradient_t")
GROUPS = (1, 2, 4, 8)


def summary(ms):
    med = statistics.median(ms)
    return {"ms": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med}


def timed(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t0) * 1e3 / reps


def hierarchy(N, group=None):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    if group is None:
        os.environ.pop("MG_POINT_GROUP", None)
    else:
        os.environ["MG_POINT_GROUP"] = str(group)       # read once, when the handle is made
    h = DeviceHierarchy(3, 0, 1, c=N // 2)
    os.environ.pop("MG_POINT_GROUP", None)
    h.set_level_grid(1)                                 # (the kernels read the grid's dimensions only)
    return h


def times(N, M, lanes, reps, rounds):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(4)
    n = (N + 1) ** 3
    Bmax = max(lanes)
    rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen)
    pts = rand(M, 3)
    operand = {"sample": rand(Bmax, n) - 0.5, "load": rand(Bmax, M) - 0.5, "gradient_t": rand(Bmax, 3 * M) - 0.5}
    operand["gradient"] = operand["sample"]
    empty = lambda count: torch.empty((Bmax, count), dtype=torch.float64, device="cuda")
    out = {"sample": empty(M), "gradient": empty(3 * M), "load": empty(n), "gradient_t": empty(n)}
    check = {k: torch.empty_like(out[k]) for k in ENTRIES}
    ptrs = lambda t, B: [t.data_ptr() + 8 * t.shape[1] * b for b in range(B)]
    rep = {"N": N, "M": M, "reps": reps, "rounds": rounds, "lanes": {}}
    torch.cuda.synchronize()
    with hierarchy(N) as h:
        ps = h.points(1, (pts.data_ptr(), M))
        rep["info"] = ps.info
        rep["bytes_per_point"] = ps.info["bytes"] / M
        loop = lambda k, B, dst=out: [getattr(h, "diffusion_point_" + k)(1, M, pts.data_ptr(), i, o)
                                      for i, o in zip(ptrs(operand[k], B), ptrs(dst[k], B))]
        one = lambda k, B: getattr(ps, k + "_many")(ptrs(operand[k], B), ptrs(out[k], B))
        for k in ENTRIES:                               # warm-up, and the bytes of both ways once
            loop(k, Bmax, check)
            one(k, Bmax)
            rep["same_bytes_" + k] = bool(torch.equal(out[k].view(torch.int64), check[k].view(torch.int64)))
        for B in lanes:
            ms_loop, ms_set = {k: [] for k in ENTRIES}, {k: [] for k in ENTRIES}
            for _ in range(rounds):
                for k in ENTRIES:
                    ms_loop[k].append(timed(lambda: loop(k, B), reps))
                    ms_set[k].append(timed(lambda: one(k, B), reps))
            r = rep["lanes"][str(B)] = {}
            for k in ENTRIES:
                r["loop_" + k], r["set_" + k] = summary(ms_loop[k]), summary(ms_set[k])
                r["loop_over_set_" + k] = r["loop_" + k]["median_ms"] / r["set_" + k]["median_ms"]
                print(N, M, B, k, "loop %.4f ms (spread %.0f %%), set %.4f ms (spread %.0f %%), ratio %.2f"
                      % (r["loop_" + k]["median_ms"], 100 * r["loop_" + k]["spread"], r["set_" + k]["median_ms"],
                         100 * r["set_" + k]["spread"], r["loop_over_set_" + k]), flush=True)
        ps.close()
        create = lambda: h.points(1, (pts.data_ptr(), M)).close()
        create()
        rep["create"] = summary([timed(create, max(1, reps // 2)) for _ in range(rounds)])
        print(N, M, "create %.4f ms (spread %.0f %%)" % (rep["create"]["median_ms"], 100 * rep["create"]["spread"]), flush=True)
    # launch-group candidates: one handle per group size, the set calls at the largest B, rounds interleaved over the sizes
    handles = {g: hierarchy(N, g) for g in GROUPS}
    sets = {g: handles[g].points(1, (pts.data_ptr(), M)) for g in GROUPS}
    ms = {g: {k: [] for k in ENTRIES} for g in GROUPS}
    for g in GROUPS:
        for k in ENTRIES:
            getattr(sets[g], k + "_many")(ptrs(operand[k], Bmax), ptrs(out[k], Bmax))
    for _ in range(rounds):
        for k in ENTRIES:
            for g in GROUPS:
                ms[g][k].append(timed(lambda: getattr(sets[g], k + "_many")(ptrs(operand[k], Bmax), ptrs(out[k], Bmax)), reps))
    rep["groups"] = {"lanes": Bmax}
    for g in GROUPS:
        rep["groups"][str(g)] = {k: summary(ms[g][k]) for k in ENTRIES}
    for g in GROUPS:
        for k in ENTRIES:
            ratio = rep["groups"][str(g)][k]["median_ms"] / rep["groups"]["4"][k]["median_ms"]
            rep["groups"][str(g)][k]["per_lane_over_group_4"] = ratio
            print(N, M, "group", g, k, "%.4f ms per lane, %.2f of group 4" % (rep["groups"][str(g)][k]["median_ms"] / Bmax, ratio), flush=True)
    for g in GROUPS:
        sets[g].close()
        handles[g].close()
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--points", default="10000,1000000")
    ap.add_argument("--lanes", default="1,4,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    report = {"points": {}}
    lanes = [int(b) for b in args.lanes.split(",")]
    for M in (int(m) for m in args.points.split(",")):
        report["points"][str(M)] = times(args.N, M, lanes, args.reps, args.rounds)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
