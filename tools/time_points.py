"""The point family (mg_diffusion_points.hip.h) on 257^3 nodes with M = 10^4 and 10^6 random points:
  entries  mg_diffusion_point_sample, _load, _gradient and _gradient_t on device addresses, each call synchronous (checks, the
           coordinate check kernel, for the transposes the temporaries, the sort and the run sums included): --rounds interleaved
           rounds of --reps calls each, median and spread ((max - min) / median) of the ms per call
  torch    the same sums written with torch: the locate step with floor / argsort, S and G with gathers, S^T and G^T with
           index_add_ (whose order is not deterministic), same rounds
Recorded, not gated: these calls are small next to a solve.

    python tools/time_points.py [--N 256] [--points 10000,1000000] [--json profiles/diffusion_points_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENTRIES = ("sample", "load", "gradient", "gradient_t")


def summary(ms):
    med = statistics.median(ms)
    return {"ms": ms, "median_ms": med, "spread": (max(ms) - min(ms)) / med}


def torch_locate(pts, N):
    import torch
    n1 = N + 1
    t = pts * float(N)
    c = torch.clamp(torch.floor(t), max=N - 1)
    xi = t - c
    pi = torch.argsort(xi, dim=1, descending=True, stable=True)
    s = torch.gather(xi, 1, pi)
    stride = torch.tensor([1, n1, n1 * n1], device=pts.device)[pi]
    c = c.to(torch.int64)
    n0 = (c[:, 2] * n1 + c[:, 1]) * n1 + c[:, 0]
    nodes = n0[:, None] + torch.cat([torch.zeros_like(stride[:, :1]), torch.cumsum(stride, dim=1)], dim=1)
    lam = torch.stack([1.0 - s[:, 0], s[:, 0] - s[:, 1], s[:, 1] - s[:, 2], s[:, 2]], dim=1)
    return nodes, lam, pi


def torch_entry(name, N, pts, x, w, p):
    import torch
    nodes, lam, pi = torch_locate(pts, N)
    if name == "sample":
        return torch.sum(lam * x[nodes], dim=1)
    if name == "gradient":
        d = (x[nodes[:, 1:]] - x[nodes[:, :-1]]) * float(N)
        return torch.zeros_like(d).scatter_(1, pi, d)
    if name == "load":
        contrib = lam * w[:, None]
    else:
        P = torch.gather(p, 1, pi) * float(N)
        contrib = torch.cat([-P[:, :1], P[:, :-1] - P[:, 1:], P[:, 2:]], dim=1)
    return torch.zeros((N + 1) ** 3, dtype=torch.float64, device=pts.device).index_add_(0, nodes.reshape(-1), contrib.reshape(-1))


def times(N, M, reps, rounds):
    import torch
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    gen = torch.Generator(device="cuda").manual_seed(4)
    n = (N + 1) ** 3
    rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device="cuda", generator=gen)
    pts, x, w, p = rand(M, 3), rand(n) - 0.5, rand(M) - 0.5, rand(M, 3) - 0.5
    out = {"sample": torch.empty(M, dtype=torch.float64, device="cuda"), "gradient": torch.empty(3 * M, dtype=torch.float64, device="cuda"),
           "load": torch.empty(n, dtype=torch.float64, device="cuda"), "gradient_t": torch.empty(n, dtype=torch.float64, device="cuda")}
    operand = {"sample": x, "gradient": x, "load": w, "gradient_t": p}
    rep = {"N": N, "M": M, "reps": reps, "rounds": rounds}
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.set_level_grid(1)             # (the kernels read the grid's dimensions only)
        torch.cuda.synchronize()
        call = {k: (lambda k=k: getattr(h, "diffusion_point_" + k)(1, M, pts.data_ptr(), operand[k].data_ptr(), out[k].data_ptr()))
                for k in ENTRIES}
        for k in ENTRIES:
            call[k]()
            want = torch_entry(k, N, pts, x, w, p).reshape(-1)
            rep["max_abs_distance_to_torch_" + k] = float((out[k] - want).abs().max())
        ms = {k: [] for k in ENTRIES}
        ms_torch = {k: [] for k in ENTRIES}
        for _ in range(rounds):
            for k in ENTRIES:
                t0 = time.perf_counter()
                for _ in range(reps):
                    call[k]()
                ms[k].append((time.perf_counter() - t0) * 1e3 / reps)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    torch_entry(k, N, pts, x, w, p)
                torch.cuda.synchronize()
                ms_torch[k].append((time.perf_counter() - t0) * 1e3 / reps)
        for k in ENTRIES:
            rep[k] = summary(ms[k])
            rep["torch_" + k] = summary(ms_torch[k])
            rep["torch_over_entry_" + k] = rep["torch_" + k]["median_ms"] / rep[k]["median_ms"]
            print(N, M, k, rep[k]["median_ms"], "ms; torch", rep["torch_" + k]["median_ms"], "ms", flush=True)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--points", default="10000,1000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before libmg_hip.so is loaded: one HIP runtime for torch and the library)
    report = {"points": {}}
    for M in (int(m) for m in args.points.split(",")):
        report["points"][str(M)] = times(args.N, M, args.reps, args.rounds)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
