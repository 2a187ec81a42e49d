"""Solve to a tolerance with the reference's transfers against the P1 natural embedding and its transpose, on the
device-generated hierarchies of BASELINE configs 1-4.  For each of
  ref        injection + the reference's Q1 interpolation (the default), rediscretised levels
  p1         P1 prolongation + P^T restriction, rediscretised levels
  p1_gal     P1 prolongation + P^T restriction, Galerkin coarse levels (mg_galerkin_hierarchy from the finest level)
it reports finest-level V-cycles and seconds to ||r||_2 <= rtol ||f||_2 from zero for a loop of mg_vcycle, mg_pcg and FMG
(mu0 = 2, then cycles on the finest level).  FMG on Galerkin levels gets the generated right-hand sides of the coarse levels
through set_rhs_true (a Galerkin level starts with none).  --scale: Galerkin set-up time and device memory at
1025^3 -> 513^3 (wall clock of a first and a second call, device memory sampled with hipMemGetInfo during the first)
and the average time of the two transfer kernels there (mg_time_kernel).

    python tools/time_transfers_p1.py [--configs c1,c2,c3,c4] [--mus 2] [--rtol 1e-10] [--max 400] [--json out.json]
    python tools/time_transfers_p1.py --configs none --scale
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


def make(cfg, variant, mu):
    dim, lo, hi = CONFIGS[cfg]
    if variant == "p1_gal":
        h = DeviceHierarchy.galerkin_from_matrix(dim, lo, hi, c=8, mu1=mu, mu2=mu)
        with DeviceHierarchy.synthetic(dim, lo, hi - 1, c=8) as s:
            for l in range(lo, hi):
                h.set_rhs_true(l, s.get_vector(l, "f"))
        return h
    h = DeviceHierarchy.synthetic(dim, lo, hi, c=8, mu1=mu, mu2=mu)
    if variant == "p1":
        h.set_params(mu, mu, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
    return h


def run(cfg, variant, mu, rtol, max_it):
    dim, lo, hi = CONFIGS[cfg]
    row = {"config": cfg, "variant": variant, "mu": mu, "rtol": rtol}
    with make(cfg, variant, mu) as h:
        bn = h.norm2(hi, "f")
        h.zero_vector(hi, "v")
        h.vcycle(hi, 2)                       # warm-up: graphs, the direct coarsest solve, PCG work vectors
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
        row["pcg"] = {"s": dt, "cycles": len(hist), "reached": bool(len(hist) and hist[-1] <= rtol * bn),
                      "true_rel": h.norm2(hi, "r") / bn}

        dt, fh = timed(h, lambda: h.fmg(2, tol=rtol * bn, max_cycles=max_it, top_level=hi))
        row["fmg"] = {"s": dt, "cycles": len(fh), "reached": bool(len(fh) and fh[-1] <= rtol * bn)}
    return row


class DeviceMemorySampler:
    """Device memory in use, sampled with hipMemGetInfo every `period` seconds from a second thread while a call runs
    (ctypes releases the GIL around both): the peak of the samples is a lower bound of the true peak, the baseline the
    memory in use when sampling started.  Every process on the device counts."""

    def __init__(self, device=0, period=0.002):
        import ctypes
        import threading
        self._ct = ctypes
        self._hip = ctypes.CDLL("libamdhip64.so")
        self._hip.hipSetDevice(device)
        self._period = period
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)
        self.baseline = self.used()
        self.peak = self.baseline

    def used(self):
        free, total = self._ct.c_size_t(), self._ct.c_size_t()
        if self._hip.hipMemGetInfo(self._ct.byref(free), self._ct.byref(total)) != 0:
            raise RuntimeError("hipMemGetInfo failed")
        return total.value - free.value

    def _run(self):
        while not self._stop.is_set():
            self.peak = max(self.peak, self.used())
            self._stop.wait(self._period)

    def __enter__(self):
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()
        self.peak = max(self.peak, self.used())


def scale(reps):
    """1025^3 -> 513^3: Galerkin set-up (wall clock of a first and a second call on the same handle, device memory sampled
    during the first), memory held by the handle, transfer kernels."""
    out = {}
    h = DeviceHierarchy(3, 7, 8, c=4)
    try:
        h.gen_poisson_level(8)
        h.sync()
        before = h.memory_bytes()
        with DeviceMemorySampler(h.device) as mem:
            dt, _ = timed(h, lambda: h.galerkin(8))
        after = h.memory_bytes()
        dt2, _ = timed(h, lambda: h.galerkin(8))          # level 7 rebuilt: its storage is freed first
        nc = 513 ** 3
        out["galerkin_s_first"] = dt
        out["galerkin_s_second"] = dt2
        out["bytes_before"] = before
        out["bytes_after"] = after
        out["device_used_before"] = mem.baseline
        out["device_used_peak_sampled"] = mem.peak
        out["peak_over_before_sampled"] = mem.peak - mem.baseline
        # (what the buffer sizes say: the product's CSR, 15 entries per row, lives during the CSR builder's run)
        out["csr_temp_bytes"] = (nc + 1) * 8 + nc * 15 * 12
        out["coarse_info"] = h.level_info(7)
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_prolongation("p1")
        nf = 1025 ** 3
        for k, nbytes in (("restrict", 8 * nf + 8 * nc), ("prolong", 16 * nf + 8 * nc)):
            h.time_kernel(k, 8, 3)
            ms = h.time_kernel(k, 8, reps)
            out[k] = {"ms": ms, "bytes": nbytes, "TB_s": nbytes / ms / 1e9, "of_8TBs": nbytes / ms / 1e9 / 8.0}
    finally:
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c2,c3,c4")
    ap.add_argument("--variants", default="ref,p1,p1_gal")
    ap.add_argument("--mus", default="2")
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--max", type=int, default=400)
    ap.add_argument("--scale", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for cfg in [c for c in args.configs.split(",") if c in CONFIGS]:
        for mu in [int(m) for m in args.mus.split(",")]:
            for variant in args.variants.split(","):
                r = run(cfg, variant, mu, args.rtol, args.max)
                rows.append(r)
                f = lambda d: f"{d['cycles']:4d}{'' if d['reached'] else '+'} {d['s']:7.3f} s"
                print(f"{cfg} V({mu},{mu}) {variant:7s} vcycle {f(r['vcycle_loop'])} | pcg {f(r['pcg'])} | "
                      f"fmg {f(r['fmg'])}", flush=True)
    result = {"rows": rows}
    if args.scale:
        result["scale"] = scale(args.reps)
        s = result["scale"]
        print(f"galerkin 1025^3 -> 513^3: first call {s['galerkin_s_first']:.2f} s, second call {s['galerkin_s_second']:.2f} s; "
              f"handle {s['bytes_before'] / 1e9:.1f} -> {s['bytes_after'] / 1e9:.1f} GB; device in use "
              f"{s['device_used_before'] / 1e9:.1f} GB before, {s['device_used_peak_sampled'] / 1e9:.1f} GB peak "
              f"(sampled, +{s['peak_over_before_sampled'] / 1e9:.1f} GB)", flush=True)
        for k in ("restrict", "prolong"):
            print(f"{k} 1025^3: {s[k]['ms']:.3f} ms, {s[k]['TB_s']:.2f} TB/s = {s[k]['of_8TBs']:.2f} of 8 TB/s", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1, default=str)


if __name__ == "__main__":
    main()
