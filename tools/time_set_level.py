"""Wall time of one CSR hand-off (`set_level`), the set-up cost the host-side structural check (`mg_csr_check`) adds to.

    python tools/time_set_level.py [--n 128] [--dim 3] [--repeats 5] [--lib PATH/libmg_hip.so]

Hands the Poisson level of `poisson.make_level(n, dim)` (129^3 = 2.1 M rows by default) to a fresh level `repeats` times
after one warm-up and prints one JSON line with every time and the median.  `--lib` times another build of the library
(the parent commit's, say) in the same way; start one process per library.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    from multigrid_dolfinx_amd import _capi, poisson
    if args.lib:
        import ctypes
        _capi.LIB_PATH = os.path.abspath(args.lib)
        other = ctypes.CDLL(_capi.LIB_PATH)         # an older build may lack newer entry points: bind what it has
        _capi.SIGNATURES = {k: v for k, v in _capi.SIGNATURES.items() if hasattr(other, k)}
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    A = poisson.make_level(args.n, args.dim).A
    times = []
    with DeviceHierarchy(args.dim, 0, 1, c=args.n // 2) as h:
        for i in range(args.repeats + 1):
            h.sync()
            t0 = time.perf_counter()
            h.set_level(1, A)
            h.sync()
            if i:
                times.append(time.perf_counter() - t0)
    print(json.dumps({"lib": _capi.LIB_PATH, "rows": A.shape[0], "nnz": int(A.nnz), "set_level_s": times,
                      "median_s": statistics.median(times)}))


if __name__ == "__main__":
    main()
