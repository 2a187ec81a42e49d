"""Worker for the slab test of `mg_pcg` (spawned with torch.multiprocessing, one process per slab on one GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def gpu_pcg_slab_worker(rank, world, port, dim, lo, hi, c, mu, replicate_below):
    """world processes share GPU 0 through the host-staged callback transport over gloo; the slab solve is checked against
    a single-handle solve on the same GPU.  The dot products are summed per rank and then across ranks, so the match is to
    round-off, not bit for bit."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from tests.dist_helpers import GlooTransport, init_gloo
    dist = init_gloo(rank, world, port)
    try:
        t = GlooTransport(dist, rank, world)

        def comm(h):
            h.set_comm_callbacks(rank, world, t.exchange, t.allreduce, t.allgatherv, replicate_below=replicate_below)

        with DeviceHierarchy.synthetic(dim, lo, hi, c=c, mu1=mu, mu2=mu, comm=comm) as par, \
                DeviceHierarchy.synthetic(dim, lo, hi, c=c, mu1=mu, mu2=mu) as ser:
            info = par.level_info(hi)
            assert not info["replicated"] and info["n_local"] < info["n_global"]
            f_before = par.get_vector(hi, "f", gather=True)
            for h in (par, ser):
                h.zero_vector(hi, "v")
            hp = par.pcg(rtol=0.0, max_iter=10)
            hs = ser.pcg(rtol=0.0, max_iter=10)
            assert len(hp) == len(hs) == 10
            assert np.all(np.abs(hp - hs) <= 1e-9 * hs), np.max(np.abs(hp - hs) / hs)
            xp = par.get_vector(hi, "v", gather=True)
            xs = ser.get_vector(hi, "v")
            assert np.linalg.norm(xp - xs) <= 1e-9 * np.linalg.norm(xs)
            assert np.array_equal(par.get_vector(hi, "f", gather=True), f_before)
            # to a tolerance: the same iteration count
            for h in (par, ser):
                h.zero_vector(hi, "v")
            hp = par.pcg(rtol=1e-10, max_iter=200)
            hs = ser.pcg(rtol=1e-10, max_iter=200)
            assert len(hp) == len(hs) and len(hs) < 200, (len(hp), len(hs))
    finally:
        dist.destroy_process_group()
