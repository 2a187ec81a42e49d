"""Worker for the slab test of the Chebyshev smoother (spawned with torch.multiprocessing, one process per slab on one GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def gpu_cheb_slab_worker(rank, world, port, dim, lo, hi, c, replicate_below):
    """world processes share GPU 0 through the host-staged callback transport over gloo.  With the intervals set explicitly
    the slab smoother and whole V(2,2) cycles equal the single handle bit for bit (one step per launch, halo of v after each
    step); with estimated intervals every rank reports the same bits, within 1e-10 of the single handle's estimate."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from tests.dist_helpers import GlooTransport, init_gloo
    dist = init_gloo(rank, world, port)
    try:
        t = GlooTransport(dist, rank, world)

        def comm(h):
            h.set_comm_callbacks(rank, world, t.exchange, t.allreduce, t.allgatherv, replicate_below=replicate_below)

        with DeviceHierarchy.synthetic(dim, lo, hi, c=c, mu1=2, mu2=2, comm=comm) as par, \
                DeviceHierarchy.synthetic(dim, lo, hi, c=c, mu1=2, mu2=2) as ser:
            assert not par.level_info(hi)["replicated"]
            for h in (par, ser):
                h.set_params(2, 2, 0.0, restriction="p1_transpose", smoother="chebyshev")
                h.set_prolongation("p1")
            # estimated intervals: the same bits on every rank, round-off of the single handle's
            for l in range(lo + 1, hi + 1):
                bp, bs = par.chebyshev_bounds(l), ser.chebyshev_bounds(l)
                mine = np.array([bp["lmin"], bp["lmax"], bp["lmax_estimate"]])
                every = [np.zeros(3) for _ in range(world)]
                dist.all_gather_object(every, mine)
                assert all(np.array_equal(mine, e) for e in every), every
                assert abs(bp["lmax_estimate"] - bs["lmax_estimate"]) <= 1e-10 * bs["lmax_estimate"], (bp, bs)
            # explicit intervals: bit for bit
            for h in (par, ser):
                for l in range(lo + 1, hi + 1):
                    h.set_chebyshev_bounds(l, 0.3, 2.1)
            rng = np.random.default_rng(5)
            for m in (1, 3):
                v0 = rng.standard_normal(par.n_dofs(hi))
                f = rng.standard_normal(par.n_dofs(hi))
                got = {}
                for name, h in (("par", par), ("ser", ser)):
                    h.set_vector(hi, "v", v0)
                    h.set_vector(hi, "f", f)
                    h.smooth(hi, m)
                    got[name] = h.get_vector(hi, "v", gather=True)
                assert np.array_equal(got["par"], got["ser"]), m
            f = rng.standard_normal(par.n_dofs(hi))
            got = {}
            for name, h in (("par", par), ("ser", ser)):
                h.zero_vector(hi, "v")
                h.set_vector(hi, "f", f)
                h.vcycle(hi, 2)
                got[name] = h.get_vector(hi, "v", gather=True)
            assert np.array_equal(got["par"], got["ser"])
    finally:
        dist.destroy_process_group()
