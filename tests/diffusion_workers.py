"""Helpers of tests/test_diffusion.py: coefficient fields, and the slab worker (spawned with torch.multiprocessing, one
process per slab on one GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def cell_x(N, dim):
    """x of every cell centre, in the cell order of poisson.diffusion_level (x fastest)."""
    x = (np.arange(N) + 0.5) / N
    return np.broadcast_to(x, (N,) * dim).reshape(-1)


def jump_kappa(N, dim, jump=1000.0):
    """The planar 1:jump field: jump for x < 1/2, 1 elsewhere (aligned on every level of an even hierarchy)."""
    return np.where(cell_x(N, dim) < 0.5, jump, 1.0)


def lognormal_kappa(N, dim, seed=0, sigma=1.0):
    """Cell-wise independent log-normal field exp(sigma * z), z ~ N(0, 1), seeded."""
    return np.exp(sigma * np.random.default_rng(seed).standard_normal(N ** dim))


def kappa_levels(kappa_top, dim, nlev, averaging="arithmetic"):
    """[kappa_0 .. kappa_top] coarsened with poisson.coarsen_kappa."""
    from multigrid_dolfinx_amd import poisson
    out = [np.asarray(kappa_top, dtype=np.float64)]
    for _ in range(nlev - 1):
        out.insert(0, poisson.coarsen_kappa(out[0], dim, averaging))
    return out


def gpu_diffusion_slab_worker(rank, world, port, dim, lo, hi, c, replicate_below):
    """Slabs of a log-normal diffusion hierarchy, built with per-level mg_gen_diffusion_level calls (every rank passes the
    whole kappa), give the single handle's V-cycle iterates bit for bit, replicated coarse levels included; the hierarchy
    entry is refused on slabs and leaves the handle usable."""
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from tests.dist_helpers import GlooTransport, init_gloo
    dist = init_gloo(rank, world, port)
    try:
        t = GlooTransport(dist, rank, world)

        def comm(h):
            h.set_comm_callbacks(rank, world, t.exchange, t.allreduce, t.allgatherv, replicate_below=replicate_below)

        kappa = lognormal_kappa(c << hi, dim, seed=5)
        with DeviceHierarchy.synthetic_diffusion(dim, lo, hi, kappa, c=c, comm=comm) as par, \
                DeviceHierarchy.synthetic_diffusion(dim, lo, hi, kappa, c=c) as ser:
            assert not par.level_info(hi)["replicated"]
            assert any(par.level_info(l)["replicated"] for l in range(lo, hi + 1))
            for l in range(lo, hi + 1):
                assert np.array_equal(par.get_vector(l, "f", gather=True), ser.get_vector(l, "f", gather=True)), l
            f = np.random.default_rng(9).standard_normal(par.n_dofs(hi))
            got = {}
            for name, h in (("par", par), ("ser", ser)):
                h.zero_vector(hi, "v")
                h.set_vector(hi, "f", f)
                h.vcycle(hi, 3)
                got[name] = h.get_vector(hi, "v", gather=True)
            assert np.array_equal(got["par"], got["ser"])
            try:
                par.gen_diffusion_hierarchy(kappa)
                raise AssertionError("mg_gen_diffusion_hierarchy accepted a slab handle")
            except MgError as exc:
                assert "slab" in str(exc), exc
            par.zero_vector(hi, "v")
            par.vcycle(hi, 3)
            assert np.array_equal(par.get_vector(hi, "v", gather=True), got["par"])
    finally:
        dist.destroy_process_group()
