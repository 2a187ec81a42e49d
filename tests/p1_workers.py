"""Worker for the slab test of the P1 transfers (spawned with torch.multiprocessing, one process per slab on one GPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def gpu_p1_slab_worker(rank, world, port, dim, lo, hi, c, replicate_below):
    """world processes share GPU 0 through the host-staged callback transport over gloo.  The P1 prolongation (add 0 and 1)
    and P^T on the slabs equal the single handle's bit for bit (the Kuhn-pattern check's verdict is all-reduced on the way);
    whole V(2,2) cycles agree to round-off (the norms are all-reduced); mg_galerkin_level refuses a slab."""
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
            rng = np.random.default_rng(17)
            for h in (par, ser):
                h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", keep_err=True)
                h.set_prolongation("p1")
            for l in range(lo + 1, hi + 1):
                vc = rng.standard_normal(par.n_dofs(l - 1))
                vf = rng.standard_normal(par.n_dofs(l))
                rf = rng.standard_normal(par.n_dofs(l))
                got = {}
                for name, h in (("par", par), ("ser", ser)):
                    h.set_vector(l - 1, "v", vc)
                    h.set_vector(l, "v", vf)
                    h.prolong(l, add=False)
                    e0 = h.get_vector(l, "err", gather=True)
                    h.prolong(l, add=True)
                    v1 = h.get_vector(l, "v", gather=True)
                    h.set_vector(l, "r", rf)
                    h.restrict(l, "p1_transpose")
                    got[name] = (e0, v1, h.get_vector(l - 1, "f", gather=True))
                for a, b in zip(got["par"], got["ser"]):
                    assert np.array_equal(a, b), l
            f = rng.standard_normal(par.n_dofs(hi))
            hist = {}
            for name, h in (("par", par), ("ser", ser)):
                h.zero_vector(hi, "v")
                h.set_vector(hi, "f", f)
                hist[name] = h.vcycle(hi, 4, residuals=True)
            assert np.all(np.abs(hist["par"] - hist["ser"]) <= 1e-12 * hist["ser"]), (hist["par"], hist["ser"])
            # Galerkin levels need a whole fine level: every rank refuses alike
            from multigrid_dolfinx_amd._capi import MgError
            try:
                par.galerkin_level(hi)
                raise AssertionError("mg_galerkin_level accepted a slab")
            except MgError as exc:
                assert "not a slab" in str(exc), exc
    finally:
        dist.destroy_process_group()
