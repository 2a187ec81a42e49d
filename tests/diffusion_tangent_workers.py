"""Bodies of the DiffusionSolver tests of tests/test_diffusion_tangent.py, and the host references they compare with: the
tangent solve and the Hessian-vector product of J = 1/2 ||u - d||^2 built on scipy's spsolve, poisson.diffusion_dkappa and
poisson.diffusion_apply_dkappa.  The torch bodies run in a process of their own that imports torch before libmg_hip.so is
loaded (one HIP runtime for both); each prints its figures and ends with an "... ok" line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests.diffusion_adjoint_workers import _gradient_case, _rel, host_solve  # noqa: E402

EPS = np.finfo(np.float64).eps


_EDGES = ((2, 0), (1, 0), (0, 0), (0, 1), (1, 1), (2, 1))       # (axis, side) of z-, y-, x-, x+, y+, z+


def _rows(N, cells, x):
    """Per node: the six edge sums of `cells` (se[axis][side]) and their sum, the x value of the six neighbours in the order
    of _EDGES with a boundary neighbour taken as 0, and the mask of the interior rows."""
    n1 = N + 1
    se, t = poisson._edge_sums_3d(np.pad(np.asarray(cells, dtype=np.float64).reshape(N, N, N), 1, constant_values=1.0), n1)
    idx = np.arange(n1 ** 3, dtype=np.int64)
    ijk = [idx % n1, (idx // n1) % n1, idx // (n1 * n1)]
    inner = np.ones(n1 ** 3, dtype=bool)
    for c in ijk:
        inner &= (c >= 1) & (c <= N - 1)
    strides = (1, n1, n1 * n1)
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    xp = np.concatenate([np.zeros(strides[2]), v, np.zeros(strides[2])])
    neighbours = []
    for axis, side in _EDGES:
        delta = strides[axis] if side else -strides[axis]
        on_boundary = ijk[axis] + (1 if side else -1) == (N if side else 0)
        neighbours.append(np.where(on_boundary, 0.0, xp[strides[2] + delta:strides[2] + delta + v.size]))
    return se, t, neighbours, v, inner


def row_terms(N, dkappa, x):
    """The products an interior row of (dA/dkappa . dkappa) x sums: the diagonal's and the six neighbours', [7, nodes]."""
    h = 1.0 / N
    se, t, neighbours, v, _ = _rows(N, dkappa, x)
    return np.array([((t / 6.0) * h) * v] + [-((se[axis][side] / 6.0) * h) * xj for (axis, side), xj in zip(_EDGES, neighbours)])


def row_bound(N, dkappa, x):
    """Per row i: 16 eps (h / 6) sum over the row's six edges e = (i, j) of (sum_c n_c |dkappa_c|) (|x_i| + |x~_j|), x~ = x with
    the boundary nodes taken as 0.  On the absolute values of the cell terms: an edge sum of a sign-indefinite dkappa can
    cancel, and what it is the sum of still carries its rounding.  0 on boundary rows."""
    se, _, neighbours, v, inner = _rows(N, np.abs(dkappa), np.abs(x))
    s = np.zeros(v.size)
    for (axis, side), xj in zip(_EDGES, neighbours):
        s += se[axis][side] * (v + xj)
    return np.where(inner, 16 * EPS * ((1.0 / N) / 6.0) * s, 0.0)


def host_tangent(N, kappa, f, dkappa, df):
    u = host_solve(N, kappa, f)
    return u, host_solve(N, kappa, df - poisson.diffusion_apply_dkappa(N, dkappa, u))


def host_hessian_vector(N, kappa, f, d, v):
    """J = 1/2 ||u - d||^2 with A(kappa) u = f, g = dJ/dkappa = -D(lambda, u), A lambda = u - d.  In the direction v of kappa:
    A du = -T(v, u), A dlambda = du - T(v, lambda), and (d2J/dkappa2 v, d(g . v)/df) = (-D(dlambda, u) - D(lambda, du), dlambda):
    four solves."""
    u = host_solve(N, kappa, f)
    lam = host_solve(N, kappa, u - d)
    du = host_solve(N, kappa, -poisson.diffusion_apply_dkappa(N, v, u))
    dlam = host_solve(N, kappa, du - poisson.diffusion_apply_dkappa(N, v, lam))
    return -poisson.diffusion_dkappa(N, dlam, u) - poisson.diffusion_dkappa(N, lam, du), dlam


# Relative l2 distance between the device results (mg_pcg at rtol 1e-12, V(2,2) Jacobi) and the host references above
# (spsolve): du of `tangent`, and the kappa and f blocks of the Hessian-vector product.  The limit is 100 x the largest
# figure measured once on an MI355X, the margin GRADIENT_LIMIT takes for PCG's stopping point moving by an iteration, and
# never looser than 1e-6.
# Measured (stored and matrix-free alike, 17 iterations per solve): du 3.038e-13 (df = None: 4.592e-13; u itself 2.5e-13),
# H_kk v 8.913e-13, H_fk v 1.372e-12; stored against matrix-free 2.1e-16 / 6.4e-16 / 7.7e-16.  100 x the largest:
SECOND_ORDER_LIMIT = 1.4e-10


def _second_order_case():
    N, kappa, f, d = _gradient_case()
    rng = np.random.default_rng(22)
    return N, kappa, f, d, rng.standard_normal(N ** 3), rng.standard_normal((N + 1) ** 3), rng.standard_normal(N ** 3)


def tangent_worker():
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, f, d, dkappa, df, _ = _second_order_case()
    u, du = host_tangent(N, kappa, f, dkappa, df)
    got = {}
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            ut, dut = solver.tangent(torch.tensor(kappa), torch.tensor(f, device="cuda"), torch.tensor(dkappa, device="cuda"),
                                     torch.tensor(df, device="cuda"))
            assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
            got[name] = dut.cpu().numpy().copy()
            figures = (_rel(ut.cpu().numpy(), u), _rel(got[name], du))
            print(name, "iterations", solver.last_iterations, "rel l2: u %.3e  du %.3e" % figures, flush=True)
            assert solver._generation == 1 and solver.last_generate == "host", (solver._generation, solver.last_generate)
            assert solver.n_solves == 2, solver.n_solves
            assert set(solver.last_iterations) == {"forward", "tangent"}
            assert figures[1] <= SECOND_ORDER_LIMIT, figures
            # df = None is df = 0
            _, du0 = solver.tangent(torch.tensor(kappa), torch.tensor(f, device="cuda"), torch.tensor(dkappa, device="cuda"))
            assert solver.n_solves == 4 and solver._generation == 2
    du0_host = host_tangent(N, kappa, f, dkappa, np.zeros_like(df))[1]
    print("df = None: rel l2 du %.3e" % _rel(du0.cpu().numpy(), du0_host), flush=True)
    assert _rel(du0.cpu().numpy(), du0_host) <= SECOND_ORDER_LIMIT
    between = _rel(got["matrix_free"], got["stored"])
    print("stored against matrix-free: du %.3e" % between, flush=True)
    assert between <= SECOND_ORDER_LIMIT
    print("tangent ok")


def hessian_worker():
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, f, d, _, _, v = _second_order_case()
    hk, hf = host_hessian_vector(N, kappa, f, d, v)
    got = {}
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            k = torch.tensor(kappa, requires_grad=True)                 # on the CPU
            ft = torch.tensor(f, device="cuda", requires_grad=True)
            before = solver.n_solves
            J = 0.5 * torch.sum((solver.solve(k, ft) - torch.tensor(d, device="cuda")) ** 2)
            (g,) = torch.autograd.grad(J, k, create_graph=True)
            assert solver.n_solves == before + 2, solver.n_solves
            gk, gf = torch.autograd.grad(torch.sum(g * torch.tensor(v)), (k, ft))
            assert solver.n_solves == before + 4, solver.n_solves
            assert solver._generation == 1 and solver.last_generate == "host", (solver._generation, solver.last_generate)
            assert set(solver.last_iterations) == {"forward", "adjoint"}
            assert gk.shape == k.shape and gk.device == k.device and gf.shape == ft.shape and gf.device == ft.device
            got[name] = (gk.numpy().copy(), gf.cpu().numpy().copy())
            figures = (_rel(got[name][0], hk), _rel(got[name][1], hf))
            print(name, "iterations", solver.last_iterations, "rel l2: H_kk v %.3e  H_fk v %.3e" % figures, flush=True)
            assert max(figures) <= SECOND_ORDER_LIMIT, figures
    between = (_rel(got["matrix_free"][0], got["stored"][0]), _rel(got["matrix_free"][1], got["stored"][1]))
    print("stored against matrix-free: H_kk v %.3e  H_fk v %.3e" % between, flush=True)
    assert max(between) <= SECOND_ORDER_LIMIT, between
    print("hessian ok")


def first_order_worker():
    """A plain backward is what it was: two solves in all, one generation, the warm-start solutions kept.  A backward pass
    that records gradients leaves the kept solutions alone, and a kappa on the device works through the double backward as
    well (it reaches the hierarchy once, as a refresh)."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, f, d, _, _, v = _second_order_case()
    with DiffusionSolver(N, 2, rtol=1e-12, warm_start=True) as solver:
        k = torch.tensor(kappa, requires_grad=True)
        J = 0.5 * torch.sum((solver.solve(k, torch.tensor(f, device="cuda")) - torch.tensor(d, device="cuda")) ** 2)
        J.backward()
        assert solver.n_solves == 2, solver.n_solves
        assert set(solver.last_iterations) == {"forward", "adjoint"} and set(solver.last_residual) == {"forward", "adjoint"}
        assert solver._generation == 1
        assert set(solver._warm) == {"forward", "adjoint"}
        first = k.grad.numpy().copy()
        # under create_graph the nested solves start from zero and leave the kept solutions alone
        kept = {w: x.clone() for w, x in solver._warm.items()}
        kd = torch.tensor(kappa, device="cuda", requires_grad=True)
        J = 0.5 * torch.sum((solver.solve(kd, torch.tensor(f, device="cuda")) - torch.tensor(d, device="cuda")) ** 2)
        kept["forward"] = solver._warm["forward"].clone()
        (g,) = torch.autograd.grad(J, kd, create_graph=True)
        assert solver.n_solves == 4 and all(torch.equal(solver._warm[w], kept[w]) for w in kept)
        (hv,) = torch.autograd.grad(torch.sum(g * torch.tensor(v, device="cuda")), kd)      # (records nothing: an ordinary backward pass)
        assert solver.n_solves == 6 and solver._generation == 2 and solver.last_generate == "refresh", (solver.n_solves, solver._generation)
        hk, _ = host_hessian_vector(N, kappa, f, d, v)
        print("device kappa: rel l2 gradient %.3e (against the first)  H_kk v %.3e" %
              (_rel(g.detach().cpu().numpy(), first), _rel(hv.cpu().numpy(), hk)), flush=True)
        assert _rel(g.detach().cpu().numpy(), first) <= SECOND_ORDER_LIMIT and _rel(hv.cpu().numpy(), hk) <= SECOND_ORDER_LIMIT
    print("first order ok")
