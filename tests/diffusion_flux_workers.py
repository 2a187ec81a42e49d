"""Bodies of the DiffusionSolver tests of tests/test_diffusion_flux.py, and the host adjoint of the flux misfit they compare
with.  They run in a process of their own that imports torch before libmg_hip.so is loaded (one HIP runtime for both); each
prints its figures and ends with an "... ok" line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests.diffusion_adjoint_workers import host_solve  # noqa: E402


def host_flux_misfit(N, kappa, f, q_obs):
    """J = 1/2 h^3 ||q - q_obs||^2 with q = -F(kappa, u) and A(kappa) u = f: (J, u, q) with the host restatements."""
    u = host_solve(N, kappa, f)
    q = -poisson.diffusion_cell_gradient(N, kappa, u)
    return 0.5 * (1.0 / N) ** 3 * float(np.sum((q - q_obs) ** 2)), u, q


def host_flux_adjoint(N, kappa, f, q_obs):
    """(J, u, dJ/dkappa, dJ/df) of `host_flux_misfit` through one adjoint solve.  With r = q - q_obs the cotangent of
    F(kappa, u) is P = -h^3 r; kappa gets C(P, u) directly and u gets F^T(kappa, P), the right-hand side of the adjoint solve
    A lambda = u_bar; then dJ/df = lambda and kappa gets -D(lambda, u) more."""
    J, u, q = host_flux_misfit(N, kappa, f, q_obs)
    P = -((1.0 / N) ** 3) * (q - q_obs)
    lam = host_solve(N, kappa, poisson.diffusion_cell_gradient_t(N, kappa, P))
    return J, u, poisson.diffusion_cell_gradient_dot(N, P, u) - poisson.diffusion_dkappa(N, lam, u), lam


def _rel(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


# Relative l2 distance between the device gradients of J = 1/2 h^3 ||flux(kappa, u(kappa)) - q_obs||^2 (mg_pcg at rtol 1e-12,
# V(2,2) Jacobi) and the host adjoint above (spsolve).  The limit is 100 x the figure measured once on an MI355X, to leave
# room for PCG's stopping point moving by an iteration.
# Measured: grad_kappa 1.631e-12, grad_f 1.781e-12 (stored and matrix-free alike, 17 iterations each; u itself 9.0e-13, J
# 7.9e-14).  100 x the largest:
FLUX_GRADIENT_LIMIT = 1.8e-10


def _flux_case():
    from tests.diffusion_workers import lognormal_kappa
    N = 16
    rng = np.random.default_rng(31)
    kappa = lognormal_kappa(N, 3, seed=6)
    f = rng.standard_normal((N + 1) ** 3)
    q_obs = rng.standard_normal(3 * N ** 3)
    return N, kappa, f, q_obs


def gradcheck_worker():
    """torch.autograd.gradcheck and gradgradcheck at torch's default tolerances on `gradient` and `flux`, N = 4 and two
    levels: the maps are bilinear, so the differences are exact to rounding.  weight None and given, kappa on the device
    and on the CPU; before any solve, so through the grid-only top level."""
    import torch
    from torch.autograd import gradcheck, gradgradcheck
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 4
    rng = np.random.default_rng(5)
    with DiffusionSolver(N, 2) as solver:
        u = torch.tensor(rng.standard_normal((N + 1) ** 3), device="cuda", requires_grad=True)
        assert gradcheck(lambda x: solver.gradient(x), (u,))
        assert gradgradcheck(lambda x: solver.gradient(x), (u,))
        print("gradient(u) ok", flush=True)
        for where in ("cuda", "cpu"):
            w = torch.tensor(rng.standard_normal(N ** 3), device=where, requires_grad=True)
            k = torch.tensor(np.exp(rng.standard_normal(N ** 3)), device=where, requires_grad=True)
            assert gradcheck(lambda x, y: solver.gradient(y, weight=x), (w, u))
            assert gradgradcheck(lambda x, y: solver.gradient(y, weight=x), (w, u))
            assert gradcheck(solver.flux, (k, u))
            assert gradgradcheck(solver.flux, (k, u))
            q = solver.flux(k, u)
            assert q.shape == (3, N, N, N) and q.device == u.device
            assert torch.equal(q, -solver.gradient(u, weight=k))
            print("gradient(u, w) and flux(kappa, u) ok with the cell fields on", where, flush=True)
        assert solver.n_solves == 0 and solver.n_generations == 0
    print("gradcheck ok")


def end_to_end_worker(measure=False):
    """N = 16, two levels, log-normal kappa, rtol 1e-12, stored and matrix-free: grad_kappa and grad_f of
    J = 1/2 h^3 ||flux(kappa, u(kappa)) - q_obs||^2 against the host adjoint; n_solves is 2 for the gradient and 4 more for
    a Hessian-vector product with create_graph=True, all on one generation."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, f, q_obs = _flux_case()
    J, u, gk, gf = host_flux_adjoint(N, kappa, f, q_obs)
    h3 = (1.0 / N) ** 3
    worst = 0.0
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            k = torch.tensor(kappa, device="cuda", requires_grad=True)
            ft = torch.tensor(f, device="cuda", requires_grad=True)
            qo = torch.tensor(q_obs, device="cuda").view(3, N, N, N)
            misfit = lambda ut: 0.5 * h3 * torch.sum((solver.flux(k, ut) - qo) ** 2)
            ut = solver.solve(k, ft)
            assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
            Jt = misfit(ut)
            gkt, gft = torch.autograd.grad(Jt, (k, ft))
            assert solver.n_solves == 2, solver.n_solves
            host = lambda t: t.detach().cpu().numpy()
            figures = (_rel(host(ut), u), abs(float(Jt.detach()) - J) / J, _rel(host(gkt), gk), _rel(host(gft), gf))
            print(name, "iterations", solver.last_iterations, "rel l2: u %.3e  J %.3e  grad_kappa %.3e  grad_f %.3e" % figures, flush=True)
            worst = max(worst, figures[2], figures[3])
            if not measure:
                assert figures[2] <= FLUX_GRADIENT_LIMIT and figures[3] <= FLUX_GRADIENT_LIMIT, figures
            # a Hessian-vector product from scratch on the operator that is in place: forward, backward, and two more solves
            v = torch.tensor(np.random.default_rng(32).standard_normal(N ** 3) * kappa, device="cuda")
            g2, = torch.autograd.grad(misfit(solver.solve(k, ft, same_operator=True)), (k,), create_graph=True)
            hv, = torch.autograd.grad(torch.sum(g2 * v), (k,))
            assert solver.n_solves == 6, solver.n_solves
            assert solver.n_generations == 1, solver.n_generations
            assert torch.all(torch.isfinite(hv)) and float(hv.abs().max()) > 0.0
            print(name, "recorded gradient against the host adjoint %.3e" % _rel(host(g2), gk), flush=True)
            if not measure:
                assert _rel(host(g2), gk) <= FLUX_GRADIENT_LIMIT      # (the same gradient, recorded)
    print("largest relative l2 distance to the host adjoint %.3e" % worst, flush=True)
    print("end to end ok")


def non_interference_worker():
    """`gradient` before any solve works (grid-only top level) and has the bytes of the host restatement; the `solve` after it
    has the bytes of a solver that never called it; a `gradient` after the solve moves neither counter."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, f, _ = _flux_case()
    kt, ft = torch.tensor(kappa, device="cuda"), torch.tensor(f, device="cuda")
    x = np.random.default_rng(33).standard_normal((N + 1) ** 3)
    for min_rows in (None, 0):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as plain:
            want = plain.solve(kt, ft)
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            g = solver.gradient(torch.tensor(x, device="cuda"))
            assert g.shape == (3, N, N, N)
            assert g.cpu().numpy().tobytes() == poisson.diffusion_cell_gradient(N, None, x).tobytes()
            assert solver.n_solves == 0 and solver.n_generations == 0
            got = solver.solve(kt, ft)
            assert torch.equal(got, want)
            counts = (solver.n_solves, solver.n_generations)
            q = solver.flux(kt, got)
            assert q.cpu().numpy().tobytes() == (-poisson.diffusion_cell_gradient(N, kappa, got.cpu().numpy())).tobytes()
            assert (solver.n_solves, solver.n_generations) == counts
            assert torch.equal(solver.solve(kt, ft), want)
    print("non-interference ok")
