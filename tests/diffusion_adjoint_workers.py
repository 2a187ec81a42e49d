"""Bodies of the DiffusionSolver tests of tests/test_diffusion_adjoint.py, and the host adjoint they compare with.  They run in
a process of their own that imports torch before libmg_hip.so is loaded (one HIP runtime for both); each prints its figures
and ends with an "... ok" line."""
import os
import sys

import numpy as np
import scipy.sparse.linalg as spl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402


def host_solve(N, kappa, rhs):
    return spl.spsolve(poisson.diffusion_level(N, 3, kappa).A.tocsc(), rhs)


def host_adjoint(N, kappa, f, d):
    """J = 1/2 ||u - d||^2 with A(kappa) u = f: (J, u, dJ/dkappa, dJ/df) through one adjoint solve."""
    u = host_solve(N, kappa, f)
    lam = host_solve(N, kappa, u - d)
    return 0.5 * float(np.sum((u - d) ** 2)), u, -poisson.diffusion_dkappa(N, lam, u), lam


# Relative l2 distance between the device gradient (mg_pcg at rtol 1e-12, V(2,2) Jacobi) and the host adjoint (spsolve).
# The limit is 100 x the figure measured once on an MI355X, to leave room for PCG's stopping point moving by an iteration,
# and never looser than 1e-6: past that a wrong edge weight would pass as round-off.
# Measured: grad_kappa 3.453e-13, grad_f 5.6e-14 (stored and matrix-free alike; u itself 2.5e-13), stored against
# matrix-free 4.6e-16 / 1.4e-16.  100 x the largest:
GRADIENT_LIMIT = 3.5e-11


def _gradient_case():
    from tests.diffusion_workers import lognormal_kappa
    N = 16
    rng = np.random.default_rng(21)
    kappa = lognormal_kappa(N, 3, seed=4)
    f, d = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    return N, kappa, f, d


def _rel(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


def gradient_worker():
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, f, d = _gradient_case()
    J, u, gk, gf = host_adjoint(N, kappa, f, d)
    got = {}
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            k = torch.tensor(kappa, requires_grad=True)                 # on the CPU
            ft = torch.tensor(f, device="cuda", requires_grad=True)
            ut = solver.solve(k, ft)
            assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
            Jt = 0.5 * torch.sum((ut - torch.tensor(d, device="cuda")) ** 2)
            Jt.backward()
            got[name] = (k.grad.numpy().copy(), ft.grad.cpu().numpy().copy())
            figures = (_rel(ut.detach().cpu().numpy(), u), abs(float(Jt) - J) / J, _rel(got[name][0], gk), _rel(got[name][1], gf))
            print(name, "iterations", solver.last_iterations, "rel l2: u %.3e  J %.3e  grad_kappa %.3e  grad_f %.3e" % figures, flush=True)
            assert k.grad.shape == k.shape and ft.grad.shape == ft.shape
            assert figures[2] <= GRADIENT_LIMIT and figures[3] <= GRADIENT_LIMIT, figures
    between = (_rel(got["matrix_free"][0], got["stored"][0]), _rel(got["matrix_free"][1], got["stored"][1]))
    print("stored against matrix-free: grad_kappa %.3e  grad_f %.3e" % between, flush=True)
    assert max(between) <= GRADIENT_LIMIT, between
    print("gradient ok")


def sgd_worker():
    """The step is sized from the first gradient (a move of at most 0.1 in log kappa), so the descent does not depend on the
    scale of J."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 32
    rng = np.random.default_rng(8)
    logk = torch.tensor(rng.standard_normal(N ** 3) * 0.5, device="cuda", requires_grad=True)      # kappa from the device
    f = torch.tensor(rng.standard_normal((N + 1) ** 3), device="cuda")
    d = torch.tensor(rng.standard_normal((N + 1) ** 3), device="cuda")
    with DiffusionSolver(N, 3, rtol=1e-10) as solver:
        misfit = lambda: 0.5 * torch.sum((solver.solve(torch.exp(logk), f) - d) ** 2)
        history = []
        opt = None
        for step in range(2):
            J = misfit()
            history.append(float(J))
            if opt is not None:
                opt.zero_grad()
            J.backward()
            g = logk.grad
            assert torch.all(torch.isfinite(g)) and torch.all(g != 0.0)
            if opt is None:
                opt = torch.optim.SGD([logk], lr=0.1 / float(g.abs().max()))
            opt.step()
        with torch.no_grad():
            history.append(float(misfit()))
    print("J:", history, flush=True)
    assert history[2] < history[1] < history[0], history
    print("sgd ok")


def max_iter_worker():
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver, NotConverged
    N, kappa, f, d = _gradient_case()
    with DiffusionSolver(N, 2, rtol=1e-12) as solver:
        k = torch.tensor(kappa, requires_grad=True)
        J = 0.5 * torch.sum((solver.solve(k, torch.tensor(f, device="cuda")) - torch.tensor(d, device="cuda")) ** 2)
        solver.max_iter = 1
        try:
            J.backward()
            raise AssertionError("the adjoint solve stopped at max_iter = 1 and a gradient came back")
        except NotConverged as exc:
            assert "adjoint solve reached max_iter" in str(exc), exc
        assert k.grad is None
    with DiffusionSolver(N, 2, rtol=1e-12, max_iter=1) as solver:
        try:
            solver.solve(torch.tensor(kappa), torch.tensor(f, device="cuda"))
            raise AssertionError("the forward solve stopped at max_iter = 1 and a solution came back")
        except NotConverged as exc:
            assert "forward solve reached max_iter" in str(exc), exc
    print("max_iter ok")
