"""Bodies of the DiffusionSolver tests of tests/test_diffusion_device_kappa.py.  They run in a process of their own that imports
torch before libmg_hip.so is loaded (one HIP runtime for both); each prints its figures and ends with an "... ok" line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.diffusion_adjoint_workers import GRADIENT_LIMIT, _gradient_case, _rel, host_adjoint  # noqa: E402
from tests.diffusion_workers import lognormal_kappa  # noqa: E402


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _misfit_gradients(solver, kappa, f, d):
    """One solve of J = 1/2 ||u - d||^2 and its backward pass with kappa on the device: (u, grad_kappa, grad_f) as tensors."""
    import torch
    k = torch.tensor(kappa, device="cuda", requires_grad=True)
    ft = torch.tensor(f, device="cuda", requires_grad=True)
    u = solver.solve(k, ft)
    (0.5 * torch.sum((u - torch.tensor(d, device="cuda")) ** 2)).backward()
    assert k.grad.shape == k.shape and k.grad.device == k.device
    return u.detach(), k.grad, ft.grad


def device_kappa_worker():
    """(a) N = 16, two levels, stored and matrix-free: "device" on the first solve, "refresh" on the second; both against the
    host adjoint; the refreshed u against a fresh solver's, as bytes."""
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa1, f, d = _gradient_case()
    kappa2 = lognormal_kappa(N, 3, seed=5)
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver, \
                DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as fresh:
            assert solver.last_generate is None
            for kappa, how in ((kappa1, "device"), (kappa2, "refresh")):
                before = solver.hierarchy.counters()
                u, gk, gf = _misfit_gradients(solver, kappa, f, d)
                assert solver.last_generate == how, (solver.last_generate, how)
                after = solver.hierarchy.counters()
                assert (after["uploads"], after["downloads"]) == (before["uploads"], before["downloads"])
                assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
                J, hu, hgk, hgf = host_adjoint(N, kappa, f, d)
                figures = (_rel(u.cpu().numpy(), hu), _rel(gk.cpu().numpy(), hgk), _rel(gf.cpu().numpy(), hgf))
                print(name, how, "iterations", solver.last_iterations, "rel l2: u %.3e  grad_kappa %.3e  grad_f %.3e" % figures,
                      flush=True)
                assert figures[1] <= GRADIENT_LIMIT and figures[2] <= GRADIENT_LIMIT, figures
            u_fresh, gk_fresh, gf_fresh = _misfit_gradients(fresh, kappa2, f, d)
            assert fresh.last_generate == "device"
            assert _bytes(u) == _bytes(u_fresh), name
            assert _bytes(gk) == _bytes(gk_fresh) and _bytes(gf) == _bytes(gf_fresh), name
    print("device kappa ok")


def stale_backward_worker():
    """(b) forward kappa_1, forward kappa_2, then the backward pass of the first: the hierarchy is refreshed from the copy the
    first solve kept and the gradient has the bytes of one taken straight away.  The caller's kappa_1 tensor is overwritten
    in between, as an optimiser would."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa1, f, d = _gradient_case()
    kappa2 = lognormal_kappa(N, 3, seed=5)
    dt = torch.tensor(d, device="cuda")
    for min_rows in (None, 0):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver, \
                DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as straight:
            _, gk_want, gf_want = _misfit_gradients(straight, kappa1, f, d)
            k1 = torch.tensor(kappa1, device="cuda", requires_grad=True)
            f1 = torch.tensor(f, device="cuda", requires_grad=True)
            J1 = 0.5 * torch.sum((solver.solve(k1, f1) - dt) ** 2)
            with torch.no_grad():
                k1.copy_(torch.tensor(kappa2, device="cuda"))           # the caller's tensor moves on
                solver.solve(k1, torch.tensor(f, device="cuda"))
            assert solver.last_generate == "refresh"
            generation = solver._generation
            J1.backward()
            assert solver._generation == generation + 1 and solver.last_generate == "refresh"
            assert _bytes(k1.grad) == _bytes(gk_want) and _bytes(f1.grad) == _bytes(gf_want), min_rows
    print("stale backward ok")


def cpu_kappa_worker():
    """(c) a kappa on the CPU takes the host path, first and later, and its gradient comes back on the CPU."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, f, d = _gradient_case()
    with DiffusionSolver(N, 2, rtol=1e-12) as solver:
        for _ in range(2):
            k = torch.tensor(kappa, requires_grad=True)
            u = solver.solve(k, torch.tensor(f, device="cuda"))
            assert solver.last_generate == "host"
            torch.sum(u).backward()
            assert k.grad.device.type == "cpu"
        # a device kappa after a host one refreshes the levels the host call generated
        solver.solve(torch.tensor(kappa, device="cuda"), torch.tensor(f, device="cuda"))
        assert solver.last_generate == "refresh"
    print("cpu kappa ok")


def warm_start_worker():
    """(d) N = 32, three levels, random f, kappa_2 = kappa_1 (1 + 0.01 eta), eta uniform in [-1, 1].  A warm solve of kappa_2
    starts from u_1, whose residual is about 3e-3 ||f||; the cold one starts at ||f||."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, rtol = 32, 1e-10
    rng = np.random.default_rng(12)
    kappa1 = lognormal_kappa(N, 3, seed=6)
    kappa2 = kappa1 * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, N ** 3))
    f = torch.tensor(rng.standard_normal((N + 1) ** 3), device="cuda")
    counts, residuals, us = {}, {}, {}
    for warm in (False, True):
        with DiffusionSolver(N, 3, rtol=rtol, warm_start=warm) as solver:
            solver.solve(torch.tensor(kappa1, device="cuda"), f)
            first = solver.last_iterations["forward"]
            us[warm] = solver.solve(torch.tensor(kappa2, device="cuda"), f)
            counts[warm], residuals[warm] = solver.last_iterations["forward"], solver.last_residual["forward"]
            print("warm_start", warm, "iterations: kappa_1", first, "kappa_2", counts[warm], "||r|| / ||f||", residuals[warm],
                  flush=True)
    print("forward iterations of kappa_2: cold", counts[False], "warm", counts[True], flush=True)
    assert counts[True] <= counts[False], counts
    for warm in (False, True):
        assert residuals[warm] is not None and residuals[warm] <= rtol, residuals
    print("warm against cold u, rel l2: %.3e" % _rel(us[True].cpu().numpy(), us[False].cpu().numpy()), flush=True)
    print("warm start ok")
