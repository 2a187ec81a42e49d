"""Host references and DiffusionSolver test bodies of tests/test_diffusion_reaction.py: the reaction field, the solve, the adjoint
and the four-solve Hessian-vector products of -div(kappa grad u) + sigma u = f with the lumped reaction term, and an implicit
Euler march with its adjoint recursion, built on scipy's sparse direct solves and the restatements of poisson.py.  The torch
bodies run in a process of their own that imports torch before libmg_hip.so is loaded (one HIP runtime for both); each prints
its figures and ends with an "... ok" line."""
import os
import sys

import numpy as np
import scipy.sparse.linalg as spl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests.diffusion_neumann_workers import free_mask, lifted_rhs  # noqa: E402

EPS = np.finfo(np.float64).eps


def reaction_sigma(N, seed=7):
    """A cell-wise independent log-normal field, its logarithm rescaled so that sigma h^2 spans 1e-3 .. 1: rows whose diagonal
    the mass dominates beside rows the stiffness dominates."""
    z = np.random.default_rng(seed).standard_normal(N ** 3)
    s = (z - z.min()) / (z.max() - z.min())
    return float(N) ** 2 * 10.0 ** (-3.0 + 3.0 * s)


def _rel(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


# ---- the solve with a reaction term on the host ------------------------------------------------------------------------------
class HostOperator:
    """A(kappa) + R(sigma) of the restated level, factorised once."""

    def __init__(self, N, kappa, sigma, faces):
        self.N, self.kappa, self.sigma, self.faces = N, kappa, sigma, faces
        self.free = free_mask(N, faces)
        A = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=faces, sigma=sigma).A.tocsc()
        A.eliminate_zeros()
        self.lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A")

    def solve(self, rhs):
        return self.lu.solve(np.asarray(rhs, dtype=np.float64).reshape(-1))

    def T(self, w, x, rows, cols):
        return poisson.diffusion_apply_dkappa(self.N, w, x, rows, cols, self.faces)

    def D(self, a, b, A, B):
        return poisson.diffusion_dkappa(self.N, a, b, A, B, self.faces)

    def Ts(self, w, x):
        return poisson.diffusion_apply_dsigma(self.N, w, x, self.faces)

    def Ds(self, a, b):
        return poisson.diffusion_dsigma(self.N, a, b, self.faces)


def host_adjoint(op, f, g, d):
    """J = 1/2 ||u - d||^2 over all nodes: (J, u, dJ/dkappa, dJ/dsigma, dJ/df, dJ/dg), as tests/diffusion_neumann_workers.py has
    it; R is diagonal on the free rows, so the lift and dJ/dg read no sigma, and dJ/dsigma = -D_sigma(lambda~, u)."""
    u = op.solve(lifted_rhs(op.N, op.kappa, f, g, op.faces))
    lam = op.solve(u - d)
    gk = -op.D(lam, u, "interior", "all")
    gs = -op.Ds(lam, u)
    gg = np.where(op.free, 0.0, (u - d) - op.T(op.kappa, lam, "all", "interior"))
    return 0.5 * float(np.sum((u - d) ** 2)), u, gk, gs, np.where(op.free, lam, 0.0), gg


def host_hessian_vector(op, f, g, d, vk, vs):
    """With q = dJ/dkappa . vk + dJ/dsigma . vs: (dq/dkappa, dq/dsigma) in four solves.  du is the derivative of u along
    (vk, vs), dlam that of lambda; the operator's derivative along the direction is T(vk, .) + T_sigma(vs, .)."""
    u = op.solve(lifted_rhs(op.N, op.kappa, f, g, op.faces))
    lam = op.solve(u - d)
    du = op.solve(-op.T(vk, u, "interior", "all") - op.Ts(vs, u))
    dlam = op.solve(du - op.T(vk, lam, "interior", "interior") - op.Ts(vs, lam))
    hk = -op.D(dlam, u, "interior", "all") - op.D(lam, du, "interior", "all")
    hs = -op.Ds(dlam, u) - op.Ds(lam, du)
    return hk, hs


def host_euler(N, kappa, dt, b, g, u0, d, steps, faces):
    """Implicit Euler, (A + R(1 / dt)) u^n = b + R(1 / dt) u^(n-1) - lift on the free rows and u^n = g on the Dirichlet nodes,
    one factorisation; J = 1/2 ||u^steps - d||^2 and its gradients with respect to kappa, u^0 and dt by the adjoint recursion
        lambda^n = (A + R)^-1 ubar^n,  ubar^steps = u^steps - d,  ubar^(n-1) = R(1 / dt) lambda~^n,
        dJ/dkappa = -sum_n D(lambda~^n, u^n; interior, all),
        dJ/dsigma = sum_n D_sigma(lambda~^n, u^(n-1)) - D_sigma(lambda~^n, u^n),   dJ/ddt = -(1 / dt^2) sum_c dJ/dsigma_c,
        dJ/du^0 = R(1 / dt) lambda~^1."""
    sigma = np.full(N ** 3, 1.0 / dt)
    op = HostOperator(N, kappa, sigma, faces)
    lift = poisson.diffusion_lift(N, kappa, g, faces)
    us = [np.asarray(u0, dtype=np.float64).reshape(-1)]
    for _ in range(steps):
        us.append(op.solve(np.where(op.free, b + op.Ts(sigma, us[-1]) - lift, g)))
    ubar = us[-1] - d
    gk, gs = np.zeros(N ** 3), np.zeros(N ** 3)
    for n in range(steps, 0, -1):
        lam = op.solve(ubar)
        gk -= op.D(lam, us[n], "interior", "all")
        gs += op.Ds(lam, us[n - 1]) - op.Ds(lam, us[n])
        ubar = op.Ts(sigma, lam)
    return us[-1], 0.5 * float(np.sum((us[-1] - d) ** 2)), gk, ubar, -float(np.sum(gs)) / dt ** 2


# Relative l2 distance between the DiffusionSolver results with a reaction term (mg_pcg at rtol 1e-12, V(2,2) Jacobi, N = 16, two
# levels) and the host references above (SuperLU).  The reference is the host adjoint; each limit is 8 x the largest figure
# measured once on an MI355X over the two face sets, both storages and (solver_worker) kappa and sigma on the device and on the
# CPU: the margin tests/diffusion_neumann_workers.py gives for the run-to-run variation of the solves' residuals.  A figure
# above 1e-10 would be a defect, not a limit (_check_limit).
# solver_worker, measured (stored and matrix-free, device and CPU fields alike to three digits; 16 to 18 iterations per solve),
# all six faces: u 1.002e-12, J 1.298e-13, grad_kappa 1.261e-12, grad_sigma 8.772e-13, grad_f 3.236e-13, grad_g 5.672e-13, the
# blocks H_kk v 1.366e-12, H_sk v 2.657e-12, H_ks v 1.467e-12, H_ss v 1.168e-12; faces x- | x+: u 2.829e-13, J 8.222e-14,
# grad_kappa 2.660e-13, grad_sigma 2.930e-13, grad_f 1.823e-13, grad_g 2.323e-13, the blocks 2.876e-13, 8.724e-13, 2.951e-13,
# 4.804e-13.  8 x the largest:
REACTION_LIMIT = 8 * 2.657e-12
# euler_worker, measured (14 to 15 iterations per solve), all six faces: u^3 6.716e-13, J 6.531e-14, grad_kappa 6.962e-13,
# grad_u0 6.859e-13, grad_dt 6.821e-14; faces x- | x+: 2.710e-13, 9.452e-15, 1.605e-13, 4.753e-13, 8.566e-15.  8 x the largest:
EULER_LIMIT = 8 * 6.962e-13

SOLVER_FACES = (None, ("x-", "x+"))


def _case():
    from tests.diffusion_workers import lognormal_kappa
    N = 16
    rng = np.random.default_rng(37)
    kappa = lognormal_kappa(N, 3, seed=4)
    n = (N + 1) ** 3
    f, d, g = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    return N, kappa, reaction_sigma(N), f, d, g, rng.standard_normal(N ** 3), N ** 2 * rng.standard_normal(N ** 3)


def _check_limit(worst, limit):
    print("largest discrepancy %.3e" % worst, flush=True)
    assert limit <= 1e-10, "a discrepancy above 1e-10 is a defect, not a limit"
    assert worst <= limit, (worst, limit)


def solver_worker():
    """u, J, the gradients with respect to kappa, sigma, f and g and the kappa-, sigma- and mixed blocks of Hessian-vector
    products against the host, for both face sets and both storages, sigma and kappa on the device; n_solves is 2 after the
    gradient, 4 after the first product and 6 after the second; the gradient of g is zero off the Dirichlet nodes.  Then kappa
    and sigma on the CPU: the same results, last_generate == "host"."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, sigma, f, d, g, vk, vs = _case()
    dev = lambda x: torch.tensor(x, device="cuda")
    zero = np.zeros(N ** 3)
    worst = 0.0
    for names in SOLVER_FACES:
        faces = poisson.face_set(names)
        op = HostOperator(N, kappa, sigma, faces)
        free = op.free
        J, u, gk, gs, gf, gg = host_adjoint(op, f, g, d)
        hkk, hsk = host_hessian_vector(op, f, g, d, vk, zero)
        hks, hss = host_hessian_vector(op, f, g, d, zero, vs)
        for name, min_rows in (("stored", None), ("matrix_free", 0)):
            for where in ("cuda", "cpu"):
                with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows, dirichlet_faces=names) as solver:
                    k = torch.tensor(kappa, device=where, requires_grad=True)
                    s = torch.tensor(sigma, device=where, requires_grad=True)
                    ft, gt = dev(f).requires_grad_(), dev(g).requires_grad_()
                    ut = solver.solve(k, ft, gt, sigma=s)
                    assert solver.last_generate == ("device" if where == "cuda" else "host"), solver.last_generate
                    assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
                    assert solver.hierarchy.level_reaction(1) and solver.hierarchy.level_reaction(0)
                    assert solver.hierarchy.diffusion_reaction() == (1, N)
                    Jt = 0.5 * torch.sum((ut - dev(d)) ** 2)
                    gkt, gst, gft, ggt = torch.autograd.grad(Jt, (k, s, ft, gt), create_graph=True)
                    assert solver.n_solves == 2, solver.n_solves
                    pkk, psk = torch.autograd.grad(torch.sum(gkt * torch.tensor(vk, device=where)), (k, s), retain_graph=True)
                    assert solver.n_solves == 4, solver.n_solves
                    pks, pss = torch.autograd.grad(torch.sum(gst * torch.tensor(vs, device=where)), (k, s))
                    assert solver.n_solves == 6, solver.n_solves
                    assert solver.n_generations == 1
                    host = lambda t: t.detach().cpu().numpy()
                    assert not host(ggt)[free].any() and not host(gft)[~free].any()
                    figures = (_rel(host(ut), u), abs(float(Jt.detach()) - J) / J, _rel(host(gkt), gk), _rel(host(gst), gs),
                               _rel(host(gft), gf), _rel(host(ggt), gg), _rel(host(pkk), hkk), _rel(host(psk), hsk),
                               _rel(host(pks), hks), _rel(host(pss), hss))
                    print(names, name, where, "iterations", solver.last_iterations, "rel l2: u %.3e  J %.3e  grad_kappa %.3e  "
                          "grad_sigma %.3e  grad_f %.3e  grad_g %.3e  H_kk v %.3e  H_sk v %.3e  H_ks v %.3e  H_ss v %.3e" % figures,
                          flush=True)
                    worst = max(worst, max(figures))
    _check_limit(worst, REACTION_LIMIT)
    print("solver ok")


def switch_worker():
    """Solves with sigma, then without, then with again on one solver with a device kappa: each change of state generates
    ("device") instead of refreshing, a repeated state refreshes, same_operator reuses the operator, and a solve without sigma
    on a solver that has seen one gives the bits of a solver that never has."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, sigma, f, d, g, vk, vs = _case()
    dev = lambda x: torch.tensor(x, device="cuda")
    with DiffusionSolver(N, 2, rtol=1e-12) as plain, DiffusionSolver(N, 2, rtol=1e-12) as solver:
        try:
            solver.solve(dev(kappa), dev(f), same_operator=True)
            raise AssertionError("same_operator without an earlier solve was accepted")
        except ValueError as exc:
            assert "there has been none" in str(exc)
        want = plain.solve(dev(kappa), dev(f))
        seen = []
        for s in (sigma, 2.0 * sigma, None, None, sigma):
            u = solver.solve(dev(kappa), dev(f), sigma=None if s is None else dev(s))
            seen.append(solver.last_generate)
            assert solver.hierarchy.level_reaction(1) == (s is not None)
            if s is None:
                assert torch.equal(u, want)
        assert seen == ["device", "refresh", "device", "refresh", "device"], seen
        assert solver.n_generations == 5
        again = solver.solve(dev(kappa), dev(f), sigma=dev(sigma), same_operator=True)
        assert solver.n_generations == 5 and torch.equal(again, u)
    print("switch ok")


def euler_worker():
    """Three implicit Euler steps by composition, sigma = 1 / dt broadcast from a scalar tensor: u^3 and the gradients of
    1/2 ||u^3 - d||^2 with respect to kappa, u^0 and dt against the host march; one generation and six solves in all."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, _, b, d, g, _, _ = _case()
    steps, dt = 3, 2.5e-3
    u0 = np.random.default_rng(41).standard_normal((N + 1) ** 3)
    dev = lambda x: torch.tensor(x, device="cuda")
    worst = 0.0
    for names in SOLVER_FACES:
        faces = poisson.face_set(names)
        u3, J, gk, gu0, gdt = host_euler(N, kappa, dt, b, g, u0, d, steps, faces)
        free = free_mask(N, faces)
        for name, min_rows in (("stored", None), ("matrix_free", 0)):
            with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows, dirichlet_faces=names) as solver:
                k = dev(kappa).requires_grad_()
                dtt = torch.tensor(dt, device="cuda", dtype=torch.float64, requires_grad=True)
                ut = dev(u0).requires_grad_()
                u_start, bt, gt = ut, dev(b), dev(g)
                for n in range(steps):
                    s = (1.0 / dtt).expand(N ** 3)
                    ut = solver.solve(k, bt + solver.reaction_apply(s, ut), gt, sigma=s, same_operator=(n > 0))
                Jt = 0.5 * torch.sum((ut - dev(d)) ** 2)
                gkt, gut, gdtt = torch.autograd.grad(Jt, (k, u_start, dtt))
                assert solver.n_generations == 1, solver.n_generations
                assert solver.n_solves == 2 * steps, solver.n_solves
                host = lambda t: t.detach().cpu().numpy()
                assert not host(gut)[~free].any()
                figures = (_rel(host(ut), u3), abs(float(Jt.detach()) - J) / J, _rel(host(gkt), gk), _rel(host(gut), gu0),
                           abs(float(gdtt) - gdt) / abs(gdt))
                print(names, name, "iterations", solver.last_iterations, "rel: u^3 %.3e  J %.3e  grad_kappa %.3e  grad_u0 %.3e  "
                      "grad_dt %.3e" % figures, flush=True)
                worst = max(worst, max(figures))
    _check_limit(worst, EULER_LIMIT)
    print("euler ok")
