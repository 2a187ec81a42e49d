"""Host references and DiffusionSolver test bodies of tests/test_diffusion_neumann.py: masks and the solve, the adjoint and the
four-solve Hessian-vector product of -div(kappa grad u) = f with a face set (Dirichlet data on some faces of the cube, no-flux
conditions with a genuine load on the free nodes of the others), built on scipy's spsolve and the restatements of poisson.py.
The torch bodies run in a process of their own that imports torch before libmg_hip.so is loaded (one HIP runtime for both);
each prints its figures and ends with an "... ok" line."""
import os
import sys

import numpy as np
import scipy.sparse.linalg as spl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402

EPS = np.finfo(np.float64).eps
FACE_SETS = (1, 32, 12, 18, 63)        # x-; z+; y- and y+; x+ and z-; all six


def free_mask(N, faces):
    return ~poisson.dirichlet_mask(N, faces)


def _rel(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


# ---- the solve with a face set on the host ---------------------------------------------------------------------------------
def host_solve(N, kappa, rhs, faces):
    return spl.spsolve(poisson.diffusion_level(N, 3, kappa, dirichlet_faces=faces).A.tocsc(), rhs)


def lifted_rhs(N, kappa, f, g, faces):
    free = free_mask(N, faces)
    return np.where(free, np.asarray(f).reshape(-1) - poisson.diffusion_lift(N, kappa, g, faces), np.asarray(g).reshape(-1))


def host_solve_g(N, kappa, f, g, faces):
    """u with A_FF u_F = f_F - A_FD g_D on the free nodes (f there is the load, flux data included) and u = g on the Dirichlet
    nodes."""
    return host_solve(N, kappa, lifted_rhs(N, kappa, f, g, faces), faces)


def host_adjoint_g(N, kappa, f, g, d, faces):
    """J = 1/2 ||u - d||^2 over all nodes: (J, u, dJ/dkappa, dJ/df, dJ/dg).  With lambda~ the adjoint solution with its entries
    on the Dirichlet nodes taken as 0: dJ/dkappa = -D(lambda~, u; free, all), dJ/df = lambda~ and
    dJ/dg = (u - d)_D - (A^(kappa) lambda~)_D."""
    free = free_mask(N, faces)
    u = host_solve_g(N, kappa, f, g, faces)
    lam = host_solve(N, kappa, u - d, faces)
    gk = -poisson.diffusion_dkappa(N, lam, u, "interior", "all", faces)
    gg = np.where(free, 0.0, (u - d) - poisson.diffusion_apply_dkappa(N, kappa, lam, "all", "interior", faces))
    return 0.5 * float(np.sum((u - d) ** 2)), u, gk, np.where(free, lam, 0.0), gg


def host_hessian_vector_g(N, kappa, f, g, d, v, faces):
    """With q = dJ/dkappa . v: (dq/dkappa, dq/df, dq/dg) in four solves, as tests/diffusion_dirichlet_workers.py has it with
    "interior" = the free nodes and "boundary" = the Dirichlet nodes."""
    free = free_mask(N, faces)
    T = lambda w, x, rows, cols: poisson.diffusion_apply_dkappa(N, w, x, rows, cols, faces)
    D = lambda a, b, A, B: poisson.diffusion_dkappa(N, a, b, A, B, faces)
    u = host_solve_g(N, kappa, f, g, faces)
    lam = host_solve(N, kappa, u - d, faces)
    du = host_solve(N, kappa, -T(v, u, "interior", "all"), faces)
    dlam = host_solve(N, kappa, du - T(v, lam, "interior", "interior"), faces)
    hk = -D(dlam, u, "interior", "all") - D(lam, du, "interior", "all")
    hg = -T(v, lam, "all", "interior") - T(kappa, dlam, "all", "interior")
    return hk, np.where(free, dlam, 0.0), np.where(free, 0.0, hg)


# Relative l2 distance between the DiffusionSolver results with a face set (mg_pcg at rtol 1e-12, V(2,2) Jacobi, N = 16, two
# levels) and the host references above (spsolve).  The reference is the host adjoint; the limit is 8 x the largest figure
# measured once on an MI355X over the two face sets and both storages: the margin for the solves' residuals, which vary from
# run to run with the summation order of mg_pcg's partial sums.
# Measured (stored and matrix-free alike to three digits; 18 to 20 iterations per solve), faces x- | x+: u 3.138e-13, J 4.082e-15,
# grad_kappa 4.069e-13, grad_f 1.689e-13, grad_g 1.863e-13, the kappa, f and g blocks of the Hessian-vector product 1.695e-13,
# 3.838e-13, 4.064e-13; face z+: u 2.920e-13, J 5.464e-14, grad_kappa 3.793e-13, grad_f 4.472e-14, grad_g 8.410e-14, the blocks
# 9.214e-14, 3.521e-13, 4.064e-13.  8 x the largest:
NEUMANN_LIMIT = 8 * 4.069e-13

SOLVER_FACES = (("x-", "x+"), ("z+",))


def _case():
    from tests.diffusion_workers import lognormal_kappa
    N = 16
    rng = np.random.default_rng(31)
    kappa = lognormal_kappa(N, 3, seed=4)
    n = (N + 1) ** 3
    f, d, g = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    return N, kappa, f, d, g, rng.standard_normal(N ** 3)


def _solvers(N, faces):
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows, dirichlet_faces=faces) as solver:
            yield name, solver
            assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
            assert solver.hierarchy.diffusion_faces() == poisson.face_set(faces)


def solver_worker():
    """u, the gradients with respect to kappa, f and g and a Hessian-vector product against the host, for both face sets and
    both storages; n_solves is 2 after the gradient and 4 after the product; the gradient of g is zero off the Dirichlet nodes."""
    import torch
    N, kappa, f, d, g, v = _case()
    dev = lambda x: torch.tensor(x, device="cuda")
    worst = 0.0
    for names in SOLVER_FACES:
        faces = poisson.face_set(names)
        free = free_mask(N, faces)
        J, u, gk, gf, gg = host_adjoint_g(N, kappa, f, g, d, faces)
        hk, hf, hg = host_hessian_vector_g(N, kappa, f, g, d, v, faces)
        for name, solver in _solvers(N, names):
            k = torch.tensor(kappa, requires_grad=True)
            ft, gt = dev(f).requires_grad_(), dev(g).requires_grad_()
            ut = solver.solve(k, ft, gt)
            Jt = 0.5 * torch.sum((ut - dev(d)) ** 2)
            gkt, gft, ggt = torch.autograd.grad(Jt, (k, ft, gt), create_graph=True)
            assert solver.n_solves == 2, solver.n_solves
            pk, pf, pg = torch.autograd.grad(torch.sum(gkt * torch.tensor(v)), (k, ft, gt))
            assert solver.n_solves == 4, solver.n_solves
            assert solver._generation == 1
            ggn = ggt.detach().cpu().numpy()
            assert not ggn[free].any() and not pg.cpu().numpy()[free].any()
            assert not gft.detach().cpu().numpy()[~free].any()
            assert np.array_equal(solver._boundary_mask().cpu().numpy(), ~free)
            figures = (_rel(ut.detach().cpu().numpy(), u), abs(float(Jt.detach()) - J) / J, _rel(gkt.detach().numpy(), gk),
                       _rel(gft.detach().cpu().numpy(), gf), _rel(ggn, gg), _rel(pk.numpy(), hk), _rel(pf.cpu().numpy(), hf),
                       _rel(pg.cpu().numpy(), hg))
            print(names, name, "iterations", solver.last_iterations, "rel l2: u %.3e  J %.3e  grad_kappa %.3e  grad_f %.3e  "
                  "grad_g %.3e  H_kk v %.3e  H_fk v %.3e  H_gk v %.3e" % figures, flush=True)
            worst = max(worst, max(figures))
    print("largest discrepancy %.3e" % worst, flush=True)
    assert worst <= NEUMANN_LIMIT, (worst, NEUMANN_LIMIT)
    print("solver ok")
