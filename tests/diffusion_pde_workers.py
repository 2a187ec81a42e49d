"""Cases, host solves and DiffusionSolver test bodies of tests/test_diffusion_pde.py: the diffusion solves against closed-form
solutions of -div(kappa grad u) + sigma u = f.  The exact fields and the loads come from tests/pde_reference.py, which shares no
arithmetic with the package; the host solves here put them through the restatements of poisson.py and scipy's sparse direct
solve.  The torch bodies run in a process of their own that imports torch before libmg_hip.so is loaded (one HIP runtime for
both); each prints its figures and ends with an "... ok" line."""
import functools
import os
import sys

import numpy as np
import scipy.sparse.linalg as spl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests import pde_reference as ref  # noqa: E402

EPS = np.finfo(np.float64).eps
KAPPA0 = 1.7                            # the constant kappa of the patch test, the sine modes and the heat march
MODES = ((2, 1, 3), (1, 1, 1))
LEVELS = {8: 3, 16: 3, 32: 4}           # levels of the DiffusionSolver per N
STORAGES = (("stored", None), ("matrix_free", 0))
N_POINTS = 500

# Observed orders p = log2(e_N / e_2N) of root-mean-square errors.  P1 on a quasi-uniform mesh with these loads is second order
# in the nodal values, in the cell-averaged flux at the cell centres (a superconvergence point of the mean gradient) and in the
# interpolant at arbitrary points, and first order in the simplex gradient at arbitrary points.  The thresholds are the theory's
# 2 less the pre-asymptotic shortfall at N = 8 (the host restatements measured 1.85 at the least), and 1 within 0.1 below and 0.2
# above.
SECOND_ORDER_AT_LEAST = 1.8
FIRST_ORDER_BETWEEN = (0.9, 1.2)


def patch_problem(which, N=6):
    """The three face sets of the patch test with the affine field: (1) Dirichlet on x- only, flux data on x+, y+ and z-, Robin
    on z+ with a random alpha per face-cell in [0.5, 1.5] and on y- with a constant one; (2) Dirichlet on x- and x+, flux data
    on y+ and z-, the same Robin faces; (3) all six faces Dirichlet, sigma only."""
    field = ref.Affine(kappa=KAPPA0, sigma=0.8)
    robin = {"z+": 0.5 + np.random.default_rng(11).random(N * N), "y-": np.full(N * N, 0.9)}
    if which == 1:
        return ref.Problem(field, N, ("x-",), ("x+", "y+", "z-"), robin)
    if which == 2:
        return ref.Problem(field, N, ("x-", "x+"), ("y+", "z-"), robin)
    return ref.Problem(field, N, ref.FACES)


def order_problem(config, N):
    """(a) all faces Dirichlet, with sigma; (b) Dirichlet on x- and x+, flux data on y-, y+ and z-, Robin alpha = 1.5 on z+, with
    sigma.  The smooth field of tests/pde_reference.py."""
    field = ref.Smooth(reaction=True)
    if config == "a":
        return ref.Problem(field, N, ref.FACES)
    return ref.Problem(field, N, ("x-", "x+"), ("y-", "y+", "z-"), {"z+": np.full(N * N, 1.5)})


def points():
    return np.random.default_rng(2024).random((N_POINTS, 3))


def host_system(p):
    """(A, rhs) of the restated level for a `pde_reference.Problem`: `diffusion_level`'s matrix, the problem's load plus the
    ambient load of its Robin faces on the free rows less the lift of g, and g on the Dirichlet rows."""
    faces = list(p.dirichlet)
    sigma = p.sigma if np.any(p.sigma) else None
    A = poisson.diffusion_level(p.N, 3, p.kappa, dirichlet_faces=faces, sigma=sigma, robin=p.robin or None).A.tocsc()
    A.eliminate_zeros()
    load = p.load.copy()
    for face, alpha in p.robin.items():
        load = load + poisson.diffusion_apply_drobin(p.N, face, alpha, p.u_ext[face], faces)
    rhs = np.where(p.is_dirichlet, p.g, load - poisson.diffusion_lift(p.N, p.kappa, p.g, faces))
    assert np.array_equal(p.is_dirichlet, poisson.dirichlet_mask(p.N, faces))
    return A, rhs


def host_solve(p):
    A, rhs = host_system(p)
    return spl.splu(A, permc_spec="MMD_AT_PLUS_A").solve(rhs)


@functools.lru_cache(maxsize=None)
def host_order_solution(config, N):
    return host_solve(order_problem(config, N))


def rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def errors(p, pts, nodal, flux, sampled, sampled_gradient):
    """Root-mean-square errors of the four quantities against the exact field of the problem: the nodal values over all nodes,
    the cell flux against -kappa grad u at the cell centres, the interpolant and its gradient at the points."""
    fld = p.field
    cx = ref.cell_centres(p.N)
    q = np.stack([-fld.kappa(*cx) * g for g in fld.grad(*cx)]).reshape(-1)
    px = (pts[:, 0], pts[:, 1], pts[:, 2])
    return {"nodal": rms(nodal - p.exact), "cell flux": rms(np.asarray(flux).reshape(-1) - q),
            "point sample": rms(sampled - fld.u(*px)),
            "point gradient": rms(np.asarray(sampled_gradient) - np.stack(fld.grad(*px), axis=1))}


def host_errors(config, N):
    p, u = order_problem(config, N), host_order_solution(config, N)
    pts = points()
    return errors(p, pts, u, -poisson.diffusion_cell_gradient(N, p.kappa, u), poisson.diffusion_point_sample(N, pts, u),
                  poisson.diffusion_point_gradient(N, pts, u))


def check_orders(label, by_N):
    """`by_N`: {N: errors}.  Prints the table row by row and asserts the orders between consecutive N."""
    Ns = sorted(by_N)
    for quantity in ("nodal", "cell flux", "point sample", "point gradient"):
        e = [by_N[N][quantity] for N in Ns]
        orders = [float(np.log2(e[i] / e[i + 1])) for i in range(len(e) - 1)]
        print("%-12s %-15s rms " % (label, quantity) + "  ".join("N=%d %.3e" % (N, x) for N, x in zip(Ns, e)) +
              "   ratios " + ", ".join("%.2f" % (e[i] / e[i + 1]) for i in range(len(e) - 1)) +
              "   orders " + ", ".join("%.3f" % o for o in orders), flush=True)
        for o in orders:
            if quantity == "point gradient":
                assert FIRST_ORDER_BETWEEN[0] <= o <= FIRST_ORDER_BETWEEN[1], (label, quantity, orders)
            else:
                assert o >= SECOND_ORDER_AT_LEAST, (label, quantity, orders)


def extreme_eigenvalues(A):
    """(smallest, largest) eigenvalue of the symmetric level matrix (identity rows included)."""
    A = A.tocsc()
    lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A")
    lo = spl.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False, OPinv=spl.LinearOperator(A.shape, matvec=lu.solve))[0]
    hi = spl.eigsh(A, k=1, which="LA", return_eigenvectors=False)[0]
    return float(lo), float(hi)


def solve_error_bound(A, rhs, residual, u):
    """What the stopping rule of `mg_pcg` allows for ||u_h - A^-1 rhs||_2 (so for every entry): the solve stops at a recursion
    residual r with ||r|| = `residual` ||rhs|| (`last_residual`), and A e = r gives ||e|| <= ||r|| / lambda_min(A).  The recursion
    residual follows the true one to rounding, cond(A) eps ||u|| in the solution, which is also what the direct solve this is
    compared with carries (tests/test_diffusion_robin.py bounds its linear solution the same way).  None: no iteration ran."""
    lo, hi = extreme_eigenvalues(A)
    return (residual or 0.0) * float(np.linalg.norm(rhs)) / lo + (hi / lo) * EPS * float(np.linalg.norm(u)), hi / lo


# ---- torch bodies ------------------------------------------------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device="cuda")


def _host(t):
    return t.detach().cpu().numpy()


def _device_solve(solver, p, many_with=None):
    """The problem through `DiffusionSolver.solve`: Dirichlet data in g, the loads in f, sigma and the Robin fields as inputs,
    the ambient load by `robin_apply`.  With `many_with` (another load vector) also through `solve_many` with the two loads as
    lanes, whose bytes must be those of `solve`."""
    import torch
    kappa, g = _dev(p.kappa), _dev(p.g)
    sigma = _dev(p.sigma) if np.any(p.sigma) else None
    robin = {face: _dev(alpha) for face, alpha in p.robin.items()} or None
    f = _dev(p.load)
    for face in p.robin:
        f = f + solver.robin_apply(face, robin[face], _dev(p.u_ext[face]))
    u = solver.solve(kappa, f, g, sigma=sigma, robin=robin)
    if many_with is not None:
        other = _dev(many_with)
        second = solver.solve(kappa, other, g, sigma=sigma, robin=robin)
        U = solver.solve_many(kappa, torch.stack([f, other]), g, sigma=sigma, robin=robin)
        assert torch.equal(U[0], u) and torch.equal(U[1], second), "solve_many does not give the bytes of solve"
        u = solver.solve(kappa, f, g, sigma=sigma, robin=robin)
    return kappa, u


def patch_worker():
    """The affine field through `solve`, `flux`, `sample` and `sample_gradient` at N = 8, three face sets, both storages."""
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 8
    pts = points()
    for which in (1, 2, 3):
        p = patch_problem(which, N)
        A, rhs = host_system(p)
        slope = np.array(p.field.slope)
        for name, min_rows in STORAGES:
            with DiffusionSolver(N, LEVELS[N], rtol=1e-12, matrix_free_min_rows=min_rows, dirichlet_faces=list(p.dirichlet)) as solver:
                kappa, u = _device_solve(solver, p)
                assert solver.hierarchy.level_matrix_free(solver.top) == (name == "matrix_free")
                bound, cond = solve_error_bound(A, rhs, solver.last_residual["forward"], p.exact)
                err = float(np.abs(_host(u) - p.exact).max())
                # The three derived quantities are linear in u_h and exact on the affine field, so their errors are those of
                # e = u_h - u: a cell gradient is a mean of differences of two nodal values over h, |.| <= 2 N max|e|, times kappa
                # for the flux; the interpolant is a convex combination of nodal values, <= max|e|; the simplex gradient is one
                # difference over h, <= 2 N max|e|.  Their own rounding is a few eps of N |u| <= 3 N (|u| < 2.5 on the cube); 16
                # covers the four differences, the scale and the product of the cell gradient.
                rounding = 16 * EPS * 3.0 * N
                q = _host(solver.flux(kappa, u)).reshape(3, -1)
                eq = float(np.abs(q + KAPPA0 * slope[:, None]).max())
                X = _dev(pts)
                es = float(np.abs(_host(solver.sample(u, X)) - p.field.u(pts[:, 0], pts[:, 1], pts[:, 2])).max())
                eg = float(np.abs(_host(solver.sample_gradient(u, X)) - slope[None, :]).max())
                print("patch %d %-11s iterations %s residual %.3e cond %.3e  max error: u %.3e (bound %.3e)  flux %.3e  sample %.3e  "
                      "gradient %.3e" % (which, name, solver.last_iterations["forward"], solver.last_residual["forward"] or 0.0, cond,
                                         err, bound, eq, es, eg), flush=True)
                assert err <= bound, (which, name, err, bound)
                assert eq <= KAPPA0 * (2 * N * bound + rounding), (which, name, eq)
                assert es <= bound + rounding, (which, name, es)
                assert eg <= 2 * N * bound + rounding, (which, name, eg)
    print("patch ok")


def orders_worker(config):
    """The smooth field through `solve`, `flux`, `sample` and `sample_gradient` at N = 8, 16, 32, both storages: the orders
    of the host test, the host's sparse direct solution within the limit of tests/test_diffusion_robin.py, `solve_many` = `solve`."""
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    from tests.diffusion_robin_workers import ROBIN_LIMIT
    pts = points()
    other = {"a": "b", "b": "a"}[config]
    for name, min_rows in STORAGES:
        by_N = {}
        for N in sorted(LEVELS):
            p = order_problem(config, N)
            with DiffusionSolver(N, LEVELS[N], rtol=1e-12, matrix_free_min_rows=min_rows, dirichlet_faces=list(p.dirichlet)) as solver:
                kappa, u = _device_solve(solver, p, many_with=order_problem(other, N).load)
                assert solver.hierarchy.level_matrix_free(solver.top) == (name == "matrix_free")
                X = _dev(pts)
                by_N[N] = errors(p, pts, _host(u), _host(solver.flux(kappa, u)), _host(solver.sample(u, X)),
                                 _host(solver.sample_gradient(u, X)))
                want = host_order_solution(config, N)
                rel = float(np.linalg.norm(_host(u) - want) / np.linalg.norm(want))
                print("orders %s %-11s N %2d iterations %s  rel l2 against the direct solve %.3e (limit %.3e)"
                      % (config, name, N, solver.last_iterations["forward"], rel, ROBIN_LIMIT), flush=True)
                assert rel <= ROBIN_LIMIT, (config, name, N, rel)
        check_orders("device " + config + " " + name, by_N)
    print("orders ok")


def heat_worker():
    """Five implicit Euler steps of a sine mode, sigma = 1 / dt, on one generation."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, dt, steps = 16, 1e-3, 5
    h = 1.0 / N
    mode = MODES[0]
    v = ref.sine_mode(N, mode)
    lam = ref.sine_eigenvalue(N, mode, KAPPA0)
    for name, min_rows in STORAGES:
        with DiffusionSolver(N, LEVELS[N], rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            kappa = torch.full((N ** 3,), KAPPA0, dtype=torch.float64, device="cuda")
            sigma = torch.full((N ** 3,), 1.0 / dt, dtype=torch.float64, device="cuda")
            u = _dev(v)
            # Per step the solve leaves e_m with (R + A) e_m = r_m, ||r_m|| = last_residual ||rhs_m||, and on the free rows
            # lambda_min(R + A) >= h^3 / dt (R = h^3 / dt there: 24 simplices at every free node, A is positive), so
            # ||e_m|| <= last_residual ||rhs_m|| dt / h^3.  Later steps multiply an error by (R + A)^-1 R, of norm < 1, so the errors
            # add at most.  Rounding: cond(R + A) eps ||u|| per step with cond <= 1 + dt lambda_max(A) / h^3 <= 1 + 12 kappa dt / h^2
            # (Gershgorin: a row of A sums 12 kappa h in absolute value).
            cond = 1.0 + 12.0 * KAPPA0 * dt / h ** 2
            allowed = 0.0
            for m in range(1, steps + 1):
                rhs = solver.reaction_apply(sigma, u)
                u = solver.solve(kappa, rhs, sigma=sigma, same_operator=m > 1)
                allowed += (solver.last_residual["forward"] or 0.0) * float(torch.linalg.vector_norm(rhs)) * dt / h ** 3
                allowed += cond * EPS * float(torch.linalg.vector_norm(u))
                want = v * (1.0 + dt * lam) ** -m
                err = float(np.linalg.norm(_host(u) - want))
                print("heat %-11s step %d factor %.6f  l2 error %.3e (allowed %.3e)" % (name, m, (1.0 + dt * lam) ** -m, err, allowed),
                      flush=True)
                assert err <= allowed, (name, m, err, allowed)
            assert solver.hierarchy.level_matrix_free(solver.top) == (name == "matrix_free")
            assert solver.n_generations == 1, solver.n_generations
    print("heat ok")


def derivative_worker():
    """dJ/dkappa of J = 1/2 ||u||^2 for a uniform kappa, f a sine mode."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 16
    h = 1.0 / N
    mode = MODES[0]
    v = ref.sine_mode(N, mode)
    lam = ref.sine_eigenvalue(N, mode, KAPPA0)
    # A(kappa) is linear in kappa, so with kappa uniform sum_c dA/dkappa_c = A / kappa, and the adjoint formula
    # dJ/dkappa_c = -lambda^T (dA/dkappa_c) u with A lambda = u sums to -u^T u / kappa; u = f / (lambda_h h^3).
    want = -float(v @ v) / (lam * h ** 3) ** 2 / KAPPA0
    # lambda_min = lambda_h(1,1,1) h^3 and lambda_max <= max(1, 12 kappa h) (identity rows; Gershgorin) bound cond(A) from the
    # closed form.  The forward solve is within cond rtol of u in relative l2; the adjoint solve inherits that through A^-1
    # (another factor cond at most) and adds its own cond rtol; the sum over D(lambda, u) is bilinear, so the relative error is at
    # most the sum of the two, (cond^2 + 2 cond) rtol, rtol being the larger last_residual, plus the same with eps for rounding.
    cond = max(1.0, 12.0 * KAPPA0 * h) / (ref.sine_eigenvalue(N, (1, 1, 1), KAPPA0) * h ** 3)
    for name, min_rows in STORAGES:
        with DiffusionSolver(N, LEVELS[N], rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            kappa = torch.full((N ** 3,), KAPPA0, dtype=torch.float64, device="cuda", requires_grad=True)
            u = solver.solve(kappa, _dev(v))
            J = 0.5 * torch.sum(u * u)
            (gk,) = torch.autograd.grad(J, [kappa])
            assert solver.n_solves == 2 and solver.n_generations == 1
            got = float(gk.sum())
            rho = max(solver.last_residual["forward"] or 0.0, solver.last_residual["adjoint"] or 0.0)
            allowed = (cond ** 2 + 2 * cond) * (rho + EPS)
            print("derivative %-11s sum grad_kappa %.12e closed form %.12e  relative %.3e (allowed %.3e, cond %.1f)"
                  % (name, got, want, abs(got - want) / abs(want), allowed, cond), flush=True)
            assert abs(got - want) <= allowed * abs(want), (name, got, want)
    print("derivative ok")
