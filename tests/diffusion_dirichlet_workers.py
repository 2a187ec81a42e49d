"""Host references and DiffusionSolver test bodies of tests/test_diffusion_dirichlet.py: the per-row terms and bound of
T(w, x; rows, cols) = M_rows A^(w) M_cols x on boundary rows and columns as well, the solve with Dirichlet data g through the
lifted system and scipy's spsolve, its adjoint gradients with respect to kappa, f and g, its tangent and its four-solve
Hessian-vector product.  The torch bodies run in a process of their own that imports torch before libmg_hip.so is loaded (one
HIP runtime for both); each prints its figures and ends with an "... ok" line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests.diffusion_adjoint_workers import _gradient_case, _rel, host_solve  # noqa: E402

EPS = np.finfo(np.float64).eps
PAIRS = [(r, c) for r in ("interior", "all") for c in ("interior", "all")]
_EDGES = ((2, 0), (1, 0), (0, 0), (0, 1), (1, 1), (2, 1))       # (axis, side) of z-, y-, x-, x+, y+, z+


def inner_mask(N):
    m = np.zeros((N + 1,) * 3, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m.reshape(-1)


def mask_of(N, nodes):
    """M_nodes as a vector of 0 / 1."""
    return inner_mask(N).astype(np.float64) if nodes == "interior" else np.ones((N + 1) ** 3)


def boundary_part(N, g):
    return np.where(inner_mask(N), 0.0, np.asarray(g, dtype=np.float64).reshape(-1))


def natural_row_terms(N, w, x, rows="interior", cols="interior"):
    """The seven products a row of M_rows A^(w) M_cols x sums: the diagonal's and the six neighbours' (z-, y-, x-, x+, y+, z+),
    [7, nodes], a cell and a neighbour outside the grid counting as 0; 0 on the rows that `rows` masks."""
    n1 = N + 1
    h = 1.0 / N
    se, t = poisson._edge_sums_3d(np.pad(np.asarray(w, dtype=np.float64).reshape(N, N, N), 1, constant_values=0.0), n1)
    xm = np.asarray(x, dtype=np.float64).reshape(-1) * mask_of(N, cols)
    idx = np.arange(n1 ** 3, dtype=np.int64)
    ijk = [idx % n1, (idx // n1) % n1, idx // (n1 * n1)]
    strides = (1, n1, n1 * n1)
    xp = np.concatenate([np.zeros(strides[2]), xm, np.zeros(strides[2])])
    terms = [((t / 6.0) * h) * xm]
    for axis, side in _EDGES:
        delta = strides[axis] if side else -strides[axis]
        outside = ijk[axis] + 1 > N if side else ijk[axis] - 1 < 0
        xj = np.where(outside, 0.0, xp[strides[2] + delta:strides[2] + delta + xm.size])
        terms.append(-((se[axis][side] / 6.0) * h) * xj)
    return np.array(terms) * mask_of(N, rows)


def natural_row_bound(N, w, x, rows="interior", cols="interior"):
    """diffusion_tangent_workers.row_bound on every row that `rows` keeps: 16 eps (h / 6) sum over the row's (up to) six edges
    e = (i, j) of (sum_c n_c |w_c|) (|x~_i| + |x~_j|), x~ = M_cols x, over the cells of the grid that hold the edge."""
    absw, absx = np.abs(np.asarray(w, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64))
    terms = np.abs(natural_row_terms(N, absw, absx, rows, cols))
    # the diagonal's product is (sum of the six edge sums) |x~_i|: with the six neighbours' that is sum_e se_e (|x~_i| + |x~_j|)
    return 16 * EPS * terms.sum(axis=0)


# ---- the solve with Dirichlet data on the host ---------------------------------------------------------------------------------
def lifted_rhs(N, kappa, f, g):
    return np.where(inner_mask(N), np.asarray(f).reshape(-1) - poisson.diffusion_lift(N, kappa, g), np.asarray(g).reshape(-1))


def host_solve_g(N, kappa, f, g):
    """u with -div(kappa grad u) = f inside and u = g on the boundary: spsolve of the lifted system."""
    return host_solve(N, kappa, lifted_rhs(N, kappa, f, g))


def host_adjoint_g(N, kappa, f, g, d):
    """J = 1/2 ||u - d||^2 over all nodes: (J, u, dJ/dkappa, dJ/df, dJ/dg, lambda) through one adjoint solve.  With lambda~ the
    adjoint solution with its boundary entries taken as 0: dJ/dkappa = -D(lambda~, u; interior, all), dJ/df = lambda~ (the
    boundary entries of f do not count) and dJ/dg = (u - d)_B - (A^(kappa) lambda~)_B."""
    u = host_solve_g(N, kappa, f, g)
    lam = host_solve(N, kappa, u - d)
    inner = inner_mask(N)
    gk = -poisson.diffusion_dkappa(N, lam, u, "interior", "all")
    gg = np.where(inner, 0.0, (u - d) - poisson.diffusion_apply_dkappa(N, kappa, lam, "all", "interior"))
    return 0.5 * float(np.sum((u - d) ** 2)), u, gk, np.where(inner, lam, 0.0), gg, lam


def host_tangent_g(N, kappa, f, g, dkappa, df, dg):
    """(u, du) in the direction (dkappa, df, dg): A du = df - T(dkappa, u; interior, all) - T(kappa, dg_B; interior, all) inside,
    du = dg on the boundary."""
    u = host_solve_g(N, kappa, f, g)
    rhs = df - poisson.diffusion_apply_dkappa(N, dkappa, u, "interior", "all") - poisson.diffusion_lift(N, kappa, dg)
    return u, host_solve(N, kappa, np.where(inner_mask(N), rhs, dg))


def host_hessian_vector_g(N, kappa, f, g, d, v):
    """With q = dJ/dkappa . v: (dq/dkappa, dq/df, dq/dg) in four solves.  In the direction v of kappa, A du = -T(v, u; interior,
    all) (du = 0 on the boundary) and A dlambda = du - T(v, lambda~; interior, interior); then
    dq/dkappa = -D(dlambda~, u; interior, all) - D(lambda~, du; interior, all), dq/df = dlambda~ and, second derivatives being
    symmetric, dq/dg = the derivative of dJ/dg along v = -(A^(v) lambda~)_B - (A^(kappa) dlambda~)_B."""
    inner = inner_mask(N)
    u = host_solve_g(N, kappa, f, g)
    lam = host_solve(N, kappa, u - d)
    du = host_solve(N, kappa, -poisson.diffusion_apply_dkappa(N, v, u, "interior", "all"))
    dlam = host_solve(N, kappa, du - poisson.diffusion_apply_dkappa(N, v, lam))
    hk = -poisson.diffusion_dkappa(N, dlam, u, "interior", "all") - poisson.diffusion_dkappa(N, lam, du, "interior", "all")
    hg = -poisson.diffusion_apply_dkappa(N, v, lam, "all", "interior") - poisson.diffusion_apply_dkappa(N, kappa, dlam, "all", "interior")
    return hk, np.where(inner, dlam, 0.0), np.where(inner, 0.0, hg)


# Relative l2 distance between the device results with Dirichlet data (mg_pcg at rtol 1e-12, V(2,2) Jacobi, N = 16, two levels)
# and the host references above (spsolve).  The rule of SECOND_ORDER_LIMIT (tests/diffusion_tangent_workers.py): 100 x the
# largest figure measured once on an MI355X, the margin for PCG's stopping point moving by an iteration, and never looser
# than 1e-6.
# Measured (stored and matrix-free alike, kappa on the CPU and on the device alike; 16 to 18 iterations per solve): u 2.522e-13,
# J 2.788e-14, grad_kappa 3.440e-13, grad_f 5.604e-14, grad_g 1.067e-13; du of `tangent` 3.322e-13 (df = dg = None: 1.846e-12);
# the kappa, f and g blocks of the Hessian-vector product 4.481e-13, 5.522e-13, 3.264e-13.  100 x the largest:
DIRICHLET_LIMIT = 1.9e-10


def _dirichlet_case():
    N, kappa, f, d = _gradient_case()
    rng = np.random.default_rng(23)
    n, cells = (N + 1) ** 3, N ** 3
    g, dg, df = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    return N, kappa, f, d, g, rng.standard_normal(cells), df, dg, rng.standard_normal(cells)


def _solvers():
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = _dirichlet_case()[0]
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            yield name, solver
            assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")


def gradient_worker():
    """u against spsolve of the lifted system and the gradients of J with respect to kappa (a CPU and a device tensor), f and
    g against the host adjoint: one solve forward, one more for the backward pass, one generation."""
    import torch
    N, kappa, f, d, g, *_ = _dirichlet_case()
    J, u, gk, gf, gg, _ = host_adjoint_g(N, kappa, f, g, d)
    masked = -poisson.diffusion_dkappa(N, host_solve(N, kappa, u - d), u)
    print("the gradient without the lift would miss by %.3e" % _rel(masked, gk), flush=True)
    dt = torch.tensor(d, device="cuda")
    for name, solver in _solvers():
        for where in ("cpu", "cuda"):
            k = torch.tensor(kappa, device=where, requires_grad=True)
            ft = torch.tensor(f, device="cuda", requires_grad=True)
            gt = torch.tensor(g, device="cuda", requires_grad=True)
            before, generation = solver.n_solves, solver._generation
            ut = solver.solve(k, ft, gt)
            assert solver.n_solves == before + 1
            Jt = 0.5 * torch.sum((ut - dt) ** 2)
            Jt.backward()
            assert solver.n_solves == before + 2 and solver._generation == generation + 1, (solver.n_solves, solver._generation)
            assert solver.last_generate == ("host" if where == "cpu" else ("device" if generation == 0 else "refresh"))
            assert set(solver.last_iterations) == {"forward", "adjoint"}
            assert k.grad.shape == k.shape and k.grad.device == k.device and ft.grad.shape == ft.shape and gt.grad.shape == gt.shape
            un = ut.detach().cpu().numpy()
            assert not gt.grad.cpu().numpy()[inner_mask(N)].any() and not ft.grad.cpu().numpy()[~inner_mask(N)].any()
            figures = (_rel(un, u), abs(float(Jt) - J) / J, _rel(k.grad.cpu().numpy(), gk), _rel(ft.grad.cpu().numpy(), gf),
                       _rel(gt.grad.cpu().numpy(), gg))
            print(name, "kappa on", where, "iterations", solver.last_iterations,
                  "rel l2: u %.3e  J %.3e  grad_kappa %.3e  grad_f %.3e  grad_g %.3e" % figures, flush=True)
            assert max(figures) <= DIRICHLET_LIMIT, figures
    print("gradient ok")


def tangent_worker():
    import torch
    N, kappa, f, d, g, dkappa, df, dg, _ = _dirichlet_case()
    u, du = host_tangent_g(N, kappa, f, g, dkappa, df, dg)
    _, du0 = host_tangent_g(N, kappa, f, g, dkappa, np.zeros_like(df), np.zeros_like(dg))
    dev = lambda x: torch.tensor(x, device="cuda")
    for name, solver in _solvers():
        ut, dut = solver.tangent(torch.tensor(kappa), dev(f), dev(dkappa), dev(df), g=dev(g), dg=dev(dg))
        assert solver.n_solves == 2 and solver._generation == 1 and solver.last_generate == "host"
        assert set(solver.last_iterations) == {"forward", "tangent"}
        dun = dut.cpu().numpy()
        figures = [_rel(ut.cpu().numpy(), u), _rel(dun, du)]
        _, dut0 = solver.tangent(dev(kappa), dev(f), dev(dkappa), g=dev(g))         # df = None, dg = None: zero
        assert solver.n_solves == 4 and solver._generation == 2
        figures.append(_rel(dut0.cpu().numpy(), du0))
        print(name, "iterations", solver.last_iterations, "rel l2: u %.3e  du %.3e  du (df, dg = None) %.3e" % tuple(figures), flush=True)
        assert max(figures) <= DIRICHLET_LIMIT, figures
        try:
            solver.tangent(dev(kappa), dev(f), dev(dkappa), dg=dev(dg))
            raise AssertionError("dg without g was accepted")
        except ValueError:
            pass
    print("tangent ok")


def hessian_worker():
    import torch
    N, kappa, f, d, g, _, _, _, v = _dirichlet_case()
    hk, hf, hg = host_hessian_vector_g(N, kappa, f, g, d, v)
    dev = lambda x: torch.tensor(x, device="cuda")
    for name, solver in _solvers():
        k = torch.tensor(kappa, requires_grad=True)                 # on the CPU
        ft, gt = dev(f).requires_grad_(), dev(g).requires_grad_()
        J = 0.5 * torch.sum((solver.solve(k, ft, gt) - dev(d)) ** 2)
        (gk,) = torch.autograd.grad(J, k, create_graph=True)
        assert solver.n_solves == 2, solver.n_solves
        pk, pf, pg = torch.autograd.grad(torch.sum(gk * torch.tensor(v)), (k, ft, gt))
        assert solver.n_solves == 4, solver.n_solves
        assert solver._generation == 1 and solver.last_generate == "host", (solver._generation, solver.last_generate)
        assert pk.shape == k.shape and pk.device == k.device and pf.shape == ft.shape and pg.shape == gt.shape
        figures = (_rel(pk.numpy(), hk), _rel(pf.cpu().numpy(), hf), _rel(pg.cpu().numpy(), hg))
        print(name, "iterations", solver.last_iterations, "rel l2: H_kk v %.3e  H_fk v %.3e  H_gk v %.3e" % figures, flush=True)
        assert max(figures) <= DIRICHLET_LIMIT, figures
    print("hessian ok")


def without_g_worker():
    """g = None is the call without the keyword: the same bytes and the same counters, for solve, backward and tangent."""
    import torch
    N, kappa, f, d, _, dkappa, df, _, _ = _dirichlet_case()
    dev = lambda x: torch.tensor(x, device="cuda")

    def run(solver, keyword):
        extra = dict(g=None) if keyword else {}
        k, ft = torch.tensor(kappa, requires_grad=True), dev(f).requires_grad_()
        u = solver.solve(k, ft, **extra)
        (0.5 * torch.sum((u - dev(d)) ** 2)).backward()
        _, du = solver.tangent(dev(kappa), dev(f), dev(dkappa), dev(df), **(dict(g=None, dg=None) if keyword else {}))
        state = (solver.n_solves, solver._generation, solver.last_generate, dict(solver.last_iterations), sorted(solver._warm))
        return [x.detach().cpu().numpy().tobytes() for x in (u, k.grad, ft.grad, du)], state

    results = []
    for keyword in (False, True):
        for name, solver in _solvers():
            solver.warm_start = True
            results.append((name, keyword, run(solver, keyword)))
            assert solver._boundary is None
    for name in ("stored", "matrix_free"):
        plain, with_keyword = [r[2] for r in results if r[0] == name]
        print(name, "state", plain[1], flush=True)
        assert plain[1] == with_keyword[1], (plain[1], with_keyword[1])
        assert plain[1][:2] == (4, 2)
        assert plain[0] == with_keyword[0], name
    print("without g ok")
