"""The diffusion solves against closed-form solutions of -div(kappa grad u) + sigma u = f with Dirichlet, flux and Robin faces.

Every other test of the diffusion layer compares a kernel with its host restatement in poisson.py, or with another kernel; a
convention both get wrong together -- a power of h in a lumped diagonal, the T / 24 share of a load, the sign of a normal or of
`flux`, the half of a face-cell a Robin alpha belongs to, the lift of g next to a free face -- passes them all.  Here the
reference is the PDE: exact fields with hand-written derivatives and loads from an enumeration of the Kuhn mesh's simplices
(tests/pde_reference.py, which calls nothing of the package).  The CPU tests pin the restatements to it (patch test, sine modes,
orders of convergence), the GPU tests the kernels and the torch layer (the same three, a heat march and one gradient)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from multigrid_dolfinx_amd import poisson
from tests import pde_reference as ref
from tests.diffusion_pde_workers import EPS, KAPPA0, MODES, check_orders, host_errors, host_solve, patch_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- host ------------------------------------------------------------------------------------------------------------------------
def test_the_enumerated_weights_are_partitions_of_the_cube_and_its_faces():
    """The reference's own check: 24 simplices at an interior node, 6 N^3 simplices with four corners each, weights that sum
    to the cube's volume and each face's area, and a Robin diagonal that carries every alpha with the face-cell's area."""
    N = 5
    T = ref.simplex_count(N).reshape(N + 1, N + 1, N + 1)
    assert np.all(T[1:-1, 1:-1, 1:-1] == 24.0) and T.sum() == 24.0 * N ** 3
    assert T[0, 0, 0] == 6.0 and T[N, N, N] == 6.0 and T[0, 0, N] == 2.0     # the main diagonal's ends; another corner
    assert abs(ref.volume_weight(N).sum() - 1.0) <= 8 * EPS
    alpha = np.random.default_rng(5).random(N * N)
    for face in ref.FACES:
        w = ref.face_mass(N, face)
        assert abs(w.sum() - 1.0) <= 8 * EPS and not w[~ref.on_face(N, face)].any()
        assert abs(ref.face_mass(N, face, alpha).sum() - alpha.sum() / N ** 2) <= 8 * EPS


LOAD_FACE_SETS = (("x-",), ("x-", "x+"), ("y-", "z+"), ref.FACES)


def _own_load_error(N, kappa, faces, b):
    """The generated levels carry a right-hand side of their own: the constant source `poisson.source_term` and the Dirichlet
    data `poisson.boundary_data`.  On a free row it is f int phi_i less the lift of the data, and int phi_i = h^3 T_i / 24 by the
    reference's count of simplices -- the T / 24 share of a node on a free face, which no solve of a caller's load reads.
    Returns max |b + lift - f h^3 T / 24| over the free rows."""
    x, y, z = ref.node_coords(N)
    g = poisson.boundary_data(np.stack([x, y, z], axis=1), 3)
    free = ~ref.dirichlet_nodes(N, faces)
    want = poisson.source_term(3) * ref.volume_weight(N)
    got = np.asarray(b).reshape(-1) + poisson.diffusion_lift(N, kappa, g, list(faces))
    return float(np.abs(got - want)[free].max())


def _own_load_bound(N):
    """A free row has at most one Dirichlet neighbour per axis, so b is the load 12 h^3 T / 24 less three products a g with
    |a| <= kappa_max h <= 1.75 h and |g| <= 7: every partial sum is below 40 h.  Roundings: seven in each assembled entry, one per
    product, one per subtraction, 27 in all, and at most as many again in the lift that is added back: 64 eps of 40 h."""
    return 64 * EPS * 40.0 / N


@pytest.mark.parametrize("faces", LOAD_FACE_SETS, ids=lambda f: "".join(f))
def test_the_generated_load_is_the_simplex_share_on_the_host(faces):
    N = 6
    kappa = ref.Smooth().kappa(*ref.cell_centres(N))
    level = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=list(faces))
    err = _own_load_error(N, kappa, faces, level.b)
    print("own load", faces, "max error %.3e" % err)
    assert err <= _own_load_bound(N)


@pytest.mark.parametrize("which", [1, 2, 3])
def test_patch_test_on_the_host(which):
    """An affine field with constant kappa and sigma, Dirichlet data, flux data and Robin faces with their ambient values: P1
    holds the field, the lumped terms act on nodal values and the loads are the exact integrals of the constant flux, so the
    discrete solve returns the field at every node.  Not a discretisation error: what is left is the rounding of a direct solve
    of an N = 6 system with |u| < 2.5 (measured 1e-15 to 5e-15; cond(A) eps |u| with cond < 1e3 is 5e-13), and one wrong weight
    leaves 1e-2.  Hence 1e-12."""
    p = patch_problem(which, 6)
    u = host_solve(p)
    err = float(np.abs(u - p.exact).max())
    print("patch test %d: max error %.3e" % (which, err))
    assert err <= 1e-12


@pytest.mark.parametrize("N", [8, 16])
@pytest.mark.parametrize("mode", MODES)
def test_sine_modes_on_the_host(mode, N):
    """With constant kappa and six Dirichlet faces sin(k1 pi x) sin(k2 pi y) sin(k3 pi z) is an eigenvector of the free rows,
    A v = lambda_h h^3 v with lambda_h = kappa sum_d (2 - 2 cos(k_d pi h)) / h^2: exact in real arithmetic, so the residual is
    the rounding of a seven-term row, a few eps of the row's absolute sum 12 kappa h (measured 4e-16 against entries of 0.4);
    1e-13 relative to it leaves two decades.  One implicit Euler step of the lumped scheme, (R + A) u1 = R u0 with R = h^3 / dt,
    divides the mode by 1 + dt lambda_h."""
    h = 1.0 / N
    kappa = np.full(N ** 3, KAPPA0)
    A = poisson.diffusion_level(N, 3, kappa).A.tocsr()
    free = ~poisson.dirichlet_mask(N)
    v = ref.sine_mode(N, mode)
    lam = ref.sine_eigenvalue(N, mode, KAPPA0)
    r = (A @ v - lam * h ** 3 * v)[free]
    scale = 12.0 * KAPPA0 * h * np.abs(v).max()
    print("mode", mode, "N", N, "lambda_h %.6f eigen residual %.3e of %.3e" % (lam, np.abs(r).max(), scale))
    assert np.abs(r).max() <= 1e-13 * scale
    dt = 1e-3
    sigma = np.full(N ** 3, 1.0 / dt)
    step = poisson.diffusion_level(N, 3, kappa, sigma=sigma).A.tocsc()
    u1 = spl.spsolve(step, poisson.diffusion_apply_dsigma(N, sigma, v))
    want = v / (1.0 + dt * lam)
    # the direct solve's rounding: cond(R + A) eps, cond <= 1 + 12 kappa dt / h^2 (Gershgorin) < 8 here; 1e-13 as above
    assert np.abs(u1 - want).max() <= 1e-13 * np.abs(v).max()


@pytest.mark.parametrize("config", ["a", "b"])
def test_orders_of_convergence_on_the_host(config):
    """N = 8, 16, 32 with the smooth field: second order (p >= 1.8) in the nodal values, the cell flux at the cell centres and
    the interpolant at 500 random points, first order (0.9 <= p <= 1.2) in the simplex gradient at those points, in the root
    mean square (with free faces the nodal quadrature of the reference's loads leaves a maximum error on the cube's free edges
    that falls more slowly; it is the quadrature's, not the operator's)."""
    check_orders("host " + config, {N: host_errors(config, N) for N in (8, 16, 32)})


# ---- device ----------------------------------------------------------------------------------------------------------------------
def _torch_first(worker, *args):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_pde_workers as w; w.%s(*%r)" % (ROOT, worker, args)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("min_rows", [None, 0], ids=["stored", "matrix_free"])
def test_the_generated_load_is_the_simplex_share_on_the_device(min_rows):
    """The right-hand side `gen_diffusion_hierarchy` leaves on the top level, N = 8 and three levels, on the face sets of the
    host test: f h^3 T / 24 less the lift on every free row."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N, top = 8, 2
    kappa = ref.Smooth().kappa(*ref.cell_centres(N))
    for faces in LOAD_FACE_SETS:
        with DeviceHierarchy(3, 0, top, c=N >> top) as h:
            h.set_prolongation("p1")
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
            h.set_diffusion_faces(list(faces))
            h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=min_rows)
            assert h.level_matrix_free(top) == (min_rows == 0)
            err = _own_load_error(N, kappa, faces, h.get_vector(top, "f"))
        print("own load", faces, "max error %.3e" % err)
        assert err <= _own_load_bound(N)


@pytest.mark.gpu
def test_patch_test_on_the_device():
    """The affine field through `DiffusionSolver.solve` (g, flux loads in f, sigma=, robin=, the ambient load by `robin_apply`) at
    N = 8 on the three face sets, stored and matrix-free: the solution within what the stopping rule allows (`last_residual`
    ||rhs|| / lambda_min of the host matrix, `solve_error_bound`), and `flux` = -kappa slope in every cell, `sample` and
    `sample_gradient` the field and the slope at 500 points to the same accuracy (`patch_worker`)."""
    assert "patch ok" in _torch_first("patch_worker")


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["a", "b"])
def test_orders_of_convergence_on_the_device(config):
    """The orders of the host test through `solve`, `flux`, `sample` and `sample_gradient` with the same thresholds, stored and matrix-free; the
    device solution within ROBIN_LIMIT (tests/diffusion_robin_workers.py) of the host's sparse direct solution in relative l2,
    so that the orders are the host's; `solve_many` with two loads as lanes gives the bytes of `solve` (`orders_worker`)."""
    assert "orders ok" in _torch_first("orders_worker", config)


def _mode_handle(N, min_rows, omega):
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    nlev = 3 if N == 16 else 4
    top = nlev - 1
    h = DeviceHierarchy(3, 0, top, c=N >> top)
    h.set_prolongation("p1")
    h.set_params(2, 2, omega, restriction="p1_transpose")
    h.gen_diffusion_hierarchy(np.full(N ** 3, KAPPA0), matrix_free_min_rows=min_rows)
    assert h.level_matrix_free(top) == (min_rows == 0)
    return h, top


# Roundings that can reach one row's result in one Jacobi sweep v + omega (f - A v) / d, relative to ||v||_inf.  A v: 7 products
# and 6 adds; f - A v, the division by d (or a reciprocal and a product: one more), the product with omega, the add to v: 5; the
# stored entries of the row carry the roundings of their assembly (three adds, two doublings, a division and a product per edge
# sum: 7, and the diagonal's six adds on top: 13 at most).  13 + 5 + 13 = 31 roundings, each of an intermediate that is at most
# sum_j |a_ij| |v_j| / d <= 2 ||v||_inf (the row's absolute sum is 2 d): 62 eps ||v||_inf per sweep.  The sweep's matrix
# I - omega D^-1 A has infinity norm <= 1 for omega <= 1, so the sweeps' roundings add.  The mode enters rounded (1 eps, carried
# through with norm <= 1) and the closed form's factor has the roundings of a cosine, five adds, three products and the power
# (under 16 n eps): 64 in all.
ROW_ROUNDINGS = 64


@pytest.mark.gpu
@pytest.mark.parametrize("min_rows", [None, 0], ids=["stored", "matrix_free"])
@pytest.mark.parametrize("N", [16, 32])
def test_sine_modes_on_the_device(N, min_rows):
    """Constant kappa, six Dirichlet faces, f = 0, modes (2,1,3) and (1,1,1) in v: `residual` gives -lambda_h h^3 v on the free
    rows, `quadratic_form` lambda_h h^3 ||v||^2, and n Jacobi sweeps scale the mode by (1 - omega lambda_h h^2 / (6 kappa))^n for
    n = 1, 5 (a whole K-sweep pass where the level takes one) and 7 (a pass and a tail).  The closed forms are exact in real
    arithmetic; the tolerances are rounding bounds (ROW_ROUNDINGS).  Which smoother path ran is printed, not asserted."""
    omega = 2.0 / 3.0
    hh = 1.0 / N
    d = 6.0 * KAPPA0 * hh
    h, top = _mode_handle(N, min_rows, omega)
    with h:
        n_nodes = (N + 1) ** 3
        for mode in MODES:
            v = ref.sine_mode(N, mode)
            lam = ref.sine_eigenvalue(N, mode, KAPPA0)
            vmax = float(np.abs(v).max())
            h.set_vector(top, "v", v)
            h.zero_vector(top, "f")
            h.residual(top)
            r = h.get_vector(top, "r").reshape(-1)
            err = float(np.abs(r + lam * hh ** 3 * v).max())
            # one application of A: the intermediates are at most 2 d ||v||_inf
            assert err <= ROW_ROUNDINGS * EPS * 2.0 * d * vmax, (mode, err)
            q = h.quadratic_form(top, "v")
            want = lam * hh ** 3 * float(v @ v)
            # the rows as above, then a sum over the nodes whose order is the kernel's: at worst one rounding per node of the
            # running sum, sum_i |v_i| (|A| |v|)_i <= 2 d ||v||_2^2
            assert abs(q - want) <= (ROW_ROUNDINGS + n_nodes) * EPS * 2.0 * d * float(v @ v), (mode, q, want)
            print("mode", mode, "N", N, "residual error %.3e  quadratic form relative %.3e" % (err, abs(q - want) / want))
            factor = 1.0 - omega * lam * hh ** 2 / (6.0 * KAPPA0)
            for n in (1, 5, 7):
                h.set_vector(top, "v", v)
                h.reset_smoother_launches()
                h.smooth(top, n)
                got = h.get_vector(top, "v").reshape(-1)
                err = float(np.abs(got - factor ** n * v).max())
                print("  smooth n = %d factor^n %.6e error %.3e (bound %.3e) paths %s"
                      % (n, factor ** n, err, ROW_ROUNDINGS * n * EPS * vmax, h.smoother_launches(top)))
                assert err <= ROW_ROUNDINGS * n * EPS * vmax, (mode, n, err)


@pytest.mark.gpu
def test_heat_decay_on_the_device():
    """Five implicit Euler steps at N = 16, dt = 1e-3: `solve(..., sigma=1/dt, same_operator=True)` on `reaction_apply(sigma,
    u_old)` divides the mode by 1 + dt lambda_h per step, to the accumulated solver tolerance; one generation (`heat_worker`)."""
    assert "heat ok" in _torch_first("heat_worker")


@pytest.mark.gpu
def test_the_gradient_of_a_uniform_kappa_on_the_device():
    """J = 1/2 ||u||^2 with f a sine mode: the sum of `grad_kappa` is dJ/dkappa of a uniform kappa, -||u||^2 / kappa with
    u = f / (lambda_h h^3); one solve and one backward pass at N = 16 (`derivative_worker`)."""
    assert "derivative ok" in _torch_first("derivative_worker")
