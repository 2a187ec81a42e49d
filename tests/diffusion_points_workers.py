"""Bodies of the DiffusionSolver tests of tests/test_diffusion_points.py, and the point sets they share with the kernel tests.
The workers run in a process of their own that imports torch before libmg_hip.so is loaded (one HIP runtime for both); each
prints its figures and ends with an "... ok" line."""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402


def tie_points(N, cells):
    """Points of the given cells whose local coordinates tie: xi_x = xi_y, xi_y = xi_z, xi_x = xi_z and all three equal, with the
    tied value and the other one from {0, 1/4, 1/2, 3/4, 1} -- cell faces (a 0 or a 1), edges, the main diagonal and the inner
    faces between two simplices.  p = (c + xi) / N: exact where N is a power of two, one rounding otherwise."""
    vals = (0.0, 0.25, 0.5, 0.75, 1.0)
    xis = []
    for a, b in itertools.product(vals, vals):
        xis += [(a, a, b), (b, a, a), (a, b, a)]
    xis = np.array(sorted(set(xis)))
    return np.concatenate([(np.array(c, dtype=np.float64) + xis) / N for c in cells])


def special_points(N, seed):
    """What the bit tests locate: 1000 random points; nodes (all of them up to 1000, else the 8 corners and 500 random ones);
    the tie points of the first, the last and a middle cell; every point with coordinates from {0, 1, 0.3}; 1000 points in
    one cell."""
    rng = np.random.default_rng(seed)
    n1 = N + 1
    if n1 ** 3 <= 1000:
        ids = np.arange(n1 ** 3)
    else:
        corners = [((k * n1) + j) * n1 + i for k in (0, N) for j in (0, N) for i in (0, N)]
        ids = np.concatenate([corners, rng.integers(0, n1 ** 3, 500)])
    nodes = np.stack([ids % n1, (ids // n1) % n1, ids // (n1 * n1)], axis=1) / N
    mid = N // 2
    ties = tie_points(N, [(0, 0, 0), (N - 1, N - 1, N - 1), (mid, 0, N - 1)])
    ends = np.array(list(itertools.product((0.0, 1.0, 0.3), repeat=3)))
    crowd = (np.array([mid, N - 1, 0]) + rng.random((1000, 3))) / N
    pts = np.concatenate([rng.random((1000, 3)), nodes, ties, ends, np.minimum(crowd, 1.0)])
    assert pts.min() >= 0.0 and pts.max() <= 1.0
    return np.ascontiguousarray(pts)


def inside_points(N, count, seed, margin=0.05):
    """`count` random points, drawn with a fixed seed and kept only if every local coordinate, every gap between the sorted
    local coordinates and the distance of the largest one to 1 is at least `margin`: a finite-difference step far below
    margin / N never crosses a simplex face."""
    rng = np.random.default_rng(seed)
    kept = []
    while len(kept) < count:
        p = rng.random(3)
        xi = np.sort(p * N - np.floor(p * N))
        if xi[0] >= margin and np.diff(xi).min() >= margin and 1.0 - xi[2] >= margin:
            kept.append(p)
    return np.array(kept)


def gradcheck_worker():
    """torch.autograd.gradcheck and gradgradcheck at torch's default tolerances (those of the flux worker) on `sample`,
    `point_load` and `sample_gradient`, in the fields and in the points, N = 4 and two levels, 12 points from
    `inside_points`.  The maps are bilinear in (field, position inside a simplex), so the differences are exact to rounding.
    Before any solve, so through the grid-only top level."""
    import torch
    from torch.autograd import gradcheck, gradgradcheck
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, M = 4, 12
    rng = np.random.default_rng(5)
    with DiffusionSolver(N, 2) as solver:
        u = torch.tensor(rng.standard_normal((N + 1) ** 3), device="cuda", requires_grad=True)
        X = torch.tensor(inside_points(N, M, seed=6), device="cuda", requires_grad=True)
        w = torch.tensor(rng.standard_normal(M), device="cuda", requires_grad=True)
        assert gradcheck(solver.sample, (u, X))
        assert gradgradcheck(solver.sample, (u, X))
        print("sample(u, X) ok", flush=True)
        assert gradcheck(solver.point_load, (X, w))
        assert gradgradcheck(solver.point_load, (X, w))
        print("point_load(X, w) ok", flush=True)
        assert gradcheck(solver.sample_gradient, (u, X))
        assert gradgradcheck(solver.sample_gradient, (u, X))
        print("sample_gradient(u, X) ok", flush=True)
        # the fourth function, G^T, is reached above only through backward passes: once on its own
        from multigrid_dolfinx_amd.torch_diffusion import _PointGradT
        p = torch.tensor(rng.standard_normal((M, 3)), device="cuda", requires_grad=True)
        assert gradcheck(lambda q: _PointGradT.apply(q, X.detach(), solver), (p,))
        assert gradgradcheck(lambda q: _PointGradT.apply(q, X.detach(), solver), (p,))
        y = solver.sample(u, X)
        assert y.shape == (M,) and solver.point_load(X, w).shape == (N + 1, N + 1, N + 1) and solver.sample_gradient(u, X).shape == (M, 3)
        assert solver.n_solves == 0 and solver.n_generations == 0
    print("gradcheck ok")


def _localisation_case():
    from tests.diffusion_workers import lognormal_kappa
    N = 8
    kappa = lognormal_kappa(N, 3, seed=9)
    receivers = inside_points(N, 10, seed=12)
    # the source sits in a boundary cell, (0, 3, 4), well inside its simplex: its load reaches Dirichlet nodes
    source = (np.array([0.0, 3.0, 4.0]) + np.array([0.6, 0.35, 0.15])) / N
    truth = (np.array([2.0, 5.0, 1.0]) + np.array([0.2, 0.7, 0.45])) / N
    return N, kappa, receivers, source, truth


def end_to_end_worker():
    """N = 8, three levels, rtol 1e-12: J(x_s) = 1/2 ||S(solve(kappa, S^T(1, x_s), g = 0), X_r) - d||^2 with d the samples of the
    solution for another source.  dJ/dx_s from `backward` against central differences of step 1e-4, every evaluation with
    the source inside the simplex it starts in.  u is linear in the load and the load linear in x_s inside a simplex, so J
    is quadratic there and the central difference is exact up to the solver tolerance over the step, about 1e-8 of J's
    scale; 1e-6 of the gradient's norm is required."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, kappa, receivers, source, truth = _localisation_case()
    n1 = N + 1
    step = 1e-4
    with DiffusionSolver(N, 3, rtol=1e-12) as solver:
        k = torch.tensor(kappa, device="cuda")
        Xr = torch.tensor(receivers, device="cuda")
        one = torch.ones(1, dtype=torch.float64, device="cuda")
        zeros = torch.zeros(n1, n1, n1, dtype=torch.float64, device="cuda")
        field = lambda xs: solver.solve(k, solver.point_load(xs.view(1, 3), one), g=zeros)
        d = solver.sample(field(torch.tensor(truth, device="cuda")), Xr).detach()
        J = lambda xs: 0.5 * torch.sum((solver.sample(field(xs), Xr) - d) ** 2)
        before = solver.n_solves
        xs = torch.tensor(source, device="cuda", requires_grad=True)
        load = solver.point_load(xs.view(1, 3), one)
        u = field(xs)
        boundary = torch.tensor(poisson.dirichlet_mask(N, poisson.ALL_FACES), device="cuda").view(n1, n1, n1)
        assert float(load[boundary].abs().max()) > 0.0, "the source's load should reach Dirichlet nodes"
        assert float(u[boundary].abs().max()) == 0.0 and float(u.abs().max()) > 0.0
        assert abs(float(load.sum()) - 1.0) <= 4 * np.finfo(np.float64).eps      # the weights of a point sum to 1
        assert solver.n_solves == before + 1
        Jt = J(xs)
        Jt.backward()
        assert solver.n_solves == before + 3, solver.n_solves                   # u above, J's solve, its adjoint solve
        grad = xs.grad.detach().cpu().numpy()
        fd = np.zeros(3)
        for a in range(3):
            e = np.zeros(3)
            e[a] = step
            with torch.no_grad():
                fd[a] = (float(J(torch.tensor(source + e, device="cuda"))) - float(J(torch.tensor(source - e, device="cuda")))) / (2 * step)
        assert solver.n_solves == before + 9, solver.n_solves
        rel = float(np.linalg.norm(fd - grad) / np.linalg.norm(grad))
        print("J", float(Jt), "backward", grad, "central differences", fd, "relative distance %.3e" % rel, flush=True)
        assert np.linalg.norm(grad) > 0.0
        assert rel <= 1e-6, rel
        # second order through solve composed with the point functions: a Hessian-vector product in the source position
        xs2 = torch.tensor(source, device="cuda", requires_grad=True)
        g1, = torch.autograd.grad(J(xs2), (xs2,), create_graph=True)
        v = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64, device="cuda")
        hv, = torch.autograd.grad(torch.sum(g1 * v), (xs2,))
        # the gradient is affine in x_s inside the simplex, so its central difference is exact up to the gradients' own error
        # (about 1e-11 of their norm at rtol 1e-12) over the step: 1e-3, a twentieth of the source's distance to a face
        grads, wide = [], 1e-3
        for sign in (1.0, -1.0):
            xq = torch.tensor(source + sign * wide * v.cpu().numpy(), device="cuda", requires_grad=True)
            gq, = torch.autograd.grad(J(xq), (xq,))
            grads.append(gq.cpu().numpy())
        hv_fd = (grads[0] - grads[1]) / (2 * wide)
        rel2 = float(np.linalg.norm(hv_fd - hv.cpu().numpy()) / np.linalg.norm(hv_fd))
        print("Hessian-vector product", hv.cpu().numpy(), "differences of gradients", hv_fd, "relative distance %.3e" % rel2, flush=True)
        assert rel2 <= 1e-6, rel2
    print("end to end ok")


def idle_worker():
    """`sample`, `point_load` and `sample_gradient` before any solve work (grid-only top level), have the bytes of the host
    restatements and leave `n_generations` and `n_solves` at 0; the `solve` after them has the bytes of a solver that never
    called them, and calling them after the solve moves neither counter."""
    import torch
    from tests.diffusion_workers import lognormal_kappa
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 16
    rng = np.random.default_rng(33)
    kappa, f = lognormal_kappa(N, 3, seed=6), rng.standard_normal((N + 1) ** 3)
    kt, ft = torch.tensor(kappa, device="cuda"), torch.tensor(f, device="cuda")
    x, pts = rng.standard_normal((N + 1) ** 3), special_points(N, seed=3)
    w = rng.standard_normal(pts.shape[0])
    for min_rows in (None, 0):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as plain:
            want = plain.solve(kt, ft)
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows) as solver:
            xt, Xt, wt = torch.tensor(x, device="cuda"), torch.tensor(pts, device="cuda"), torch.tensor(w, device="cuda")

            def check():
                assert solver.sample(xt, Xt).cpu().numpy().tobytes() == poisson.diffusion_point_sample(N, pts, x).tobytes()
                assert solver.point_load(Xt, wt).cpu().numpy().tobytes() == poisson.diffusion_point_load(N, pts, w).tobytes()
                assert solver.sample_gradient(xt, Xt).cpu().numpy().tobytes() == poisson.diffusion_point_gradient(N, pts, x).tobytes()

            check()
            assert solver.n_solves == 0 and solver.n_generations == 0
            got = solver.solve(kt, ft)
            assert torch.equal(got, want)
            counts = (solver.n_solves, solver.n_generations)
            check()
            assert (solver.n_solves, solver.n_generations) == counts
            assert torch.equal(solver.solve(kt, ft), want)
    print("idle ok")
