"""Bodies of the DiffusionSolver tests of tests/test_diffusion_point_sets.py.  The workers run in a process of their own that
imports torch before libmg_hip.so is loaded (one HIP runtime for both); each prints its figures and ends with an "... ok"
line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.diffusion_batch_workers import EPS, _ascending, _dkappa, _within  # noqa: E402
from tests.diffusion_points_workers import inside_points  # noqa: E402
from tests.diffusion_workers import lognormal_kappa  # noqa: E402

B = 3


def gradcheck_worker():
    """torch.autograd.gradcheck and gradgradcheck at torch's default tolerances on `sample_many`, `point_load_many` and
    `sample_gradient_many`, N = 4 with three levels, B = 3 lanes, 7 points from `inside_points`: in the fields with one located
    set, and in the positions with the set located inside the checked function -- gradcheck writes its inputs in place, and a
    set is a snapshot of its tensor.  The maps are bilinear in (field, position inside a simplex), so the differences are exact
    to rounding.  Before any solve, so through the grid-only top level."""
    import torch
    from torch.autograd import gradcheck, gradgradcheck
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver, _SetGradT
    N, M = 4, 7
    n = (N + 1) ** 3
    rng = np.random.default_rng(15)
    with DiffusionSolver(N, 3) as solver:
        U = torch.tensor(rng.standard_normal((B, n)), device="cuda", requires_grad=True)
        W = torch.tensor(rng.standard_normal((B, M)), device="cuda", requires_grad=True)
        Q = torch.tensor(rng.standard_normal((B, 3 * M)), device="cuda", requires_grad=True)
        X = torch.tensor(inside_points(N, M, seed=16), device="cuda")
        with solver.locate(X) as P:
            assert P.info["M"] == M and P.info["N"] == N
            for name, fn, args in (("sample_many(U, P)", lambda u: solver.sample_many(u, P), (U,)),
                                   ("point_load_many(P, W)", lambda w: solver.point_load_many(P, w), (W,)),
                                   ("sample_gradient_many(U, P)", lambda u: solver.sample_gradient_many(u, P), (U,)),
                                   # the fourth function, G^T, is reached above only through backward passes: once on its own
                                   ("G^T(Q, P)", lambda q: _SetGradT.apply(q, P.source, P), (Q,))):
                assert gradcheck(fn, args)
                assert gradgradcheck(fn, args)
                print(name, "in the fields ok", flush=True)
            # the one-field forms with a located set have the bytes of the tensor forms
            u, w = U[0].detach(), W[0].detach()
            assert torch.equal(solver.sample(u, P), solver.sample(u, X))
            assert torch.equal(solver.point_load(P, w), solver.point_load(X, w))
            assert torch.equal(solver.sample_gradient(u, P), solver.sample_gradient(u, X))
            assert solver.sample_many(U, P).shape == (B, M) and solver.point_load_many(P, W).shape == (B, N + 1, N + 1, N + 1)
            assert solver.sample_gradient_many(U, P).shape == (B, M, 3)
        Xg = X.clone().requires_grad_()
        for name, fn, args in (("sample_many", lambda u, x: solver.sample_many(u, solver.locate(x)), (U, Xg)),
                               ("point_load_many", lambda x, w: solver.point_load_many(solver.locate(x), w), (Xg, W)),
                               ("sample_gradient_many", lambda u, x: solver.sample_gradient_many(u, solver.locate(x)), (U, Xg))):
            assert gradcheck(fn, args)
            assert gradgradcheck(fn, args)
            print(name, "in the fields and the positions ok", flush=True)
        # the position derivative is that of the single calls summed over the lanes
        Y = torch.tensor(rng.standard_normal((B, M)), device="cuda")
        got, = torch.autograd.grad(torch.sum(solver.sample_many(U, solver.locate(Xg)) * Y), (Xg,))
        want = _ascending([torch.autograd.grad(torch.sum(solver.sample(U[b], Xg) * Y[b]), (Xg,))[0] for b in range(B)])
        size = _ascending([(Y[b][:, None] * solver.sample_gradient(U[b].detach(), X)).abs() for b in range(B)])
        _within(got, want, 2 * B * EPS * size, "the position derivative of sample_many against the loop")
        assert solver.n_solves == 0 and solver.n_generations == 0
    print("gradcheck ok")


def survey_worker():
    """N = 8, three levels, matrix-free, rtol 1e-12: B = 3 off-grid sources of strengths w and 12 off-grid receivers.
    U = solve_many(kappa, point_load_many(Ps, diag(w)), g = 0) against three solve(kappa, point_load(X_s[b], w[b]), g = 0): lane b
    of the batched load is the load of source b plus exact zeros (0.0 * lambda added to a node), so its values are the single
    call's.  sample_many(U, Pr) against three sample calls.  J = sum_b 1/2 ||sample(u_b) - d_b||^2 accumulated in ascending
    lane order; dJ/dkappa against the loop's gradients accumulated in the same order.

    Which comparison applies to dJ/dkappa: g is given, so autograd adds the lift's contribution to the solves' in an order of
    its own, which tests/diffusion_batch_workers.py therefore bounds with `_within`.  Here g = 0: the lift's contribution
    D(-lambda, g_B) is a sum of products with entries of g, +-0.0 in every cell, and adding it changes no value wherever it
    enters.  What is left is the sum over the lanes that the batched backward pass forms itself in ascending lane order, so
    the construction of the case without g carries over and `torch.equal` is asserted (the bound of that file, 2 B eps
    sum_b |D(lambda_b, u_b)|, is printed beside it)."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, R = 8, 12
    n1 = N + 1
    dev = lambda x: torch.tensor(x, device="cuda")
    rng = np.random.default_rng(41)
    kappa = lognormal_kappa(N, 3, seed=9)
    sources, receivers = inside_points(N, B, seed=42), inside_points(N, R, seed=43)
    w = np.array([1.0, -0.5, 2.0])
    D = rng.standard_normal((B, R)) * 0.01
    misfit = lambda s, d: 0.5 * torch.sum((s - d) ** 2)
    zeros = torch.zeros(n1, n1, n1, dtype=torch.float64, device="cuda")
    Xs, Xr, wt = dev(sources), dev(receivers), dev(w)
    with DiffusionSolver(N, 3, rtol=1e-12, matrix_free_min_rows=0) as one, DiffusionSolver(N, 3, rtol=1e-12, matrix_free_min_rows=0) as many:
        singles, sizes = [], []
        for b in range(B):
            k = dev(kappa).requires_grad_()
            f = one.point_load(Xs[b:b + 1], wt[b:b + 1]).requires_grad_()
            u = one.solve(k, f, g=zeros)
            s = one.sample(u, Xr)
            gf, gk = torch.autograd.grad(misfit(s, dev(D[b])), [f, k])
            singles.append((f.detach(), u.detach(), s.detach(), gk))
            sizes.append(_dkappa(one, gf.reshape(-1), u.reshape(-1), "interior", "interior").abs())

        Ps, Pr = many.locate(Xs), many.locate(Xr)
        assert many.n_generations == 0 and many.n_solves == 0
        k = dev(kappa).requires_grad_()
        F = many.point_load_many(Ps, torch.diag(wt))
        assert F.shape == (B, n1, n1, n1) and many.n_generations == 0 and many.n_solves == 0
        U = many.solve_many(k, F, g=zeros)
        counts = (many.n_generations, many.n_solves, many.n_batched_solves)
        assert counts == (1, B, 1), counts
        S = many.sample_many(U, Pr)
        assert S.shape == (B, R) and (many.n_generations, many.n_solves, many.n_batched_solves) == counts
        for b in range(B):
            assert torch.equal(F[b], singles[b][0]), ("the load", b)
            assert torch.equal(U[b], singles[b][1]), ("U", b)
            assert torch.equal(S[b], singles[b][2]), ("the samples", b)
        J = _ascending([misfit(S[b], dev(D[b])) for b in range(B)])
        gk, = torch.autograd.grad(J, [k])
        assert (many.n_generations, many.n_solves, many.n_batched_solves) == (1, 2 * B, 2)
        want = _ascending([x[3] for x in singles])
        _within(gk, want, 2 * B * EPS * _ascending(sizes), "dJ/dkappa against the loop (reassociation bound; equality is asserted)")
        assert float(gk.abs().max()) > 0.0
        assert torch.equal(gk, want), float((gk - want).abs().max())

        # a stale set is never read: step the tensor it was located from in place, and every use raises
        Xo = dev(receivers).requires_grad_()
        Po = many.locate(Xo)
        loss = torch.sum(many.sample_many(U.detach(), Po) ** 2)
        loss.backward()
        assert Xo.grad is not None and float(Xo.grad.abs().max()) > 0.0
        with torch.no_grad():
            Xo -= 1e-3 * Xo.grad
        for use in (lambda: many.sample_many(U.detach(), Po), lambda: many.point_load_many(Po, S.detach()),
                    lambda: many.sample_gradient_many(U.detach(), Po), lambda: many.sample(U[0].detach(), Po)):
            try:
                use()
            except RuntimeError as e:
                assert "locate again" in str(e), e
            else:
                raise AssertionError("a stale set was read")
        Po2 = many.locate(Xo)                           # located again: works
        assert many.sample_many(U.detach(), Po2).shape == (B, R)
        assert (many.n_generations, many.n_solves, many.n_batched_solves) == (1, 2 * B, 2)
    print("survey ok")
