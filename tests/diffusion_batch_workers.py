"""DiffusionSolver.solve_many test bodies of tests/test_diffusion_batch.py.  They run in a process of their own that imports
torch before libmg_hip.so is loaded (one HIP runtime for both); each prints its figures and ends with an "... ok" line.

What is compared to the byte: everything a lane computes by itself (U[b], grad_F[b]) and every sum the batched backward pass
forms itself, in ascending lane order with the first term starting the accumulator (grad_kappa, grad_sigma, grad_alpha without
g).  Where autograd chooses the order of an accumulation -- the lift's contribution with g, the two passes of a Hessian-vector
product -- the comparison is within the reassociation bound n eps sum |addends| (n addends; two summation orders of the same
addends differ by at most 2 (n - 1) u sum |addends|, u = eps / 2), the addends' sizes taken from single solves."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.diffusion_reaction_workers import reaction_sigma  # noqa: E402
from tests.diffusion_robin_workers import robin_alpha  # noqa: E402
from tests.diffusion_workers import lognormal_kappa  # noqa: E402

EPS = np.finfo(np.float64).eps
B = 3


def _fields(N, seed=0):
    rng = np.random.default_rng(50 + N + seed)
    n = (N + 1) ** 3
    return lognormal_kappa(N, 3, seed=4), rng.standard_normal((B, n)), rng.standard_normal((B, n)), rng.standard_normal((B, n))


def _ascending(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _within(got, want, bound, what):
    """|got - want| <= bound elementwise; prints the largest difference and the largest ratio to the bound."""
    diff = (got - want).abs()
    ratio = float((diff / bound.clamp_min(1e-300)).max())
    print("%s: largest difference %.3e, largest difference / bound %.3f" % (what, float(diff.max()), ratio), flush=True)
    assert bool((diff <= bound).all()), (what, float(diff.max()), ratio)


def _dkappa(solver, a, b, a_nodes, b_nodes):
    import torch
    out = torch.empty(solver.N ** 3, dtype=torch.float64, device="cuda")
    a, b = a.detach().contiguous(), b.detach().contiguous()
    torch.cuda.synchronize()
    solver.hierarchy.diffusion_dkappa(solver.top, a.data_ptr(), b.data_ptr(), out.data_ptr(), a_nodes=a_nodes, b_nodes=b_nodes)
    return out


def gradients_worker(N, nlev):
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    dev = lambda x: torch.tensor(x, device="cuda")
    kappa, F, D, G = _fields(N)
    faces, bits = 18, (1, 32)                # Dirichlet on x+ and z-; Robin fields on x- and z+
    misfit = lambda u, d: 0.5 * torch.sum((u - d) ** 2)

    # ---- without g: kappa, sigma, two Robin fields, the right-hand sides ----
    with DiffusionSolver(N, nlev, matrix_free_min_rows=0, dirichlet_faces=faces) as one, \
            DiffusionSolver(N, nlev, matrix_free_min_rows=0, dirichlet_faces=faces) as many:
        leaves = lambda: (dev(kappa).requires_grad_(), dev(reaction_sigma(N)).requires_grad_(),
                          {bit: dev(robin_alpha(N, bit)).requires_grad_() for bit in bits})
        singles = []
        for b in range(B):
            k, s, al = leaves()
            f = dev(F[b]).requires_grad_()
            u = one.solve(k, f, sigma=s, robin=al)
            singles.append((u.detach(),) + torch.autograd.grad(misfit(u, dev(D[b])), [f, k, s] + [al[bit] for bit in bits]))
        k, s, al = leaves()
        Ft = dev(F).requires_grad_()
        U = many.solve_many(k, Ft, sigma=s, robin=al)
        assert U.shape == Ft.shape and many.n_generations == 1 and many.n_batched_solves == 1 and many.n_solves == B
        J = _ascending([misfit(U[b], dev(D[b])) for b in range(B)])
        grads = torch.autograd.grad(J, [Ft, k, s] + [al[bit] for bit in bits])
        assert many.n_batched_solves == 2 and many.n_solves == 2 * B and many.n_generations == 1
        assert len(many.last_lane_iterations["forward"]) == B and many.last_iterations["forward"] == max(many.last_lane_iterations["forward"])
        assert len(many.last_lane_iterations["adjoint"]) == B and many.last_iterations["adjoint"] == max(many.last_lane_iterations["adjoint"])
        print("iterations per lane:", many.last_lane_iterations, flush=True)
        for b in range(B):
            assert torch.equal(U[b], singles[b][0]), ("U", b)
            assert torch.equal(grads[0][b], singles[b][1]), ("grad_F", b)
        for q, name in enumerate(["grad_kappa", "grad_sigma"] + ["grad_alpha[%d]" % bit for bit in bits]):
            want = _ascending([singles[b][2 + q] for b in range(B)])
            assert torch.equal(grads[1 + q], want), (name, float((grads[1 + q] - want).abs().max()))
        assert many.hierarchy.batch_info()["lanes"] == B - 1
        # one lane, and F with more than one trailing dimension
        U1 = many.solve_many(dev(kappa), dev(F[:1]).view(1, N + 1, N + 1, N + 1), sigma=s.detach(), robin={bit: al[bit].detach() for bit in bits})
        assert U1.shape == (1, N + 1, N + 1, N + 1) and torch.equal(U1.reshape(-1), singles[0][0])

    # ---- with g, per lane and shared: all six faces Dirichlet ----
    with DiffusionSolver(N, nlev, matrix_free_min_rows=0) as one, DiffusionSolver(N, nlev, matrix_free_min_rows=0) as many:
        boundary = many._boundary_mask()
        for shared in (False, True):
            Gs = np.repeat(G[:1], B, axis=0) if shared else G
            singles, scale_k, scale_g = [], [], []
            for b in range(B):
                k, f, g = dev(kappa).requires_grad_(), dev(F[b]).requires_grad_(), dev(Gs[b]).requires_grad_()
                u = one.solve(k, f, g)
                gf, gk, gg = torch.autograd.grad(misfit(u, dev(D[b])), [f, k, g])
                singles.append((u.detach(), gf, gk, gg))
                # the addends autograd accumulates, their sizes from this single solve.  grad_kappa: -D(lambda, u) from the solve
                # and D(-lambda, g_B; interior, all) from the lift (lambda inside = grad_F).  grad_g on the boundary: lambda there
                # (the boundary rows are identity rows: lambda = grad_u = u - d) and the lift's transpose (the rest of grad_g)
                g_b = torch.where(boundary, g.detach(), torch.zeros_like(gf))
                scale_k.append(_dkappa(one, gf, u, "interior", "interior").abs() + _dkappa(one, gf, g_b, "interior", "all").abs())
                lam_b = torch.where(boundary, u.detach() - dev(D[b]), torch.zeros_like(gf))
                scale_g.append(lam_b.abs() + (gg - lam_b).abs())
            k, Ft = dev(kappa).requires_grad_(), dev(F).requires_grad_()
            gt = dev(G[0] if shared else G).requires_grad_()
            U = many.solve_many(k, Ft, gt)
            J = _ascending([misfit(U[b], dev(D[b])) for b in range(B)])
            gF, gk, gg = torch.autograd.grad(J, [Ft, k, gt])
            for b in range(B):
                assert torch.equal(U[b], singles[b][0]), ("U with g", shared, b)
                assert torch.equal(gF[b], singles[b][1]), ("grad_F with g", shared, b)
            tag = "shared g" if shared else "g per lane"
            _within(gk, _ascending([x[2] for x in singles]), 2 * B * EPS * _ascending(scale_k), "grad_kappa, " + tag)
            if shared:      # 2 B addends in one accumulation
                _within(gg, _ascending([x[3] for x in singles]), 2 * B * EPS * _ascending(scale_g), "grad_g, " + tag)
            else:           # two addends per lane
                for b in range(B):
                    _within(gg[b], singles[b][3], 2 * EPS * scale_g[b], "grad_g[%d], %s" % (b, tag))
            assert not bool(gg.reshape(-1, boundary.numel())[:, ~boundary].any())
    print("gradients ok")


def hvp_worker(N, nlev):
    """d/dkappa of (dJ/dkappa . v) for J = sum_b J(u_b), through create_graph=True: four batched solves on one generation,
    against the sum of B single-solve products.  Per lane the product is -D(lambda', u) - D(lambda, u') (u', lambda': the
    derivatives of u and lambda along v); the batched pass sums each of the two over the lanes and then adds the sums, a single
    solve adds its two and the test then sums over lanes: 2 B addends, whose sizes come from `tangent` on single solves."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    dev = lambda x: torch.tensor(x, device="cuda")
    kappa, F, D, _ = _fields(N, seed=1)
    v = dev(np.random.default_rng(9).standard_normal(N ** 3))
    misfit = lambda u, d: 0.5 * torch.sum((u - d) ** 2)
    with DiffusionSolver(N, nlev, matrix_free_min_rows=0, rtol=1e-12) as one, DiffusionSolver(N, nlev, matrix_free_min_rows=0, rtol=1e-12) as many:
        products, sizes = [], []
        for b in range(B):
            k = dev(kappa).requires_grad_()
            u = one.solve(k, dev(F[b]))
            (gk,) = torch.autograd.grad(misfit(u, dev(D[b])), [k], create_graph=True)
            (hv,) = torch.autograd.grad(torch.sum(gk * v), [k])
            products.append(hv)
            with torch.no_grad():
                ub, du = one.tangent(dev(kappa), dev(F[b]), v)
                lam, dlam = one.tangent(dev(kappa), ub - dev(D[b]), v, df=du)
                sizes.append(_dkappa(one, dlam, ub, "interior", "interior").abs() + _dkappa(one, lam, du, "interior", "interior").abs())
        k = dev(kappa).requires_grad_()
        U = many.solve_many(k, dev(F))
        J = _ascending([misfit(U[b], dev(D[b])) for b in range(B)])
        (gk,) = torch.autograd.grad(J, [k], create_graph=True)
        assert many.n_batched_solves == 2
        (hv,) = torch.autograd.grad(torch.sum(gk * v), [k])
        assert many.n_batched_solves == 4 and many.n_generations == 1 and many.n_solves == 4 * B, (many.n_batched_solves, many.n_generations, many.n_solves)
        _within(hv, _ascending(products), 2 * B * EPS * _ascending(sizes), "Hessian-vector product")
        assert float(hv.abs().max()) > 0.0
    print("hvp ok")


def bookkeeping_worker(N, nlev):
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver, NotConverged
    dev = lambda x: torch.tensor(x, device="cuda")
    kappa, F, D, _ = _fields(N, seed=2)
    F[1] = 0.0                                  # a lane that needs no iteration
    with DiffusionSolver(N, nlev, matrix_free_min_rows=0, max_iter=1) as solver:
        try:
            solver.solve_many(dev(kappa), dev(F))
            raise AssertionError("max_iter = 1 was reported as converged")
        except NotConverged as exc:
            assert "lanes [0, 2] of 3" in str(exc), str(exc)
        assert solver.last_lane_iterations["forward"] == [1, 0, 1] and solver.n_solves == B and solver.n_batched_solves == 1
    with DiffusionSolver(N, nlev, matrix_free_min_rows=0, warm_start=True) as solver:
        U = solver.solve_many(dev(kappa), dev(F))
        assert solver.n_generations == 1 and solver.last_lane_iterations["forward"][1] == 0
        cold = list(solver.last_lane_iterations["forward"])
        again = solver.solve_many(dev(kappa), dev(F), same_operator=True)       # no generation; starts from the kept solution
        assert solver.n_generations == 1 and solver.n_batched_solves == 2
        assert solver.last_iterations["forward"] <= 1 < max(cold), (solver.last_lane_iterations, cold)
        assert float((again - U).abs().max()) <= 1e-8 * float(U.abs().max())
        two = solver.solve_many(dev(kappa), dev(F[:2]), same_operator=True)      # another B: from zero
        assert solver.last_lane_iterations["forward"] == cold[:2] and torch.equal(two[0], U[0])
        single = solver.solve(dev(kappa), dev(F[0]))                          # a plain solve beside the lanes
        assert solver.n_generations == 2
        assert solver.hierarchy.batch_info()["lanes"] == B - 1
        try:
            solver.solve_many(dev(kappa), dev(F[0]))
            raise AssertionError("a right-hand side without leading rows was accepted")
        except ValueError as exc:
            assert "leading rows" in str(exc)
        h = solver.hierarchy
    assert not h._h                              # closed: the lanes went with the handle
    with DiffusionSolver(N, nlev, matrix_free_min_rows=0) as plain:
        assert torch.equal(plain.solve(dev(kappa), dev(F[0])), single)
    print("bookkeeping ok")
