"""A survey: B point sources and M receivers, all of them off the grid nodes, in one medium.  -div(kappa grad u_b) =
delta(x - x_b), u_b = 0 on the boundary, observed at the receivers x_r:
    J(kappa) = sum_b 1/2 || S(u_b(kappa), x_r) - d_b ||^2.
The positions never change, so they are located once (`locate`): `point_load_many` builds the B consistent loads, `solve_many`
solves them on one generation of the hierarchy, `sample_many` reads all lanes at the receivers, and the backward pass is their
transposes around one more batched solve.  The loop of single calls -- `point_load`, `solve`, `sample` per source, each of which
checks, locates and, for a transpose, sorts the points again -- gives the same bits; the script prints the agreement.

The data d_b come from a medium with an inclusion; the gradient at the homogeneous guess points at it.

    python examples/survey_tomography.py [N=32]
"""
import os
import sys

import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n1, B, M = N + 1, 6, 64
dev = torch.device("cuda")
gen = torch.Generator(device="cuda").manual_seed(3)
rand = lambda *shape: torch.rand(*shape, dtype=torch.float64, device=dev, generator=gen)

# the sources: random points of the lower half; the receivers: random points of a slab near the top; unit strengths
sources = 0.15 + 0.7 * rand(B, 3) * torch.tensor([1.0, 1.0, 0.4], dtype=torch.float64, device=dev)
receivers = 0.1 + 0.8 * rand(M, 3)
receivers[:, 2] = 0.7 + 0.2 * rand(M)
strengths = torch.eye(B, dtype=torch.float64, device=dev)
zeros = torch.zeros(n1, n1, n1, dtype=torch.float64, device=dev)

# the true medium: kappa = 1 with a ball of kappa = 5 off the centre; the guess: kappa = 1
c = (torch.arange(N, device=dev) + 0.5) / N
ball = ((c[None, None, :] - 0.6) ** 2 + (c[None, :, None] - 0.4) ** 2 + (c[:, None, None] - 0.5) ** 2) < 0.15 ** 2
kappa_true = torch.where(ball, 5.0, 1.0).to(torch.float64).reshape(-1)

with DiffusionSolver(N, 3, rtol=1e-10, matrix_free_min_rows=0) as solver:
    Ps, Pr = solver.locate(sources), solver.locate(receivers)
    F = solver.point_load_many(Ps, strengths)           # (B, N + 1, N + 1, N + 1); f on Dirichlet nodes does not count with g given
    with torch.no_grad():
        data = solver.sample_many(solver.solve_many(kappa_true, F, g=zeros), Pr)
    kappa = torch.ones(N ** 3, dtype=torch.float64, device=dev, requires_grad=True)
    S = solver.sample_many(solver.solve_many(kappa, F, g=zeros), Pr)
    J = 0.5 * torch.sum((S[0] - data[0]) ** 2)
    for b in range(1, B):
        J = J + 0.5 * torch.sum((S[b] - data[b]) ** 2)
    J.backward()
    print(f"N = {N}, {B} sources, {M} receivers: J = {float(J.detach()):.6e}")
    print(f"  located sets: sources {Ps.info['bytes']} bytes in {Ps.info['runs']} runs, receivers {Pr.info['bytes']} bytes in "
          f"{Pr.info['runs']} runs")
    print(f"  batched solves {solver.n_batched_solves} (one for the data, two for J and its gradient), solves {solver.n_solves}, "
          f"generations {solver.n_generations}")
    g = kappa.grad.view(N, N, N)
    print(f"  mean dJ/dkappa inside the inclusion {float(g[ball].mean()):.3e}, outside {float(g[~ball].mean()):.3e}")
    assert solver.n_batched_solves == 3 and solver.n_generations == 2

    # the loop of single calls on the tensors themselves: the same loads, samples and -- summed in the same lane order -- gradient
    kappa_loop = torch.ones(N ** 3, dtype=torch.float64, device=dev, requires_grad=True)
    same_loads = same_samples = True
    grad_loop = None
    for b in range(B):
        f = solver.point_load(sources[b:b + 1], strengths[b, b:b + 1])
        s = solver.sample(solver.solve(kappa_loop, f, g=zeros), receivers)
        same_loads &= bool(torch.equal(f, F[b]))
        same_samples &= bool(torch.equal(s, S[b]))
        gb, = torch.autograd.grad(0.5 * torch.sum((s - data[b]) ** 2), [kappa_loop])
        grad_loop = gb if grad_loop is None else grad_loop + gb
    same_grad = bool(torch.equal(grad_loop, kappa.grad))
    print(f"  against the loop of single calls: loads bit-identical {same_loads}, samples bit-identical {same_samples}, "
          f"dJ/dkappa bit-identical {same_grad} (largest difference {float((grad_loop - kappa.grad).abs().max()):.3e})")
    assert same_loads and same_samples and same_grad
