"""Eight point sources in one medium: -div(kappa grad u_s) = delta(x - x_s), u_s = 0 on the boundary, s = 0 .. 7, each observed
at a ring of receivers.  The misfit summed over the sources,
    J(kappa) = sum_s 1/2 || R (u_s(kappa) - d_s) ||^2,
and its gradient with respect to kappa cost two batched solves: `solve_many` solves the eight right-hand sides on one generation
of the hierarchy in one `mg_pcg_batch` -- on the matrix-free levels the march rebuilds each row from kappa once for four lanes --
and the backward pass is one more batched solve with the eight cotangents.

The data d_s come from a medium with an inclusion; the gradient at the homogeneous guess points at it.

    python examples/multi_source.py [N=32]
"""
import os
import sys

import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n1, n, S = N + 1, (N + 1) ** 3, 8
dev = torch.device("cuda")
node = lambda i, j, k: (k * n1 + j) * n1 + i

# the sources: the corners of a cube inside the domain; the receivers: every fourth node of the plane z = 3/4
F = torch.zeros(S, n, dtype=torch.float64, device=dev)
lo, hi = N // 4, N - N // 4
for s in range(S):
    F[s, node(hi if s & 1 else lo, hi if s & 2 else lo, hi if s & 4 else lo)] = 1.0
receivers = torch.zeros(n1, n1, n1, dtype=torch.float64, device=dev)
receivers[3 * N // 4, 2:-2:4, 2:-2:4] = 1.0
receivers = receivers.reshape(-1)

# the true medium: kappa = 1 with a ball of kappa = 5 off the centre; the guess: kappa = 1
c = (torch.arange(N, device=dev) + 0.5) / N
ball = ((c[None, None, :] - 0.6) ** 2 + (c[None, :, None] - 0.4) ** 2 + (c[:, None, None] - 0.5) ** 2) < 0.15 ** 2
kappa_true = torch.where(ball, 5.0, 1.0).to(torch.float64).reshape(-1)
kappa = torch.ones(N ** 3, dtype=torch.float64, device=dev, requires_grad=True)

with DiffusionSolver(N, 3, rtol=1e-10, matrix_free_min_rows=0) as solver:
    with torch.no_grad():
        data = solver.solve_many(kappa_true, F)
    U = solver.solve_many(kappa, F)
    J = 0.5 * torch.sum((receivers * (U - data)) ** 2)
    J.backward()
    print(f"N = {N}, {S} sources: J = {float(J):.6e}")
    print(f"  batched solves {solver.n_batched_solves} (one for the data, two for J and its gradient), solves {solver.n_solves}, "
          f"generations {solver.n_generations}")
    print(f"  iterations per lane: forward {solver.last_lane_iterations['forward']}, adjoint {solver.last_lane_iterations['adjoint']}")
    g = kappa.grad.view(N, N, N)
    inside, outside = float(g[ball].mean()), float(g[~ball].mean())
    print(f"  mean dJ/dkappa inside the inclusion {inside:.3e}, outside {outside:.3e}")
    counts = solver.hierarchy.smoother_launches(solver.top)["matrix_free"]
    print(f"  finest level: {counts[1]} Jacobi sweeps in {counts[0]} launches of the matrix-free march")
    assert solver.n_batched_solves == 3 and solver.n_generations == 2
