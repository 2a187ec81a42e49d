"""Implicit Euler for du/dt - div(kappa grad u) = f on the unit cube, u = g on the boundary, written as a chain of
`DiffusionSolver.solve` calls, and the gradient of a final-time misfit with respect to kappa through the whole march.

One step is (M / dt + A(kappa)) u_new = M u_old / dt + b: the solve with sigma = 1 / dt in every cell and the right-hand side
b + reaction_apply(sigma, u_old).  dt is constant, so every step after the first reuses the operator (`same_operator=True`):
one generation of the hierarchy serves the march and its backward pass.

    python examples/heat_implicit_euler.py [N=32] [steps=5]
"""
import os
import sys

import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dt = 1e-3
n = (N + 1) ** 3
dev = torch.device("cuda")

kappa = torch.ones(N ** 3, dtype=torch.float64, device=dev, requires_grad=True)
sigma = torch.full((N ** 3,), 1.0 / dt, dtype=torch.float64, device=dev)
b = torch.zeros(n, dtype=torch.float64, device=dev)             # no source
g = torch.zeros(n, dtype=torch.float64, device=dev)             # u = 0 on the boundary
x = torch.linspace(0.0, 1.0, N + 1, dtype=torch.float64, device=dev)
u = (torch.sin(torch.pi * x)[:, None, None] * torch.sin(torch.pi * x)[None, :, None] * torch.sin(torch.pi * x)[None, None, :]).reshape(-1)
target = 0.5 * u

with DiffusionSolver(N, 3, rtol=1e-10) as solver:
    for step in range(steps):
        u = solver.solve(kappa, b + solver.reaction_apply(sigma, u), g, sigma=sigma, same_operator=step > 0)
    misfit = 0.5 * torch.sum((u - target) ** 2) / n
    misfit.backward()
    print(f"{steps} steps of dt = {dt}: misfit {float(misfit.detach()):.6e}, |d misfit / d kappa| {float(kappa.grad.norm()):.6e}, "
          f"{solver.n_solves} solves on {solver.n_generations} generation(s)")
