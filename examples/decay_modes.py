"""The three slowest decay modes of rho u_t = div(kappa grad u) in a heterogeneous block that is held at u = 0 on five faces
and cools through the sixth (a Robin face, z+): `DiffusionSolver.eigenpairs` gives the rates lambda_j and the shapes u_j of
u(t) = sum_j c_j exp(-lambda_j t) u_j.

lambda_1 is then checked against what a time march shows: implicit Euler steps (M / dt + K) u_new = M u_old / dt started from
u_1 shrink it by exactly 1 / (1 + dt lambda_1) per step (the steps after the first with `same_operator=True`).  It ends with one
gradient step on kappa that raises lambda_1, the fundamental rate a design problem would maximise: d lambda_1 / d kappa =
D(u_1, u_1), one sensitivity launch and no solve.

    python examples/decay_modes.py [N=32]
"""
import os
import sys

import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
dt, steps = 1e-3, 4
n = (N + 1) ** 3
dev = torch.device("cuda")
gen = torch.Generator(device="cuda").manual_seed(3)

kappa = torch.exp(torch.randn(N ** 3, dtype=torch.float64, device=dev, generator=gen)).requires_grad_()
rho = torch.exp(0.5 * torch.randn(N ** 3, dtype=torch.float64, device=dev, generator=gen))
robin = {"z+": torch.full((N * N,), 5.0, dtype=torch.float64, device=dev)}      # kappa du/dn + 5 u = 0 on z+
zero = torch.zeros(n, dtype=torch.float64, device=dev)

with DiffusionSolver(N, 3, rtol=1e-12, dirichlet_faces=("x-", "x+", "y-", "y+", "z-")) as solver:
    lam, U = solver.eigenpairs(kappa, 3, rho=rho, robin=robin)
    print("decay rates:", ", ".join("%.6f" % v for v in lam.detach().tolist()), f"({solver.last_iterations['eigs']} iterations)")

    # the first mode under implicit Euler: sigma = rho / dt is the mass term of a step
    sigma = rho / dt
    u = U[0].reshape(-1)
    for step in range(steps):
        u_new = solver.solve(kappa.detach(), solver.reaction_apply(sigma, u), zero, sigma=sigma, robin=robin, same_operator=step > 0)
        shrink = float(torch.linalg.vector_norm(u_new) / torch.linalg.vector_norm(u))
        u = u_new
    rate = (1.0 / shrink - 1.0) / dt
    lam1 = float(lam[0].detach())
    print(f"lambda_1 = {lam1:.9f}, from the shrinking of u_1 under {steps} implicit Euler steps: {rate:.9f}")
    assert abs(rate - lam1) <= 1e-6 * lam1, (rate, lam1)

    # one gradient step on kappa that raises the fundamental rate
    lam[0].backward()
    with torch.no_grad():
        better = kappa + 0.1 * kappa.grad / kappa.grad.abs().max()
    lam2, _ = solver.eigenpairs(better, 3, rho=rho, robin=robin, x0=U)
    print(f"after one gradient step on kappa: lambda_1 = {float(lam2[0]):.9f} (was {lam1:.9f})")
    assert float(lam2[0]) > lam1
