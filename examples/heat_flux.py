"""Where the heat of the block of convective_cooling.py goes: -div(kappa grad u) = q on the unit cube, the base (z-) held
at u = 0, the top (z+) exchanging heat with a colder ambient through alpha, no flux through the four sides.
`DiffusionSolver.flux(kappa, u)` gives the cell averages of q = -kappa grad u_h.  The heat leaving through the base is taken
from the bottom cell layer, -sum q_z h^2 (the outward normal is -z); the heat leaving through the top is the Robin term,
sum_i b(alpha)_i (u_i - u_ext); their sum is printed beside the total source.

The balance closes to the solver's tolerance, not merely to discretisation accuracy: the hat functions of the base nodes add
up to 1 - z / h on the bottom layer, so -sum q_z h^2 over that layer IS the nodal reaction at the base, and the P1 equations
conserve heat exactly.  What is only discretisation-accurate is the flux itself, cell by cell.  How the heat splits between
base and top depends on kappa; the gradient of the base's share with respect to kappa comes from one adjoint solve.

    python examples/heat_flux.py [N=32]
"""
import os
import sys

import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n1, n = N + 1, (N + 1) ** 3
dev = torch.device("cuda")
h = 1.0 / N

kappa = torch.ones(N ** 3, dtype=torch.float64, device=dev, requires_grad=True)
alpha = torch.full((N * N,), 5.0, dtype=torch.float64, device=dev)  # face-cell (cx, cy) at cy * N + cx
u_ext = torch.full((n,), -0.25, dtype=torch.float64, device=dev)    # the ambient is colder than the base
g = torch.zeros(n, dtype=torch.float64, device=dev)                 # u = 0 on z-
# a heat source in a box off the centre: q = 500 there, as the lumped load q h^3 on interior nodes
c = torch.arange(n1, device=dev) * h
box = ((c > 0.5) & (c < 0.8))[None, None, :] & ((c > 0.3) & (c < 0.6))[None, :, None] & ((c > 0.5) & (c < 0.9))[:, None, None]
f = (500.0 * h ** 3) * box.reshape(-1).to(torch.float64)

with DiffusionSolver(N, 3, rtol=1e-10, dirichlet_faces=("z-",)) as solver:
    rhs = f + solver.robin_apply("z+", alpha, u_ext)
    u = solver.solve(kappa, rhs, g, robin={"z+": alpha})
    q = solver.flux(kappa, u)                                       # (3, N, N, N), [d, ck, cj, ci]
    base = -torch.sum(q[2, 0]) * h ** 2
    top = torch.sum(solver.robin_apply("z+", alpha, u - u_ext))
    base.backward()
    grad = kappa.grad.view(N, N, N)
    ck, rest = divmod(int(torch.argmax(grad.abs())), N * N)
    cj, ci = divmod(rest, N)
    source = float(f.sum())
    print(f"N = {N}: heat leaving through the base {float(base.detach()):.6e}, through the top {float(top.detach()):.6e}, "
          f"together {float((base + top).detach()):.6e}, total source {source:.6e} "
          f"(imbalance {abs(float((base + top).detach()) - source) / source:.1e}); largest |q| {float(q.detach().norm(dim=0).max()):.4f}; "
          f"d base / d kappa is largest ({float(grad[ck, cj, ci]):.3e}) in cell ({ci}, {cj}, {ck}), |d/d kappa| {float(grad.norm()):.3e}; "
          f"{solver.n_solves} solves on {solver.n_generations} generation(s)")
