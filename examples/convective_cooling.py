"""A heated block cooled by convection: -div(kappa grad u) = q on the unit cube, the base (z-) held at u = 0, the top (z+)
exchanging heat with an ambient at u_ext through a coefficient alpha that varies over the face,
    kappa du/dn + alpha (u - u_ext) = 0,
and no flux through the four sides.  The gradient of a hot-spot functional -- the mean of u^2 over a patch under the top face
-- with respect to alpha says where more cooling pays.

The Robin face enters the operator as the lumped boundary diagonal B(alpha) (`solve(..., robin={"z+": alpha})`) and the
right-hand side as the ambient load alpha u_ext int phi_i = `robin_apply("z+", alpha, u_ext)`; both are differentiable in alpha.

    python examples/convective_cooling.py [N=32]
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

kappa = torch.ones(N ** 3, dtype=torch.float64, device=dev)
alpha = torch.full((N * N,), 5.0, dtype=torch.float64, device=dev, requires_grad=True)  # face-cell (cx, cy) at cy * N + cx
u_ext = torch.full((n,), -0.25, dtype=torch.float64, device=dev)    # the ambient is colder than the base
g = torch.zeros(n, dtype=torch.float64, device=dev)                 # u = 0 on z-
# a heat source in a box off the centre: q = 500 there, as the lumped load q h^3 on interior nodes
c = torch.arange(n1, device=dev) * h
box = ((c > 0.5) & (c < 0.8))[None, None, :] & ((c > 0.3) & (c < 0.6))[None, :, None] & ((c > 0.5) & (c < 0.9))[:, None, None]
f = (500.0 * h ** 3) * box.reshape(-1).to(torch.float64)
# the hot spot: the nodes of the top face above the source
patch = torch.zeros(n1, n1, n1, dtype=torch.bool, device=dev)
patch[N] = ((c > 0.5) & (c < 0.8))[None, :] & ((c > 0.3) & (c < 0.6))[:, None]
patch = patch.reshape(-1)

with DiffusionSolver(N, 3, rtol=1e-10, dirichlet_faces=("z-",)) as solver:
    rhs = f + solver.robin_apply("z+", alpha, u_ext)
    u = solver.solve(kappa, rhs, g, robin={"z+": alpha})
    hot = torch.sum(u[patch] ** 2) / int(patch.sum())
    hot.backward()
    grad = alpha.grad.view(N, N)
    cy, cx = divmod(int(torch.argmin(grad)), N)
    print(f"N = {N}: hot-spot functional {float(hot.detach()):.6e}, max u {float(u.detach().max()):.4f}; d/d alpha is most negative "
          f"({float(grad.min()):.3e}) at face-cell ({cx}, {cy}) of z+, |d/d alpha| {float(grad.norm()):.3e}; "
          f"{solver.n_solves} solves on {solver.n_generations} generation(s)")
