"""A sealed box: -div(kappa grad u) = f on the unit cube with no flux through any face (`dirichlet_faces="insulated"`).

Part one, the singular case: a point source and an equal point sink at off-grid positions (`point_load`), the potential
difference between two off-grid receivers (`sample`) and its gradient with respect to kappa -- one forward and one adjoint
solve, both the projected solve u = Q A^+ Q^T f, whose u_h has integral zero.  A potential difference does not depend on
that choice of the constant.

Part two, the regular case: three implicit Euler steps of the same body with sigma = 1 / dt and f = 0,
(M / dt + A(kappa)) u_new = M u_old / dt, on one generation of the hierarchy (`same_operator=True`).  No heat leaves an
insulated body: the integral of u_h, w.u with w the lumped mass, is conserved to rounding.

    python examples/insulated_body.py [N=32]
"""
import os
import sys

import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n = (N + 1) ** 3
dev = torch.device("cuda")
f64 = dict(dtype=torch.float64, device=dev)

torch.manual_seed(0)
kappa = torch.exp(0.5 * torch.randn(N ** 3, **f64)).requires_grad_(True)
electrodes = torch.tensor([[0.23, 0.31, 0.67], [0.81, 0.72, 0.28]], **f64)      # source, sink
receivers = torch.tensor([[0.52, 0.18, 0.44], [0.37, 0.83, 0.59]], **f64)
current = torch.tensor([1.0, -1.0], **f64)

with DiffusionSolver(N, 3, rtol=1e-10, dirichlet_faces="insulated") as solver:
    u = solver.solve(kappa, solver.point_load(electrodes, current))
    singular = solver.hierarchy.diffusion_nullspace()
    v = solver.sample(u, receivers)
    dv = v[0] - v[1]
    dv.backward()
    ones = torch.ones(N ** 3, **f64)
    w = solver.reaction_apply(ones, torch.ones(n, **f64)).reshape(-1)           # the lumped mass: w_i = the integral of phi_i
    print(f"sealed box, source and sink: projected solve {singular}, {solver.last_iterations['forward']} + "
          f"{solver.last_iterations['adjoint']} iterations, potential difference {float(dv.detach()):.6e}, "
          f"|d dv / d kappa| {float(kappa.grad.norm()):.6e}, integral of u_h {float(w @ u.detach().reshape(-1)):.1e}")

    dt = 1e-2
    sigma = torch.full((N ** 3,), 1.0 / dt, **f64)
    x = torch.linspace(0.0, 1.0, N + 1, **f64)
    heat = (1.0 + torch.cos(torch.pi * x)[:, None, None] * torch.cos(2 * torch.pi * x)[None, :, None] * x[None, None, :]).reshape(-1)
    k = kappa.detach()
    before = float(w @ heat)
    for step in range(3):
        heat = solver.solve(k, solver.reaction_apply(sigma, heat), sigma=sigma, same_operator=step > 0)
        print(f"step {step + 1}: projected solve {solver.hierarchy.diffusion_nullspace()}, integral of u_h {float(w @ heat.reshape(-1)):.15e} "
              f"(start {before:.15e}), max {float(heat.max()):.4f}, min {float(heat.min()):.4f}")
