"""Where is the source?  -div(kappa grad u) = delta(x - x_s), u = 0 on the boundary, observed at fifty receivers that sit on no
grid node.  The position x_s is recovered from the data by steepest descent on
    J(x_s) = 1/2 || S(u(x_s), X_r) - d ||^2,    u(x_s) = solve(kappa, point_load(x_s, 1), g = 0),
with `point_load` the consistent load of the point source and `sample` the P1 interpolant at the receivers, both
differentiable in the positions.  Inside one simplex of the mesh J is quadratic in x_s, so the exact line step along the
gradient g is g.g / g.Hg with the Hessian-vector product from a second backward pass (`create_graph=True`): four solves per
step.  A step is cut at one cell, h = 1 / N, because the quadratic model ends at the simplex's faces.

    python examples/source_localisation.py [N=32] [steps=20]
"""
import os
import sys

import torch    # (before libmg_hip.so is loaded: one HIP runtime for torch and the library)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n1 = N + 1
dev = torch.device("cuda")
f64 = dict(dtype=torch.float64, device=dev)

# the receivers: a 5 x 5 array under the lid z = 0.77 and one beside the wall x = 0.21, at coordinates of no grid
line = (torch.arange(5, **f64) + 0.5) / 5 * 0.8 + 0.113
a, b = torch.meshgrid(line, line, indexing="ij")
lid = torch.stack([a, b, torch.full_like(a, 0.77)], dim=-1).reshape(-1, 3)
wall = torch.stack([torch.full_like(a, 0.21), a, b - 0.05], dim=-1).reshape(-1, 3)
receivers = torch.cat([lid, wall]).contiguous()

truth = torch.tensor([0.37, 0.58, 0.41], **f64)
kappa = torch.ones(N ** 3, **f64)
one = torch.ones(1, **f64)
zeros = torch.zeros(n1, n1, n1, **f64)

with DiffusionSolver(N, 3, rtol=1e-10) as solver:
    # g = 0: the load of a source in a boundary cell reaches Dirichlet nodes, where f must not be read as boundary data
    field = lambda x: solver.solve(kappa, solver.point_load(x.view(1, 3), one), g=zeros)
    with torch.no_grad():
        data = solver.sample(field(truth), receivers)
    x = torch.tensor([0.5, 0.5, 0.5], **f64)
    first = float(torch.linalg.norm(x - truth))
    print(f"N = {N}, {receivers.shape[0]} receivers, source at {truth.tolist()}, first guess {x.tolist()}: error {first:.3e}")
    for it in range(steps):
        x.requires_grad_(True)
        J = 0.5 * torch.sum((solver.sample(field(x), receivers) - data) ** 2)
        g, = torch.autograd.grad(J, (x,), create_graph=True)
        Hg, = torch.autograd.grad(torch.sum(g * g.detach()), (x,))
        g = g.detach()
        curvature = float(torch.sum(g * Hg))
        step = -(float(torch.sum(g * g)) / curvature) * g if curvature > 0.0 else -g / (N * torch.linalg.norm(g))
        length = float(torch.linalg.norm(step))
        if length > 1.0 / N:
            step = step * (1.0 / N / length)
        x = (x.detach() + step).clamp(0.0, 1.0)
        print(f"  step {it + 1:2d}: J = {float(J):.3e}, position error {float(torch.linalg.norm(x - truth)):.3e}")
    last = float(torch.linalg.norm(x - truth))
    print(f"position error {first:.3e} -> {last:.3e} in {steps} steps, {solver.n_solves} solves")
    assert last < first
