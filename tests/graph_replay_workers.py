"""Bodies of the DiffusionSolver tests of tests/test_graph_replay.py: second-order products on a deep hierarchy, once with
captured V-cycles (the default) and once with "graph" 0, compared byte for byte.  They run in a process of their own that
imports torch before libmg_hip.so is loaded; each prints its figures and ends with an "... ok" line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.diffusion_workers import lognormal_kappa  # noqa: E402

# the smallest shape of tests/test_graph_replay.py's SOLVE_SHAPES: 3^3 .. 65^3
N, LEVELS, RTOL = 64, 6, 1e-6


def _case():
    rng = np.random.default_rng(23)
    n1 = (N + 1) ** 3
    return (lognormal_kappa(N, 3, seed=11), rng.standard_normal(n1), rng.standard_normal(n1), rng.standard_normal(N ** 3),
            rng.standard_normal(n1))


def _solver(graph):
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    solver = DiffusionSolver(N, LEVELS, rtol=RTOL, matrix_free_min_rows=0)
    if not graph:
        solver.hierarchy.set_tuning("graph", 0)
    return solver


def _same(name, runs):
    for key in runs[0]:
        assert runs[0][key].tobytes() == runs[1][key].tobytes(), "%s: %s differs between captured and eager cycles" % (name, key)


def backward_worker():
    """One forward solve and its plain backward pass: the adjoint solve replays, in torch.autograd's thread, the cycle the
    forward solve captured in the caller's."""
    import torch
    kappa, f, d, _, _ = _case()
    runs = []
    for graph in (1, 0):
        with _solver(graph) as solver:
            k = torch.tensor(kappa, requires_grad=True)
            ft = torch.tensor(f, device="cuda", requires_grad=True)
            J = 0.5 * torch.sum((solver.solve(k, ft) - torch.tensor(d, device="cuda")) ** 2)
            J.backward()
            counters = solver.hierarchy.counters()
            print("graph", graph, "solves", solver.n_solves, "iterations", solver.last_iterations, counters, flush=True)
            assert solver.n_solves == 2 and solver._generation == 1, (solver.n_solves, solver._generation)
            assert (counters["graph_replays"] > 0) == bool(graph), counters
            runs.append({"J": J.detach().cpu().numpy().copy(), "grad_kappa": k.grad.numpy().copy(), "grad_f": ft.grad.cpu().numpy().copy()})
            assert all(np.isfinite(x).all() for x in runs[-1].values())
    _same("backward", runs)
    print("backward ok")


def hessian_worker():
    import torch
    kappa, f, d, v, _ = _case()
    runs = []
    for graph in (1, 0):
        with _solver(graph) as solver:
            k = torch.tensor(kappa, requires_grad=True)
            ft = torch.tensor(f, device="cuda", requires_grad=True)
            J = 0.5 * torch.sum((solver.solve(k, ft) - torch.tensor(d, device="cuda")) ** 2)
            (g,) = torch.autograd.grad(J, k, create_graph=True)
            gk, gf = torch.autograd.grad(torch.sum(g * torch.tensor(v)), (k, ft))
            counters = solver.hierarchy.counters()
            print("graph", graph, "solves", solver.n_solves, "iterations", solver.last_iterations, counters, flush=True)
            assert solver.n_solves == 4 and solver._generation == 1, (solver.n_solves, solver._generation)
            assert (counters["graph_replays"] > 0) == bool(graph), counters
            runs.append({"gradient": g.detach().numpy().copy(), "H_kk v": gk.numpy().copy(), "H_fk v": gf.cpu().numpy().copy()})
            assert all(np.isfinite(x).all() for x in runs[-1].values())
    _same("hessian", runs)
    print("hessian ok")


def tangent_worker():
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import _Solve
    kappa, f, d, dkappa, df = _case()
    runs = []
    for graph in (1, 0):
        with _solver(graph) as solver:
            u, du = solver.tangent(torch.tensor(kappa), torch.tensor(f, device="cuda"), torch.tensor(dkappa, device="cuda"),
                                   torch.tensor(df, device="cuda"))
            more = [_Solve.apply(None, torch.tensor(rhs, device="cuda"), solver, solver._last_operator, "tangent", True) for rhs in (d, df)]
            counters = solver.hierarchy.counters()
            print("graph", graph, "solves", solver.n_solves, "iterations", solver.last_iterations, counters, flush=True)
            assert solver.n_solves == 4 and solver._generation == 1, (solver.n_solves, solver._generation)
            assert (counters["graph_replays"] > 0) == bool(graph), counters
            runs.append({"u": u.cpu().numpy().copy(), "du": du.cpu().numpy().copy(), "third": more[0].cpu().numpy().copy(),
                         "fourth": more[1].cpu().numpy().copy()})
            assert all(np.isfinite(x).all() for x in runs[-1].values())
    _same("tangent", runs)
    print("tangent ok")
