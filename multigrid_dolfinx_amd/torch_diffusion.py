"""Differentiable solves of -div(kappa grad u) = f on the device: `DiffusionSolver.solve(kappa, f) -> u` with gradients
with respect to kappa and f by the adjoint method.

The only module of the package that imports torch.  Tensors enter and leave `libmg_hip.so` by device pointer
(`mg_set_vector_device`, `mg_get_vector_device`, `mg_diffusion_dkappa`).  So does a kappa that lives on the solver's
device: the first solve generates the hierarchy from its address (`mg_gen_diffusion_hierarchy_device`), later solves put
the new kappa into the hierarchy that is there (`mg_refresh_diffusion_hierarchy`), and nothing of kappa crosses to the
host.  A kappa on the CPU is uploaded as `mg_gen_diffusion_hierarchy` takes it.

Import order matters: torch (or this module) must be imported before anything loads `libmg_hip.so`, so that the library
binds to the HIP runtime torch ships and both see the same device memory; `DiffusionSolver` raises otherwise.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .hierarchy import DeviceHierarchy

__all__ = ["DiffusionSolver", "NotConverged"]


class NotConverged(RuntimeError):
    """`mg_pcg` reached `max_iter` before the tolerance: no solution, and no gradient, is returned."""


def _need_one_hip_runtime():
    """torch ships its own HIP runtime under the soname libmg_hip.so links against.  Imported first, torch's copy serves
    both and a device pointer means the same to both; a libmg_hip.so loaded earlier is bound to another copy, torch cannot
    initialise beside it and its pointers would mean nothing to the library."""
    from . import _capi
    _capi.load()
    with open("/proc/self/maps") as fh:
        copies = {line.split()[-1] for line in fh if "libamdhip64" in line}
    if len(copies) > 1:
        raise RuntimeError("libmg_hip.so was loaded before torch and uses another HIP runtime than torch does (" +
                           ", ".join(sorted(copies)) + "): import torch before anything loads libmg_hip.so -- "
                           "import multigrid_dolfinx_amd.torch_diffusion (or torch) first in the process")


class DiffusionSolver:
    """u(kappa, f) = A(kappa)^-1 f for the P1 matrix of -div(kappa grad u) on the unit cube with N^3 cells
    (`poisson.diffusion_level`), solved by `mg_pcg` on a hierarchy of `n_levels` generated levels with P1 transfers.

    Contract: `f` is the FULL right-hand side in lexicographic node order, boundary entries included.  Boundary rows are
    identity rows, so u_b = f_b, and interior rows have no boundary column.  A lifted inhomogeneous Dirichlet load (the
    -a_ib g_b terms that `mg_gen_diffusion_level` folds into its own right-hand side) depends on kappa itself; that
    dependence is the caller's: build the lifted f from kappa with differentiable torch operations if it matters.

    `kappa`: N^3 positive float64, cell (ci, cj, ck) at (ck * N + cj) * N + ci, any shape, on the CPU (uploaded, every
    level regenerated) or on the solver's device (it stays there: the first solve generates, later ones refresh in
    place; `last_generate` says which of "host", "device", "refresh" the last one was).  `f`, `u`: (N + 1)^3 float64 on
    the handle's device.  `averaging` and `matrix_free_min_rows` as in `DeviceHierarchy.gen_diffusion_hierarchy`; `set_params` are those of
    `DeviceHierarchy.set_params` (defaults: V(2,2), omega 2/3, Jacobi; the restriction is always the P1 transpose).

    backward: one more `mg_pcg` on the same hierarchy (A is symmetric), A lambda = grad_u; then grad_f = lambda and
    grad_kappa = -mg_diffusion_dkappa(lambda, u).  A solve that reaches `max_iter` raises `NotConverged`.

    `warm_start=True` keeps the last forward and the last adjoint solution and starts the next solve of each kind from
    them instead of from zero (kappa that moves a little between solves).  The stopping test is relative to the
    right-hand side either way, so the gradients are those of the converged solve."""

    def __init__(self, N: int, n_levels: int, averaging: str = "arithmetic", matrix_free_min_rows: Optional[int] = None,
                 rtol: float = 1e-10, max_iter: int = 200, device: int = 0, warm_start: bool = False, **set_params):
        if n_levels < 2 or N % (1 << (n_levels - 1)):
            raise ValueError("N must be a multiple of 2^(n_levels - 1), with at least two levels")
        self.N, self.top = int(N), n_levels - 1
        self.averaging, self.matrix_free_min_rows = averaging, matrix_free_min_rows
        self.rtol, self.max_iter = float(rtol), int(max_iter)
        self.device = torch.device("cuda", device)
        _need_one_hip_runtime()
        self.hierarchy = DeviceHierarchy(3, 0, self.top, c=N >> self.top, device=device)
        params = dict(mu1=2, mu2=2, omega=2.0 / 3.0)
        params.update(set_params)
        params["restriction"] = "p1_transpose"
        self.hierarchy.set_params(**params)
        self.hierarchy.set_prolongation("p1")
        self._generation = 0
        self._generated = False         # a hierarchy call has generated the levels: a device kappa can refresh them
        self.last_generate = None       # "host" / "device" / "refresh": how the last kappa reached the hierarchy
        self.warm_start = bool(warm_start)
        self._warm = {}                 # "forward" / "adjoint": the last solution of that kind (warm_start)
        self.last_iterations = {}       # "forward" / "adjoint": iterations of the last solve of that kind
        self.last_residual = {}         # ... and ||r|| / ||rhs|| of mg_pcg's recursion where it stopped (None: no iteration was needed)

    def close(self):
        self.hierarchy.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def solve(self, kappa: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
        return _Solve.apply(kappa, f, self)

    # ---- what the autograd function calls --------------------------------------------------------------------
    def _generate(self, kappa) -> int:
        """`kappa`: a host array (today's path) or a contiguous float64 tensor on the solver's device."""
        if isinstance(kappa, np.ndarray):
            self.hierarchy.gen_diffusion_hierarchy(kappa, self.averaging, matrix_free_min_rows=self.matrix_free_min_rows)
            self.last_generate = "host"
        else:
            torch.cuda.current_stream(self.device).synchronize()    # kappa is complete before the handle's stream reads it
            if self._generated:
                self.hierarchy.refresh_diffusion_hierarchy(kappa.data_ptr(), self.averaging)
                self.last_generate = "refresh"
            else:
                self.hierarchy.gen_diffusion_hierarchy(kappa.data_ptr(), self.averaging,
                                                       matrix_free_min_rows=self.matrix_free_min_rows)
                self.last_generate = "device"
        self._generated = True
        self._generation += 1
        return self._generation

    def _device_vector(self, x: torch.Tensor, what: str) -> torch.Tensor:
        n = self.hierarchy.n_dofs(self.top)
        if x.dtype != torch.float64 or x.device != self.device or x.numel() != n:
            raise ValueError(f"{what} must hold {n} float64 on {self.device} (got {x.numel()} {x.dtype} on {x.device})")
        return x.detach().contiguous()

    def _pcg(self, rhs: torch.Tensor, which: str) -> torch.Tensor:
        """A x = rhs from zero, or from the last solution of this kind (warm_start); rhs and x by pointer."""
        h = self.hierarchy
        torch.cuda.current_stream(self.device).synchronize()        # rhs is complete before the handle's stream reads it
        h.set_vector_device(self.top, "f", rhs.data_ptr())
        x0 = self._warm.get(which) if self.warm_start else None
        if x0 is not None:
            h.set_vector_device(self.top, "v", x0.data_ptr())
        else:
            h.zero_vector(self.top, "v")
        hist = h.pcg(rtol=self.rtol, max_iter=self.max_iter, level=self.top)
        self.last_iterations[which] = len(hist)
        self.last_residual[which] = float(hist[-1]) / h.norm2(self.top, "f") if len(hist) else None
        if len(hist) >= self.max_iter and not hist[-1] <= self.rtol * h.norm2(self.top, "f"):
            raise NotConverged(f"the {which} solve reached max_iter = {self.max_iter} at ||r|| = {hist[-1]:.3e} "
                               f"(rtol {self.rtol:g}): no gradient is returned")
        x = torch.empty_like(rhs)
        h.get_vector_device(self.top, "v", x.data_ptr())
        if self.warm_start:
            self._warm[which] = x.clone()
        return x


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kappa, f, solver):
        if kappa.dtype != torch.float64 or kappa.numel() != solver.N ** 3:
            raise ValueError(f"kappa must hold {solver.N ** 3} float64")
        if kappa.device == solver.device:       # no .cpu(): a device copy that the caller's later updates do not reach feeds the library
            kappa_kept = kappa.detach().reshape(-1).clone()
        else:
            kappa_kept = np.ascontiguousarray(kappa.detach().cpu().numpy().reshape(-1))
        rhs = solver._device_vector(f, "f")
        ctx.generation = solver._generate(kappa_kept)
        u = solver._pcg(rhs, "forward")
        ctx.solver, ctx.kappa_kept = solver, kappa_kept
        ctx.kappa_like = (kappa.shape, kappa.device)
        ctx.save_for_backward(u)
        return u.view(f.shape)

    @staticmethod
    def backward(ctx, grad_u):
        solver = ctx.solver
        (u,) = ctx.saved_tensors
        if ctx.generation != solver._generation:        # another kappa has been solved since: this one's operator again
            ctx.generation = solver._generate(ctx.kappa_kept)
        lam = solver._pcg(solver._device_vector(grad_u, "grad_u"), "adjoint")
        grad_kappa = None
        if ctx.needs_input_grad[0]:
            shape, device = ctx.kappa_like
            out = torch.empty(solver.N ** 3, dtype=torch.float64, device=solver.device)
            torch.cuda.current_stream(solver.device).synchronize()
            solver.hierarchy.diffusion_dkappa(solver.top, lam.data_ptr(), u.data_ptr(), out.data_ptr())
            grad_kappa = out.neg_().view(shape).to(device)
        grad_f = lam.view(grad_u.shape) if ctx.needs_input_grad[1] else None
        return grad_kappa, grad_f, None
