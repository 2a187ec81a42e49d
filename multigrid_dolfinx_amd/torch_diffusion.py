"""Differentiable solves of -div(kappa grad u) = f, u = g on the boundary, on the device:
`DiffusionSolver.solve(kappa, f, g) -> u` with gradients with respect to kappa, f and g by the adjoint method.

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
from .poisson import ALL_FACES, _one_face, dirichlet_mask, face_set

__all__ = ["DiffusionSolver", "LocatedPoints", "NotConverged"]


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

    Contract: without `g`, `f` is the FULL right-hand side in lexicographic node order, boundary entries included.  Boundary
    rows are identity rows, so u_b = f_b, and interior rows have no boundary column.  With Dirichlet data `g` ((N + 1)^3
    float64 on the solver's device; only its boundary entries are read, its interior gets a zero gradient) the right-hand
    side is where(boundary, g, f - T(kappa, g_B; interior, all)): the lifted load -A_IB(kappa) g_B that
    `mg_gen_diffusion_level` folds into its own right-hand side, g_B = g on the boundary and 0 inside, and u_b = g_b.  The
    lift depends on kappa, and it is written with the autograd functions below (T and D with a node set per side,
    `mg_diffusion_apply_dkappa_ex` / `mg_diffusion_dkappa_ex`), so the gradients with respect to kappa, f and g and their
    second derivatives come out of `torch.autograd` with no solve beyond those counted below: grad_kappa =
    -D(lambda~, u; interior, all), grad_g = (grad_u - A^ lambda~) on the boundary.  The boundary entries of `f` do not
    count then.  A kappa on the CPU goes to the device for the lift by a differentiable `.to`.

    `kappa`: N^3 positive float64, cell (ci, cj, ck) at (ck * N + cj) * N + ci, any shape, on the CPU (uploaded, every
    level regenerated) or on the solver's device (it stays there: the first solve generates, later ones refresh in
    place; `last_generate` says which of "host", "device", "refresh" the last one was).  `f`, `u`: (N + 1)^3 float64 on
    the handle's device.  `averaging` and `matrix_free_min_rows` as in `DeviceHierarchy.gen_diffusion_hierarchy`; `set_params` are those of
    `DeviceHierarchy.set_params` (defaults: V(2,2), omega 2/3, Jacobi; the restriction is always the P1 transpose).

    backward: one more `mg_pcg` on the same hierarchy (A is symmetric), A lambda = grad_u; then grad_f = lambda and
    grad_kappa = -mg_diffusion_dkappa(lambda, u).  A solve that reaches `max_iter` raises `NotConverged`.

    Higher derivatives: the backward pass is itself written with S(kappa, f) = A^-1 f, D(a, b) = mg_diffusion_dkappa and
    T(w, x) = mg_diffusion_apply_dkappa = (dA/dkappa . w) x, whose derivatives close on each other (S: lambda = S(kappa, g),
    f_bar = lambda, kappa_bar = -D(lambda, u); D with cotangent w: a_bar = T(w, b), b_bar = T(w, a); T with cotangent y:
    w_bar = D(y, x), x_bar = T(w, y)), so `torch.autograd.grad(..., create_graph=True)` through `solve` can be differentiated
    again: a Hessian-vector product of J(u(kappa)) is four solves on one generation (`n_solves` counts them).  Solves started
    from a backward pass count as "adjoint" in `last_iterations`, `last_residual` and `NotConverged`; while a backward pass
    records gradients they start from zero and leave the kept warm-start solutions alone.  Without `create_graph` the
    backward pass is the one solve and one sensitivity kernel described above.  `tangent` is the forward-mode derivative.

    `warm_start=True` keeps the last forward and the last adjoint solution and starts the next solve of each kind from
    them instead of from zero (kappa that moves a little between solves).  The stopping test is relative to the
    right-hand side either way, so the gradients are those of the converged solve.

    `dirichlet_faces` (None: all six; names "x-" .. "z+" or the integer of `poisson.face_set`): only those faces carry the
    Dirichlet condition (`DeviceHierarchy.set_diffusion_faces`), the others are no-flux faces whose nodes are free nodes.
    Everything above then reads with "boundary" = the Dirichlet nodes and "interior" = the free nodes: `g` is read on the
    Dirichlet nodes only and gets a zero gradient elsewhere, and `f` on a free boundary node is a genuine load entry -- where
    prescribed flux data, the integral of q phi_i over the face, goes.  The derivative algebra and the solve counts are
    the same.

    `sigma` (`solve`, `tangent`): N^3 float64 >= 0 in kappa's cell order, on the solver's device or the CPU, a
    differentiable input like kappa.  The operator is then A(kappa) + R(sigma) with the lumped reaction diagonal of
    `poisson.reaction_diag` (`DeviceHierarchy.set_diffusion_reaction`): absorption, a screened Poisson problem, or with
    sigma = 1 / dt one implicit Euler step of du/dt - div(kappa grad u) = f, whose right-hand side is
    b + `reaction_apply`(sigma, u_old).  grad_sigma = -D_sigma(lambda, u) comes from the adjoint solve that gives grad_kappa;
    the lift of `g` does not involve sigma (R is diagonal).  D_sigma and T_sigma close under differentiation as D and T do,
    so `create_graph=True` gives the kappa-kappa, kappa-sigma and sigma-sigma blocks of a Hessian-vector product, in the same
    number of solves.  The operator of a solve keeps sigma with kappa; going from solves with sigma to solves without, or
    the reverse, generates the hierarchy again instead of refreshing it (`last_generate`).

    `solve(..., same_operator=True)` solves on the operator of the last `solve` without touching the hierarchy, as `tangent`
    does: the caller asserts that kappa, sigma and the Robin fields hold the values of that solve (the steps of a time march
    with a constant dt).  Gradients with respect to them still flow.  `n_generations` counts the generations and refreshes.

    `dirichlet_faces="insulated"` (`poisson.INSULATED`): no Dirichlet node at all (`DeviceHierarchy.set_diffusion_insulated`;
    DESIGN.md, "Insulated bodies").  `g` must be None -- anything else raises ValueError -- and `robin` may name any of the six
    faces.  With `sigma` or at least one Robin field the operator is regular and everything is as on any face set (an
    implicit heat step of an insulated body, convective cooling all round); a field that is zero everywhere is the caller's
    mistake and ends in `NotConverged`.  With neither the operator is singular (its null space is the constants) and
    `solve` returns u = S f, S = Q A^+ Q^T with Q = I - 1 w^T / s, w the lumped mass of rho = 1 and s = w.1: A u = f - w (1.f) / s
    and w.u = 0 -- a uniform source density is taken off the load, and u_h has integral zero.  S is symmetric and dS = -S dA S,
    so the adjoint solve is the same projected solve, grad_f = lambda, grad_kappa = -D(lambda, u): first and second
    derivatives and `tangent` are as everywhere.  `solve_many` and `eigenpairs` raise in the singular case and work in the
    regular one; going between solves with and without sigma or alpha regenerates the hierarchy, as on any face set.

    `robin` (`solve`, `tangent`): a mapping of faces outside `dirichlet_faces` (names "x-" .. "z+" or bits) to N^2 float64
    alpha >= 0, one per boundary face-cell (face-cell (ca, cb) at cb * N + ca, (a, b) the in-plane axes in ascending order),
    on the solver's device or the CPU, each a differentiable input.  Those faces carry kappa du/dn + alpha (u - u_ext) = 0
    instead of the no-flux condition: the operator gains the lumped boundary diagonal B(alpha) of `poisson.robin_diag`
    (`DeviceHierarchy.set_diffusion_robin`), and the ambient load alpha u_ext int phi_i is `robin_apply`(face, alpha, u_ext),
    which the caller adds to `f`.  grad_alpha_F = -D_alpha,F(lambda, u) comes from the one adjoint solve; the lift of `g`
    involves no alpha.  D_alpha and T_alpha close under differentiation, so `create_graph=True` gives the kappa-alpha,
    alpha-kappa and alpha-alpha blocks of a Hessian-vector product in the same number of solves.  The operator of a solve
    keeps the fields beside kappa and sigma; changing WHICH faces hold a field generates the hierarchy again instead of
    refreshing it (`last_generate`).

    `solve_many(kappa, F, g=None, sigma=None, same_operator=False, robin=None) -> U` solves one operator for the B >= 1
    right-hand sides F[0], F[1], ... ((N + 1)^3 float64 each, B leading rows, on the solver's device; `g`: None, one field
    shared by all lanes, or B fields) in ONE generation and ONE batched solve (`DeviceHierarchy.pcg_batch`): on matrix-free
    levels the march rebuilds each row from kappa once for several lanes.  U[b] has the bits of `solve(kappa, F[b], ...)`.  The
    backward pass is one more batched solve with the B cotangents, then grad_F = Lambda, grad_kappa = -(D(lambda_0, u_0) +
    D(lambda_1, u_1) + ...) summed in ascending lane order (grad_sigma and grad_alpha alike), grad_g per lane as in `solve`
    and summed over the lanes where g is shared.  It is written with the autograd functions themselves, so `create_graph=True`
    works and a Hessian-vector product of a sum over B sources is four batched solves.  `n_solves` grows by B per batched
    solve and `n_batched_solves` by 1; `last_iterations[kind]` is the largest lane count and `last_lane_iterations[kind]`
    holds them all; if any lane reaches `max_iter`, `NotConverged` names the lanes.  `warm_start` keeps the last batched
    solution of each kind and reuses it when B is the same.  `tangent` is not batched.

    `gradient(u, weight=None)` and `flux(kappa, u)` = -`gradient`(u, kappa) give the cell gradient and the flux q = -kappa grad u
    of a nodal field, (3, N, N, N) indexed [d, ck, cj, ci]: per cell the mean of grad u_h over its six simplices
    (`mg_diffusion_cell_gradient`), differentiable in both arguments to second order through F, its transpose and its
    contraction (`_CellGrad`, `_CellGradT`, `_CellGradDot`), which close under differentiation as D and T do.  They read the top
    level's grid and nothing else: they work before the first solve and leave the hierarchy and the counters alone.

    `sample(u, points)`, `point_load(points, w)` and `sample_gradient(u, points)` put observations and sources anywhere in the
    unit cube: the P1 interpolant S on the located Kuhn simplex, its transpose S^T (the consistent point load) and the
    simplex gradient G (`mg_diffusion_point_sample`, `_load`, `_gradient`, `_gradient_t`), differentiable to second order in
    the fields and in the positions (`_PointSample`, `_PointLoad`, `_PointGrad`, `_PointGradT`, which close under
    differentiation).  The position derivative is the one inside the located simplex.  They too read the top level's grid
    alone."""

    def __init__(self, N: int, n_levels: int, averaging: str = "arithmetic", matrix_free_min_rows: Optional[int] = None,
                 rtol: float = 1e-10, max_iter: int = 200, device: int = 0, warm_start: bool = False, dirichlet_faces=None,
                 **set_params):
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
        self.dirichlet_faces = face_set(dirichlet_faces)
        self.insulated = self.dirichlet_faces == 0      # (`face_set`: only "insulated" gives 0)
        if self.insulated:
            self.hierarchy.set_diffusion_insulated()
        elif self.dirichlet_faces != ALL_FACES:
            self.hierarchy.set_diffusion_faces(self.dirichlet_faces)
        self._generation = 0
        self._generated = False         # a hierarchy call has generated the levels: a device kappa can refresh them
        self._generated_react = False   # ... with a reaction field: a refresh needs the same state
        self._generated_robin = ()      # ... and with Robin fields on these faces (bits)
        self.last_generate = None       # "host" / "device" / "refresh": how the last kappa reached the hierarchy
        self.warm_start = bool(warm_start)
        self._warm = {}                 # "forward" / "adjoint": the last solution of that kind (warm_start)
        self._last_operator = None      # the _Operator of the last `solve`: what `tangent` solves again on
        self._grid_only = False         # `reaction_apply` before the first solve has made the top level a grid-only level
        self._boundary = None           # the mask of the Dirichlet nodes on the device (solves with g)
        self.n_solves = 0               # mg_pcg calls so far: what a product costs (a Hessian-vector product: four)
        self.last_iterations = {}       # "forward" / "adjoint" / "tangent": iterations of the last solve of that kind
        self.last_residual = {}         # ... and ||r|| / ||rhs|| of mg_pcg's recursion where it stopped (None: no iteration was needed)
        self.n_batched_solves = 0       # mg_pcg_batch calls so far (`solve_many`): each adds its lanes to n_solves
        self.last_lane_iterations = {}  # ... the iterations of every lane of the last batched solve of that kind
        self._warm_many = {}            # ... its solution (warm_start; reused when the next one has as many lanes)

    def close(self):
        if self.n_batched_solves and self.hierarchy._h:
            self.hierarchy.release_batch()
        self.hierarchy.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def n_generations(self) -> int:
        """Hierarchy generations and refreshes so far: what a march with `same_operator=True` saves."""
        return self._generation

    def _robin_inputs(self, robin, what: str = "robin"):
        """(bits, tensors) of a mapping of faces to N^2 float64 tensors, in ascending bit order; ((), ()) for None."""
        if not robin:
            return (), ()
        fields = {}
        for face, alpha in robin.items():
            bit = _one_face(face)
            if bit in fields:
                raise ValueError(f"{what}: face {bit} is given twice")
            if bit & self.dirichlet_faces:
                raise ValueError(f"{what}: face {bit} is a Dirichlet face of this solver (dirichlet_faces = {self.dirichlet_faces})")
            if alpha.dtype != torch.float64 or alpha.numel() != self.N ** 2:
                raise ValueError(f"{what}: the field of face {bit} must hold {self.N ** 2} float64")
            fields[bit] = alpha
        bits = tuple(sorted(fields))
        return bits, tuple(fields[b] for b in bits)

    def _no_dirichlet_data(self, g, what: str = "g"):
        if self.insulated and g is not None:
            raise ValueError(f"the insulated solver (dirichlet_faces=\"insulated\") has no Dirichlet node: {what} must be None")

    def _singular(self, sigma, bits) -> bool:
        """The insulated solver with neither a reaction nor a Robin field: the operator is singular and `solve` projects."""
        return self.insulated and sigma is None and not bits

    def _operator_to_reuse(self, same_operator: bool, sigma, bits) -> Optional["_Operator"]:
        """None, or with `same_operator` the operator of the last solve, which must have had what this one has."""
        if not same_operator:
            return None
        op = self._last_operator
        if op is None:
            raise ValueError("same_operator=True reuses the operator of the last solve: there has been none")
        if (sigma is None) != (op.sigma_kept is None):
            raise ValueError("same_operator=True: the last solve had " + ("no" if sigma is not None else "a") + " sigma")
        if bits != tuple(sorted(op.robin_kept)):
            raise ValueError(f"same_operator=True: the last solve had Robin fields on the faces {sorted(op.robin_kept)}")
        return op

    def _lifted(self, kv: torch.Tensor, gv: torch.Tensor, fv: torch.Tensor) -> torch.Tensor:
        """where(boundary, g, f - T(kappa, g_B; interior, all)) for one g and one f, or several rows of them."""
        boundary = self._boundary_mask()
        g_b = torch.where(boundary, gv, torch.zeros_like(gv))
        return torch.where(boundary, gv, fv - _T.apply(kv, g_b, self, _kappa_field("interior", "all")))

    def solve(self, kappa: torch.Tensor, f: torch.Tensor, g: Optional[torch.Tensor] = None,
              sigma: Optional[torch.Tensor] = None, same_operator: bool = False, robin=None) -> torch.Tensor:
        self._no_dirichlet_data(g)
        bits, alphas = self._robin_inputs(robin)
        op = self._operator_to_reuse(same_operator, sigma, bits)
        if g is None:
            return _Solve.apply(kappa, f, self, op, "forward", True, False, sigma, bits, *alphas)
        gv, fv = self._same_size(g, "g").reshape(-1), self._same_size(f, "f").reshape(-1)
        if op is None:
            op = self._put_operator(kappa, sigma, dict(zip(bits, alphas)))  # first: the lift runs on the level's grid, which the first generation sets
        rhs = self._lifted(kappa.reshape(-1).to(self.device), gv, fv)
        return _Solve.apply(kappa, rhs.view(f.shape), self, op, "forward", True, False, sigma, bits, *alphas)

    def solve_many(self, kappa: torch.Tensor, F: torch.Tensor, g: Optional[torch.Tensor] = None,
                   sigma: Optional[torch.Tensor] = None, same_operator: bool = False, robin=None) -> torch.Tensor:
        """`solve` for the B right-hand sides F[0] .. F[B - 1] on one operator: one generation, one batched solve forward and
        one backward (see the class)."""
        n = self.hierarchy.n_dofs(self.top)
        if F.dtype != torch.float64 or F.device != self.device or F.dim() < 2 or F.shape[0] < 1 or F[0].numel() != n:
            raise ValueError(f"F must hold B >= 1 leading rows of {n} float64 on {self.device} (got {tuple(F.shape)} {F.dtype} on {F.device})")
        B = F.shape[0]
        self._no_dirichlet_data(g)
        bits, alphas = self._robin_inputs(robin)
        if self._singular(sigma, bits):
            raise ValueError("solve_many: the insulated solver with neither sigma nor robin has a singular operator, and batched "
                             "solves have no projected form: call solve per right-hand side")
        op = self._operator_to_reuse(same_operator, sigma, bits)
        if g is None:
            return _Solve.apply(kappa, F, self, op, "forward", True, True, sigma, bits, *alphas)
        if g.dtype != torch.float64 or g.device != self.device or g.numel() not in (n, B * n) or (g.numel() == B * n and B > 1 and g.shape[0] != B):
            raise ValueError(f"g must hold {n} float64 (shared by all lanes) or {B} leading rows of them on {self.device}")
        shared = g.numel() == n and not (B == 1 and g.dim() == F.dim())
        Fv = F.reshape(B, n)
        if op is None:
            op = self._put_operator(kappa, sigma, dict(zip(bits, alphas)))  # first: the lift runs on the level's grid, which the first generation sets
        kv = kappa.reshape(-1).to(self.device)
        if shared:      # one lift for all lanes: autograd sums its lanes' contributions
            rhs = self._lifted(kv, g.reshape(-1), Fv)
        else:
            gv = g.reshape(B, n)
            rhs = torch.stack([self._lifted(kv, gv[b], Fv[b]) for b in range(B)])
        return _Solve.apply(kappa, rhs.view(F.shape), self, op, "forward", True, True, sigma, bits, *alphas)

    def eigenpairs(self, kappa: torch.Tensor, k: int, *, rho: Optional[torch.Tensor] = None, sigma: Optional[torch.Tensor] = None,
                   robin=None, block: Optional[int] = None, x0: Optional[torch.Tensor] = None, rtol: float = 1e-8,
                   max_iter: int = 100, same_operator: bool = False):
        """The `k` smallest eigenpairs of K u = lambda M(rho) u, K = A(kappa) + R(sigma) + B(alpha) on the free nodes and
        M(rho) = R(rho) the lumped mass (rho: N^3 float64 > 0 on the solver's device; None: 1): the decay rates and shapes of
        rho u_t = div(kappa grad u) - sigma u under the solver's boundary conditions, by `DeviceHierarchy.eigs` (LOBPCG, one
        V-cycle per vector and iteration; `block` vectors, default min(MG_EIGS_MAX, k + 2)).  The operator is put in place as
        `solve` puts it; `same_operator=True` reuses the generation of the last solve.  Returns `(lam, U)`: `lam` of shape
        (k,), ascending; `U` of shape (k, N + 1, N + 1, N + 1), detached, u^T M u = 1, exactly 0 on the Dirichlet nodes, each
        vector's sign chosen so that its entry of largest magnitude is positive (the lowest index on ties).  `x0`: a previous
        `U`, or a (block, ...) tensor, as a warm start (rows it lacks are filled with seeded noise).  Raises `NotConverged`
        when one of the first k residuals ||K u - lam M u|| / (lam ||M u||) is above `rtol` after `max_iter` iterations.

        `lam` is differentiable to FIRST order in kappa, sigma, every alpha and rho: d lam_j = D(u_j, u_j) . dkappa +
        D_sigma(u_j, u_j) . dsigma + D_F(u_j, u_j) . dalpha_F - lam_j D_sigma(u_j, u_j) . drho, one sensitivity launch per
        vector and field and no solve.  That gradient is defined for a SIMPLE eigenvalue and for the SUM over a whole cluster
        of equal eigenvalues; it is NOT defined for one member of a degenerate cluster, whose vector is an arbitrary element
        of the eigenspace (the closed-form cube's (1,1,2) triple, say): differentiate the cluster's sum, or break the
        symmetry.  Second derivatives need eigenvector derivatives and are not provided: differentiating twice raises."""
        bits, alphas = self._robin_inputs(robin)
        if self._singular(sigma, bits):
            raise ValueError("eigenpairs: the insulated solver with neither sigma nor robin has a singular operator (its smallest "
                             "eigenvalue is 0, the constants): eigenpairs are not provided for it")
        op = self._operator_to_reuse(same_operator, sigma, bits)
        return _Eigs.apply(kappa, self, op, int(k), block, x0, float(rtol), int(max_iter), rho, sigma, bits, *alphas)

    def _top_level_grid(self):
        """The kernels of `robin_apply`, `reaction_apply` and `gradient` read the top level's grid and nothing else: before the
        first solve has generated the level, it becomes a grid-only level."""
        if not self._generated and not self._grid_only:
            self.hierarchy.set_level_grid(self.top)
            self._grid_only = True

    def robin_apply(self, face, w: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """T_alpha,F(w, x) = b_F(w) x on the free nodes of `face`, 0 on every other node (`mg_diffusion_apply_drobin`),
        differentiable in both: with w = alpha and x = u_ext the ambient load of a Robin face.  `w`: N^2 float64 of any sign,
        on the solver's device or the CPU; `x`: (N + 1)^3 float64 on the solver's device."""
        self._top_level_grid()
        return _T.apply(w.reshape(-1).to(self.device), x.reshape(-1), self, _alpha_field(_one_face(face))).view(x.shape)

    def reaction_apply(self, w: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """T_sigma(w, x) = R(w) x on the free nodes, 0 on the Dirichlet nodes (`mg_diffusion_apply_dsigma`), differentiable in
        both: with w = 1 / dt in every cell the M u / dt of an implicit Euler step.  `w`: N^3 float64 of any sign, on the
        solver's device or the CPU; `x`: (N + 1)^3 float64 on the solver's device."""
        self._top_level_grid()
        return _T.apply(w.reshape(-1).to(self.device), x.reshape(-1), self, _SIGMA_FIELD).view(x.shape)

    def gradient(self, u: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cell gradient of the nodal field `u`, (3, N, N, N) indexed [d, ck, cj, ci]: per cell the mean of grad u_h over
        its six simplices (`mg_diffusion_cell_gradient`), times `weight` (N^3 float64 of any sign in kappa's cell order, on the
        solver's device or the CPU) where one is given.  Differentiable in both to second order.  `u`: (N + 1)^3 float64 on
        the solver's device, read as it is (Dirichlet values included).  Works before the first solve and leaves the
        hierarchy alone: `n_generations` and `n_solves` do not move."""
        self._top_level_grid()
        w = None if weight is None else weight.reshape(-1).to(self.device)
        return _CellGrad.apply(w, self._same_size(u, "u").reshape(-1), self).view(3, self.N, self.N, self.N)

    def flux(self, kappa: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        """q = -kappa grad u per cell, (3, N, N, N): the exact cell average of the flux of the P1 field, -`gradient`(u, kappa).
        With u a pressure it is the Darcy velocity, with u a temperature the heat flux."""
        return -self.gradient(u, weight=kappa)

    def sample(self, u: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
        """u_h at the points, (M,): the P1 interpolant on the Kuhn simplices the operator is built on
        (`mg_diffusion_point_sample`), not a trilinear one.  `u`: (N + 1)^3 float64 on the solver's device, read as it is
        (Dirichlet values included); `points`: (M, 3) float64 rows (x, y, z) in [0, 1]^3 on the solver's device.
        Differentiable to second order in `u` and in `points`.  The position derivative is the derivative inside the
        located simplex, grad u_h there (`sample_gradient`): u_h is piecewise linear and kinks on simplex faces, so at a point
        on a face it is the one-sided derivative of the simplex that `poisson.diffusion_point_locate` picks.  Works before
        the first solve and leaves the hierarchy alone: `n_generations` and `n_solves` do not move.  `points` may be the
        `LocatedPoints` of `locate` instead, here and in `point_load` and `sample_gradient`: the same bits without the
        per-call check, allocations and sort."""
        self._top_level_grid()
        if isinstance(points, LocatedPoints):
            return self.sample_many(self._same_size(u, "u").reshape(1, -1), points)[0]
        return _PointSample.apply(self._same_size(u, "u").reshape(-1), points, self)

    def point_load(self, points: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """The consistent load of point sources of strength `w` (M float64 on the solver's device) at `points` ((M, 3), as in
        `sample`): f_i = sum_m w_m phi_i(x_m), the transpose of `sample` (`mg_diffusion_point_load`), (N + 1, N + 1, N + 1)
        indexed [k, j, i].  Each node sums its points in ascending point index: the same bits on every call.  Differentiable
        to second order in `w` and in `points`; the position derivative is the one inside the located simplex, as in `sample`.
        A point in a boundary cell puts load on Dirichlet nodes.  `solve(kappa, f)` without `g` reads the entries of `f` on
        Dirichlet nodes as boundary values, so a point-source solve is `solve(kappa, point_load(X, w), g=zeros)`: with `g`
        given, `f` on Dirichlet nodes does not count.  Works before the first solve and leaves the hierarchy alone."""
        self._top_level_grid()
        n1 = self.N + 1
        if isinstance(points, LocatedPoints):
            return self.point_load_many(points, w.reshape(1, -1))[0]
        return _PointLoad.apply(w.reshape(-1), points, self).view(n1, n1, n1)

    def sample_gradient(self, u: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
        """grad u_h at the points, (M, 3) with components (x, y, z): the gradient of the simplex that holds each point
        (`mg_diffusion_point_gradient`).  `u` and `points` as in `sample`.  Differentiable to second order in `u`; piecewise
        constant in `points`, which get no derivative: u_h is piecewise linear and its gradient jumps on simplex faces.
        Works before the first solve and leaves the hierarchy alone."""
        self._top_level_grid()
        if isinstance(points, LocatedPoints):
            return self.sample_gradient_many(self._same_size(u, "u").reshape(1, -1), points)[0]
        return _PointGrad.apply(self._same_size(u, "u").reshape(-1), points, self)

    def locate(self, points: torch.Tensor) -> "LocatedPoints":
        """The points ((M, 3) float64 rows (x, y, z) in [0, 1]^3 on the solver's device) checked, located and sorted once on the
        top level (`mg_points_create`): a `LocatedPoints`, which `sample`, `point_load` and `sample_gradient` take in place of
        the tensor -- same bits, without the per-call check, allocations and sort -- and which the `_many` forms need.  The
        set is a snapshot: after an in-place change of `points` every use raises (locate again).  Works before the first
        solve and moves neither `n_generations` nor `n_solves`."""
        self._top_level_grid()
        return LocatedPoints(self, points)

    def _located(self, P: "LocatedPoints") -> "LocatedPoints":
        if not isinstance(P, LocatedPoints) or P.solver is not self:
            raise TypeError("the batched point functions take the LocatedPoints of this solver's locate()")
        return P.fresh()

    def sample_many(self, U: torch.Tensor, P: "LocatedPoints") -> torch.Tensor:
        """`sample` of the B fields U[0] .. U[B - 1] ((B, ...) with (N + 1)^3 float64 each) at a located set, (B, M): one
        sequence of launch groups forward and one backward for all lanes (`mg_points_sample`), every lane with the bits of
        `sample(U[b], X)`.  Differentiable to second order in U and, where the tensor P was located from requires grad, in the
        positions: that tensor receives sum_b y_b[:, None] * grad u_b,h at the points."""
        P = self._located(P)
        n = self.hierarchy.n_dofs(self.top)
        return _SetSample.apply(U.reshape(U.shape[0], -1) if U.dim() >= 2 and U[0].numel() == n else U, P.source, P)

    def point_load_many(self, P: "LocatedPoints", W: torch.Tensor) -> torch.Tensor:
        """`point_load` of the B weight vectors W[0] .. W[B - 1] ((B, M)) at a located set, (B, N + 1, N + 1, N + 1)
        (`mg_points_load`), every lane with the bits of `point_load(X, W[b])`.  Differentiable as `sample_many`."""
        P = self._located(P)
        n1 = self.N + 1
        return _SetLoad.apply(W, P.source, P).view(-1, n1, n1, n1)

    def sample_gradient_many(self, U: torch.Tensor, P: "LocatedPoints") -> torch.Tensor:
        """`sample_gradient` of the B fields of U at a located set, (B, M, 3) (`mg_points_gradient`), every lane with the bits of
        `sample_gradient(U[b], X)`.  Differentiable to second order in U; the positions get no derivative."""
        P = self._located(P)
        n = self.hierarchy.n_dofs(self.top)
        return _SetGrad.apply(U.reshape(U.shape[0], -1) if U.dim() >= 2 and U[0].numel() == n else U, P.source, P)

    def tangent(self, kappa: torch.Tensor, f: torch.Tensor, dkappa: torch.Tensor, df: Optional[torch.Tensor] = None,
                g: Optional[torch.Tensor] = None, dg: Optional[torch.Tensor] = None, sigma: Optional[torch.Tensor] = None,
                dsigma: Optional[torch.Tensor] = None, robin=None, drobin=None):
        """(u, du): u = A(kappa)^-1 f and its derivative in the direction (dkappa, df),
        du = A^-1 (df - (dA/dkappa . dkappa) u), on the same operator: two solves, one generation.  The cheap derivative
        when kappa depends on a few parameters.  `kappa` as in `solve`; `f`, `dkappa` (N^3 float64, any sign) and `df`
        (None: zero) on the solver's device.  The second solve counts as "tangent" in `last_iterations`.
        With Dirichlet data `g` as in `solve` and its direction `dg` (None: zero; boundary entries only): the interior rows of
        the second right-hand side are df - T(dkappa, u; interior, all) - T(kappa, dg_B; interior, all), u with its boundary
        values g, and du = dg on the boundary.
        With `sigma` as in `solve` and its direction `dsigma` (None: zero; N^3 float64 of any sign on the solver's device) the
        operator is A(kappa) + R(sigma) and the second right-hand side loses T_sigma(dsigma, u) on the free rows.
        With `robin` as in `solve` and its directions `drobin` (a mapping of some of those faces to N^2 float64 of any sign on
        the solver's device) it loses T_alpha,F(drobin[F], u) too."""
        self._no_dirichlet_data(g)
        if g is None and dg is not None:
            raise ValueError("dg is the direction of g: it needs g")
        if sigma is None and dsigma is not None:
            raise ValueError("dsigma is the direction of sigma: it needs sigma")
        bits, alphas = self._robin_inputs(robin)
        dbits, dalphas = self._robin_inputs(drobin, "drobin")
        if set(dbits) - set(bits):
            raise ValueError("drobin holds the directions of robin: it needs a field on each of its faces")
        u = self.solve(kappa, f, g, sigma, robin=robin)
        uv = u.reshape(-1)
        rhs = _T.apply(dkappa.reshape(-1), uv, self, _kappa_field("interior", "interior" if g is None else "all")).neg()
        if df is not None:
            rhs = self._same_size(df, "df").reshape(-1) + rhs
        on_boundary = torch.zeros_like(rhs)
        if dg is not None:
            on_boundary = self._same_size(dg, "dg").reshape(-1)
            dg_b = torch.where(self._boundary_mask(), on_boundary, torch.zeros_like(on_boundary))
            rhs = rhs - _T.apply(kappa.detach().reshape(-1).to(self.device), dg_b, self, _kappa_field("interior", "all"))
        if dsigma is not None:
            rhs = rhs - _T.apply(dsigma.reshape(-1), uv, self, _SIGMA_FIELD)
        for bit, dalpha in zip(dbits, dalphas):
            rhs = rhs - _T.apply(dalpha.reshape(-1), uv, self, _alpha_field(bit))
        if g is not None:
            rhs = torch.where(self._boundary_mask(), on_boundary, rhs)
        du = _Solve.apply(kappa, rhs, self, self._last_operator, "tangent", True, False, sigma, bits, *alphas)
        return u, du.view(u.shape)

    # ---- what the autograd function calls --------------------------------------------------------------------
    def _as_library_takes(self, x):
        """A field as the hierarchy's calls take it: None and a host array as they are, a tensor on the solver's device as its
        address, once the current stream has finished writing it and the handle's stream may read it."""
        if x is None or isinstance(x, np.ndarray):
            return x
        torch.cuda.current_stream(self.device).synchronize()
        return x.data_ptr()

    def _generate(self, kappa, sigma=None, robin=None) -> int:
        """`kappa`: a host array (today's path) or a contiguous float64 tensor on the solver's device; `sigma`: None, or the
        reaction field as one of the two; `robin`: None, or the Robin fields by face bit, each as one of the two.  The
        handle's fields are set (or cleared) first: the generating calls read them."""
        robin = robin or {}
        for bit in sorted(set(robin) | set(self._generated_robin)):
            self.hierarchy.set_diffusion_robin(bit, self._as_library_takes(robin.get(bit)), N=self.N)
        if tuple(sorted(robin)) != self._generated_robin:   # levels with fields on other faces do not refresh into each other
            self._generated = False
        self._generated_robin = tuple(sorted(robin))
        react = sigma is not None
        if react or self._generated_react:
            self.hierarchy.set_diffusion_reaction(self._as_library_takes(sigma), N=self.N)
        if react != self._generated_react:      # levels with and without a reaction diagonal do not refresh into each other
            self._generated = False
        self._generated_react = react
        self._grid_only = False
        on_host = isinstance(kappa, np.ndarray)
        if self._generated and not on_host:
            self.hierarchy.refresh_diffusion_hierarchy(self._as_library_takes(kappa), self.averaging)
            self.last_generate = "refresh"
        else:
            self.hierarchy.gen_diffusion_hierarchy(self._as_library_takes(kappa), self.averaging,
                                                   matrix_free_min_rows=self.matrix_free_min_rows)
            self.last_generate = "host" if on_host else "device"
        self._generated = True
        self._generation += 1
        return self._generation

    def _boundary_mask(self) -> torch.Tensor:
        """True on the Dirichlet nodes -- the boundary nodes, or those on `dirichlet_faces` -- (N + 1)^3 lexicographic, on the
        solver's device (built by the first solve with g)."""
        if self._boundary is None:
            self._boundary = torch.from_numpy(dirichlet_mask(self.N, self.dirichlet_faces)).to(self.device)
        return self._boundary

    def _put_operator(self, kappa: torch.Tensor, sigma: Optional[torch.Tensor] = None, robin=None) -> "_Operator":
        """Puts the caller's kappa (and sigma, and the Robin fields by face bit) into the hierarchy: the operator of a
        `solve` and of what derives from it."""
        if kappa.dtype != torch.float64 or kappa.numel() != self.N ** 3:
            raise ValueError(f"kappa must hold {self.N ** 3} float64")
        if sigma is not None and (sigma.dtype != torch.float64 or sigma.numel() != self.N ** 3):
            raise ValueError(f"sigma must hold {self.N ** 3} float64")

        def kept(x):
            if x is None:
                return None
            if x.device == self.device:   # no .cpu(): a device copy that the caller's later updates do not reach feeds the library
                return x.detach().reshape(-1).clone(memory_format=torch.contiguous_format)
            return np.ascontiguousarray(x.detach().cpu().numpy().reshape(-1))

        kappa_kept, sigma_kept = kept(kappa), kept(sigma)
        robin_kept = {bit: kept(alpha) for bit, alpha in (robin or {}).items()}
        op = _Operator(kappa_kept, self._generate(kappa_kept, sigma_kept, robin_kept), sigma_kept, robin_kept)
        self._last_operator = op
        return op

    def _holds(self, x: torch.Tensor, n: int, what: str) -> torch.Tensor:
        if x.dtype != torch.float64 or x.device != self.device or x.numel() != n:
            raise ValueError(f"{what} must hold {n} float64 on {self.device} (got {x.numel()} {x.dtype} on {x.device})")
        return x

    def _same_size(self, x: torch.Tensor, what: str) -> torch.Tensor:
        return self._holds(x, self.hierarchy.n_dofs(self.top), what)

    def _device_vector(self, x: torch.Tensor, what: str) -> torch.Tensor:
        return self._same_size(x, what).detach().contiguous()

    def _pcg(self, rhs: torch.Tensor, which: str, warm: bool = True) -> torch.Tensor:
        """A x = rhs from zero, or from the last solution of this kind (warm_start and `warm`); rhs and x by pointer."""
        h = self.hierarchy
        warm = warm and self.warm_start
        torch.cuda.current_stream(self.device).synchronize()        # rhs is complete before the handle's stream reads it
        h.set_vector_device(self.top, "f", rhs.data_ptr())
        x0 = self._warm.get(which) if warm else None
        if x0 is not None:
            h.set_vector_device(self.top, "v", x0.data_ptr())
        else:
            h.zero_vector(self.top, "v")
        self.n_solves += 1
        hist = h.pcg(rtol=self.rtol, max_iter=self.max_iter, level=self.top)
        self.last_iterations[which] = len(hist)
        self.last_residual[which] = float(hist[-1]) / h.norm2(self.top, "f") if len(hist) else None
        if len(hist) >= self.max_iter and not hist[-1] <= self.rtol * h.norm2(self.top, "f"):
            raise NotConverged(f"the {which} solve reached max_iter = {self.max_iter} at ||r|| = {hist[-1]:.3e} "
                               f"(rtol {self.rtol:g}): no gradient is returned")
        x = torch.empty_like(rhs)
        h.get_vector_device(self.top, "v", x.data_ptr())
        if warm:
            self._warm[which] = x.clone()
        return x


    def _pcg_many(self, rhs: torch.Tensor, which: str, warm: bool = True) -> torch.Tensor:
        """A x_b = rhs[b] for every row of the contiguous (B, n) `rhs`, in one `pcg_batch` (at most MG_BATCH_MAX lanes per
        call), from zero or from the last batched solution of this kind with as many lanes (warm_start and `warm`)."""
        from ._capi import MG_BATCH_MAX
        h = self.hierarchy
        warm = warm and self.warm_start
        B, n = rhs.shape
        x0 = self._warm_many.get(which) if warm else None
        x = x0.clone() if x0 is not None and x0.shape == rhs.shape else torch.zeros_like(rhs)
        torch.cuda.current_stream(self.device).synchronize()        # rhs and x are complete before the handle's stream reads them
        step = 8 * n
        hists = []
        for b0 in range(0, B, MG_BATCH_MAX):
            lanes = range(b0, min(B, b0 + MG_BATCH_MAX))
            hists += h.pcg_batch([rhs.data_ptr() + b * step for b in lanes], [x.data_ptr() + b * step for b in lanes],
                                 rtol=self.rtol, max_iter=self.max_iter, level=self.top)
        self.n_solves += B
        self.n_batched_solves += 1
        its = [len(hist) for hist in hists]
        norms = torch.linalg.vector_norm(rhs, dim=1).tolist()
        self.last_iterations[which] = max(its)
        self.last_lane_iterations[which] = its
        ratios = [float(hist[-1]) / nb for hist, nb in zip(hists, norms) if len(hist)]
        self.last_residual[which] = max(ratios) if ratios else None
        late = [b for b, (hist, nb) in enumerate(zip(hists, norms)) if len(hist) >= self.max_iter and not hist[-1] <= self.rtol * nb]
        if late:
            raise NotConverged(f"the batched {which} solve reached max_iter = {self.max_iter} in the lanes {late} of {B} "
                               f"(||r|| = {', '.join('%.3e' % hists[b][-1] for b in late)}; rtol {self.rtol:g}): no gradient is returned")
        if warm:
            self._warm_many[which] = x.clone()
        return x


class _Operator:
    """The kappa (and the sigma, or None, and the Robin fields by face bit) of one `solve` as the library takes them (a host
    array or a device copy) and the generation of the hierarchy that holds them: what the solves nested in that solve's backward passes share, so that they neither upload
    nor regenerate an operator that is still in place."""

    def __init__(self, kappa_kept, generation, sigma_kept=None, robin_kept=None):
        self.kappa_kept, self.generation, self.sigma_kept = kappa_kept, generation, sigma_kept
        self.robin_kept = robin_kept or {}


class _Solve(torch.autograd.Function):
    """S(kappa, f) = A(kappa)^-1 f.  `op` None: the caller's solve, which puts kappa into the hierarchy.  `op` given: a solve
    on the operator of an earlier one (from a backward pass, or `tangent`); `kappa` is then only what the gradient is
    taken with respect to (None: nobody asked), and the hierarchy is touched only if another kappa has been solved since.
    After `warm` come, each optional but in this order: `many` (True: `f` holds B leading rows, U[b] = A^-1 F[b] in one batched
    solve, `DiffusionSolver._pcg_many`), `sigma` (None: no reaction term; the operator is A(kappa) + R(sigma), and sigma is
    to the reaction term what kappa is to the stiffness -- on a given `op`, only what the gradient is taken with respect to),
    the tuple of the Robin fields' face bits, ascending, and one alpha per face: the operator is A(kappa) + R(sigma) +
    B(alpha), and each alpha is to its face what sigma is to the reaction term."""

    @staticmethod
    def forward(ctx, kappa, f, solver, op, which, warm, *fields):
        many, sigma, bits, *alphas = fields + (False, None, ())[len(fields):]
        if many:
            n = solver.hierarchy.n_dofs(solver.top)
            if f.dtype != torch.float64 or f.device != solver.device or f.dim() < 2 or f[0].numel() != n:
                raise ValueError(f"the right-hand sides must hold leading rows of {n} float64 on {solver.device}")
            rhs = f.detach().contiguous().view(f.shape[0], n)
        else:
            rhs = solver._device_vector(f, "f" if op is None else "the right-hand side")
        if op is None:
            op = solver._put_operator(kappa, sigma, dict(zip(bits, alphas)))
        elif op.generation != solver._generation:       # another kappa has been solved since: this one's operator again
            op.generation = solver._generate(op.kappa_kept, op.sigma_kept, op.robin_kept)
        u = (solver._pcg_many if many else solver._pcg)(rhs, which, warm).view(f.shape)
        ctx.solver, ctx.op, ctx.many, ctx.bits, ctx.n_inputs = solver, op, many, bits, 6 + len(fields)
        # kappa, sigma and the alphas are kept as what the gradient is taken with respect to, never for their values (those
        # are op.kappa_kept, ...): not through save_for_backward, whose version check would refuse a caller who has
        # overwritten the tensor since
        coefficients = {0: kappa, 7: sigma, **{9 + q: a for q, a in enumerate(alphas)}}
        ctx.like = {i: (c.shape, c.device) for i, c in coefficients.items() if c is not None}
        ctx.wanted = {i: c if i in ctx.like and ctx.needs_input_grad[i] else None for i, c in coefficients.items()}
        ctx.save_for_backward(u)
        return u

    @staticmethod
    def backward(ctx, grad_u):
        # lambda = S(kappa, grad_u), grad_f = lambda, grad_kappa = -D(lambda, u): A is symmetric.  Written with the functions
        # themselves, so that under create_graph autograd can differentiate it again; without, it runs under no_grad and is
        # one mg_pcg and one sensitivity kernel.  With B lanes the nested solve is batched and D is applied per lane, the
        # lanes' terms summed in ascending order with the first term starting the accumulator.
        solver, wanted = ctx.solver, ctx.wanted
        (u,) = ctx.saved_tensors
        lam = _Solve.apply(wanted[0], grad_u, solver, ctx.op, "adjoint", not torch.is_grad_enabled(), ctx.many, wanted[7],
                           ctx.bits, *[wanted[9 + q] for q in range(len(ctx.bits))])
        lanes = u.shape[0] if ctx.many else 1
        lam_of, u_of = (lam.reshape(lanes, -1), u.reshape(lanes, -1)) if ctx.many else ((lam,), (u,))

        def minus_d(i, field):
            if wanted[i] is None:
                return None
            acc = _D.apply(lam_of[0], u_of[0], solver, field)
            for b in range(1, lanes):
                acc = acc + _D.apply(lam_of[b], u_of[b], solver, field)
            shape, device = ctx.like[i]
            return acc.neg().view(shape).to(device)

        grads = [minus_d(0, _kappa_field("interior", "interior")), lam if ctx.needs_input_grad[1] else None, None, None, None,
                 None, None, minus_d(7, _SIGMA_FIELD), None] + [minus_d(9 + q, _alpha_field(bit)) for q, bit in enumerate(ctx.bits)]
        return tuple(grads[:ctx.n_inputs])


class _Eigs(torch.autograd.Function):
    """(lam, U) of `DiffusionSolver.eigenpairs`.  Backward: sum_j lam_bar_j (d lam_j / d field) with the first-order formulas
    of an M-normalised eigenvector, by the D entries at (u_j, u_j); once differentiable."""

    @staticmethod
    def forward(ctx, kappa, solver, op, k, block, x0, rtol, max_iter, rho, sigma, bits, *alphas):
        from ._capi import MG_EIGS_MAX
        h, n = solver.hierarchy, solver.hierarchy.n_dofs(solver.top)
        block = min(MG_EIGS_MAX, k + 2) if block is None else int(block)
        if not 1 <= k <= block <= MG_EIGS_MAX:
            raise ValueError(f"1 <= k <= block <= {MG_EIGS_MAX} (MG_EIGS_MAX) is required, got k = {k}, block = {block}")
        rho_kept = None
        if rho is not None:
            rho_kept = solver._holds(rho, solver.N ** 3, "rho").detach().reshape(-1).contiguous()
        X = torch.zeros(block, n, dtype=torch.float64, device=solver.device)
        if x0 is not None:
            if x0.dtype != torch.float64 or x0.device != solver.device or x0.dim() < 2 or x0[0].numel() != n or not 1 <= x0.shape[0] <= block:
                raise ValueError(f"x0 must hold 1..{block} leading rows of {n} float64 on {solver.device}")
            have = x0.shape[0]
            X[:have] = x0.detach().reshape(have, n)
            if have < block:
                X[have:] = torch.randn(block - have, n, dtype=torch.float64, generator=torch.Generator().manual_seed(have)).to(solver.device)
        if op is None:
            op = solver._put_operator(kappa, sigma, dict(zip(bits, alphas)))
        elif op.generation != solver._generation:       # another kappa has been solved since: this one's operator again
            op.generation = solver._generate(op.kappa_kept, op.sigma_kept, op.robin_kept)
        torch.cuda.current_stream(solver.device).synchronize()      # X and rho are complete before the handle's stream reads them
        out = h.eigs(k, block, rho=None if rho_kept is None else rho_kept.data_ptr(), x_ptrs=[X.data_ptr() + 8 * n * j for j in range(block)],
                     warm=x0 is not None, rtol=rtol, max_iter=max_iter, level=solver.top)
        solver.last_iterations["eigs"] = out["iterations"]
        solver.last_residual["eigs"] = float(out["resid"][:k].max())
        solver.last_eigs = out
        if not bool((out["resid"][:k] <= rtol).all()):
            raise NotConverged(f"the eigenpairs reached max_iter = {max_iter} with residuals "
                               f"{', '.join('%.3e' % r for r in out['resid'][:k])} (rtol {rtol:g})")
        U = X[:k]
        at = U.abs().argmax(dim=1, keepdim=True)
        U = U * torch.where(U.gather(1, at) < 0, -1.0, 1.0)
        lam = torch.tensor(out["lambda"][:k], dtype=torch.float64, device=solver.device)
        coefficients = {0: kappa, 8: rho, 9: sigma, **{11 + q: a for q, a in enumerate(alphas)}}
        ctx.like = {i: (c.shape, c.device) for i, c in coefficients.items() if c is not None}
        ctx.wanted = {i: i in ctx.like and ctx.needs_input_grad[i] for i in coefficients}
        ctx.solver, ctx.bits, ctx.n_inputs = solver, bits, 11 + len(alphas)
        ctx.save_for_backward(lam, U)
        U = U.view(k, solver.N + 1, solver.N + 1, solver.N + 1)
        ctx.mark_non_differentiable(U)
        return lam, U

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_lam, grad_U):
        solver = ctx.solver
        lam, U = ctx.saved_tensors
        g = grad_lam.to(solver.device)

        def d(field, j):
            return _launch(solver, lambda *args: field.d(solver.hierarchy, *args), solver.N ** field.power, U[j], U[j])

        def summed(i, field, weight=None):
            if not ctx.wanted[i]:
                return None
            acc = None
            for j in range(U.shape[0]):
                term = (g[j] if weight is None else g[j] * weight[j]) * d(field, j)
                acc = term if acc is None else acc + term
            shape, device = ctx.like[i]
            return acc.view(shape).to(device)

        grads = [summed(0, _kappa_field("interior", "interior"))] + [None] * 7 + [summed(8, _SIGMA_FIELD, -lam), summed(9, _SIGMA_FIELD), None]
        grads += [summed(11 + q, _alpha_field(bit)) for q, bit in enumerate(ctx.bits)]
        return tuple(grads[:ctx.n_inputs])


class _Field:
    """A coefficient field of the operator as D and T see it: kappa with a node set per side, sigma, or the alpha of one face.
    `d(hierarchy, level, a, b, out)` and `t(hierarchy, level, w, x, out)` are its two entries on `DeviceHierarchy` (with the
    field's own extra argument, the node sets or the face bit, in place), `noun` is what the refusal of a direction of the
    wrong size calls it, N^`power` its length, and `transposed` the field of the transposed operator (kappa: the node sets
    swapped; R and B are diagonal)."""

    def __init__(self, noun, power, d, t, transposed=None):
        self.noun, self.power, self.d, self.t = noun, power, d, t
        self.transposed = transposed or (lambda: self)


def _kappa_field(rows: str, cols: str) -> _Field:
    """D(a, b; A, B) = mg_diffusion_dkappa(a, b) with a node set per vector ("interior": the boundary entries count as 0), and
    T(w, x; R, C) = M_R A^(w) M_C x = mg_diffusion_apply_dkappa(w, x) with a node set for the rows and one for the columns
    ((interior, interior): (dA/dkappa . w) x); N^3 cells."""
    return _Field("kappa", 3, lambda h, level, a, b, out: h.diffusion_dkappa(level, a, b, out, rows, cols),
                  lambda h, level, w, x, out: h.diffusion_apply_dkappa(level, w, x, out, rows, cols), lambda: _kappa_field(cols, rows))


# D_sigma(a, b) = mg_diffusion_dsigma(a, b) and T_sigma(w, x) = R(w) x = mg_diffusion_apply_dsigma(w, x) on the free nodes, 0
# on the Dirichlet nodes, whose entries of a and b count as 0; N^3 cells
_SIGMA_FIELD = _Field("sigma", 3, DeviceHierarchy.diffusion_dsigma, DeviceHierarchy.diffusion_apply_dsigma)


def _alpha_field(bit: int) -> _Field:
    """D_alpha,F(a, b) = mg_diffusion_drobin(a, b) and T_alpha,F(w, x) = b_F(w) x = mg_diffusion_apply_drobin(w, x) on the
    free nodes of the face with bit `bit`, 0 on every other node; N^2 face-cells."""
    return _Field("alpha", 2, lambda h, level, a, b, out: h.diffusion_drobin(level, bit, a, b, out),
                  lambda h, level, w, x, out: h.diffusion_apply_drobin(level, bit, w, x, out))


def _launch(solver, entry, n_out: int, *operands) -> torch.Tensor:
    """What every autograd function below does forward: `entry(top level, *addresses of the operands, address of the
    result)` on `n_out` fresh float64, once the current stream has finished with the operands (checked, detached and
    contiguous already; None: a null pointer), which the handle's stream reads."""
    out = torch.empty(n_out, dtype=torch.float64, device=solver.device)
    torch.cuda.current_stream(solver.device).synchronize()
    entry(solver.top, *[None if t is None else t.data_ptr() for t in operands], out.data_ptr())
    return out


class _D(torch.autograd.Function):
    """D(a, b) of a `_Field`: the derivative of a^T (the field's term of the operator) b with respect to the field, one value
    per cell.  With cotangent w: a_bar = T(w, b), b_bar = T^T(w, a), T^T the T of the transposed field."""

    @staticmethod
    def forward(ctx, a, b, solver, field):
        ctx.solver, ctx.field = solver, field
        ctx.save_for_backward(a, b)
        return _launch(solver, lambda *args: field.d(solver.hierarchy, *args), solver.N ** field.power,
                       solver._device_vector(a, "a"), solver._device_vector(b, "b"))

    @staticmethod
    def backward(ctx, w):
        a, b = ctx.saved_tensors
        grad_a = _T.apply(w, b, ctx.solver, ctx.field).view(a.shape) if ctx.needs_input_grad[0] else None
        grad_b = _T.apply(w, a, ctx.solver, ctx.field.transposed()).view(b.shape) if ctx.needs_input_grad[1] else None
        return grad_a, grad_b, None, None


class _T(torch.autograd.Function):
    """T(w, x) of a `_Field`: the field's term of the operator with the direction w in the field's place, applied to x,
    (N + 1)^3 nodes.  With cotangent y: w_bar = D(y, x), x_bar = T^T(w, y)."""

    @staticmethod
    def forward(ctx, w, x, solver, field):
        cells = solver.N ** field.power
        if w.dtype != torch.float64 or w.device != solver.device or w.numel() != cells:
            raise ValueError(f"the {field.noun} direction must hold {cells} float64 on {solver.device}")
        ctx.solver, ctx.field = solver, field
        ctx.save_for_backward(w, x)
        return _launch(solver, lambda *args: field.t(solver.hierarchy, *args), solver.hierarchy.n_dofs(solver.top),
                       w.detach().contiguous(), solver._device_vector(x, "x"))

    @staticmethod
    def backward(ctx, y):
        w, x = ctx.saved_tensors
        grad_w = _D.apply(y, x, ctx.solver, ctx.field).view(w.shape) if ctx.needs_input_grad[0] else None
        grad_x = _T.apply(w, y, ctx.solver, ctx.field.transposed()).view(x.shape) if ctx.needs_input_grad[1] else None
        return grad_w, grad_x, None, None


def _cell_field(solver, t: Optional[torch.Tensor], count: int, what: str) -> Optional[torch.Tensor]:
    return None if t is None else solver._holds(t, count * solver.N ** 3, what).detach().contiguous()


class _CellGrad(torch.autograd.Function):
    """F(w, x) = mg_diffusion_cell_gradient(w, x), 3 N^3: the cell gradient of the nodal field x weighted by the cell field w
    (None: no weight).  With cotangent P: w_bar = C(P, x), x_bar = F^T(w, P)."""

    @staticmethod
    def forward(ctx, w, x, solver):
        ctx.solver, ctx.weighted = solver, w is not None
        ctx.save_for_backward(w, x)
        return _launch(solver, solver.hierarchy.diffusion_cell_gradient, 3 * solver.N ** 3,
                       _cell_field(solver, w, 1, "the cell weight"), solver._device_vector(x, "x"))

    @staticmethod
    def backward(ctx, P):
        w, x = ctx.saved_tensors
        grad_w = _CellGradDot.apply(P, x, ctx.solver).view(w.shape) if ctx.weighted and ctx.needs_input_grad[0] else None
        grad_x = _CellGradT.apply(w, P, ctx.solver).view(x.shape) if ctx.needs_input_grad[1] else None
        return grad_w, grad_x, None


class _CellGradT(torch.autograd.Function):
    """F^T(w, p) = mg_diffusion_cell_gradient_t(w, p), (N + 1)^3 nodes: the transpose of F in x.  With cotangent y:
    w_bar = C(p, y), p_bar = F(w, y)."""

    @staticmethod
    def forward(ctx, w, p, solver):
        ctx.solver, ctx.weighted = solver, w is not None
        ctx.save_for_backward(w, p)
        return _launch(solver, solver.hierarchy.diffusion_cell_gradient_t, solver.hierarchy.n_dofs(solver.top),
                       _cell_field(solver, w, 1, "the cell weight"), _cell_field(solver, p, 3, "the cell field"))

    @staticmethod
    def backward(ctx, y):
        w, p = ctx.saved_tensors
        grad_w = _CellGradDot.apply(p, y, ctx.solver).view(w.shape) if ctx.weighted and ctx.needs_input_grad[0] else None
        grad_p = _CellGrad.apply(w, y, ctx.solver).view(p.shape) if ctx.needs_input_grad[1] else None
        return grad_w, grad_p, None


class _CellGradDot(torch.autograd.Function):
    """C(p, x) = mg_diffusion_cell_gradient_dot(p, x), N^3 cells: p_c . G(x)_c.  With cotangent z: p_bar = F(z, x),
    x_bar = F^T(z, p)."""

    @staticmethod
    def forward(ctx, p, x, solver):
        ctx.solver = solver
        ctx.save_for_backward(p, x)
        return _launch(solver, solver.hierarchy.diffusion_cell_gradient_dot, solver.N ** 3,
                       _cell_field(solver, p, 3, "the cell field"), solver._device_vector(x, "x"))

    @staticmethod
    def backward(ctx, z):
        p, x = ctx.saved_tensors
        grad_p = _CellGrad.apply(z, x, ctx.solver).view(p.shape) if ctx.needs_input_grad[0] else None
        grad_x = _CellGradT.apply(z, p, ctx.solver).view(x.shape) if ctx.needs_input_grad[1] else None
        return grad_p, grad_x, None


def _points(solver, X: torch.Tensor) -> torch.Tensor:
    if X.dtype != torch.float64 or X.device != solver.device or X.dim() != 2 or X.shape[1] != 3 or X.shape[0] < 1:
        raise ValueError(f"points must be (M, 3) float64 with M >= 1 on {solver.device} (got {tuple(X.shape)} {X.dtype} on {X.device})")
    return X.detach().contiguous()


def _point_launch(solver, method, n_out: int, X: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    M = X.shape[0]
    return _launch(solver, lambda level, pp, pv, po: method(level, M, pp, pv, po), n_out, X, v)


class _PointSample(torch.autograd.Function):
    """S(u, X) = mg_diffusion_point_sample, M values: the P1 interpolant of the nodal field u at the points X.  With cotangent
    y: u_bar = S^T(y, X), X_bar = y[:, None] * G(u, X) -- the derivative inside the located simplex."""

    @staticmethod
    def forward(ctx, u, X, solver):
        ctx.solver = solver
        ctx.save_for_backward(u, X)
        return _point_launch(solver, solver.hierarchy.diffusion_point_sample, X.shape[0], _points(solver, X),
                             solver._device_vector(u, "u"))

    @staticmethod
    def backward(ctx, y):
        u, X = ctx.saved_tensors
        grad_u = _PointLoad.apply(y, X, ctx.solver).view(u.shape) if ctx.needs_input_grad[0] else None
        grad_X = y[:, None] * _PointGrad.apply(u, X, ctx.solver) if ctx.needs_input_grad[1] else None
        return grad_u, grad_X, None


class _PointLoad(torch.autograd.Function):
    """S^T(w, X) = mg_diffusion_point_load, (N + 1)^3 nodes: the consistent point load of the weights w at the points X.  With
    cotangent y (nodes): w_bar = S(y, X), X_bar = w[:, None] * G(y, X)."""

    @staticmethod
    def forward(ctx, w, X, solver):
        ctx.solver = solver
        ctx.save_for_backward(w, X)
        Xc = _points(solver, X)
        return _point_launch(solver, solver.hierarchy.diffusion_point_load, solver.hierarchy.n_dofs(solver.top), Xc,
                             solver._holds(w, Xc.shape[0], "the point weights").detach().contiguous())

    @staticmethod
    def backward(ctx, y):
        w, X = ctx.saved_tensors
        grad_w = _PointSample.apply(y, X, ctx.solver).view(w.shape) if ctx.needs_input_grad[0] else None
        grad_X = w.reshape(-1)[:, None] * _PointGrad.apply(y, X, ctx.solver) if ctx.needs_input_grad[1] else None
        return grad_w, grad_X, None


class _PointGrad(torch.autograd.Function):
    """G(u, X) = mg_diffusion_point_gradient, (M, 3): the gradient of u_h in the simplex that holds each point.  With cotangent
    P: u_bar = G^T(P, X); piecewise constant in X, so X gets no derivative."""

    @staticmethod
    def forward(ctx, u, X, solver):
        ctx.solver = solver
        ctx.save_for_backward(u, X)
        return _point_launch(solver, solver.hierarchy.diffusion_point_gradient, 3 * X.shape[0], _points(solver, X),
                             solver._device_vector(u, "u")).view(-1, 3)

    @staticmethod
    def backward(ctx, P):
        u, X = ctx.saved_tensors
        grad_u = _PointGradT.apply(P, X, ctx.solver).view(u.shape) if ctx.needs_input_grad[0] else None
        return grad_u, None, None


class _PointGradT(torch.autograd.Function):
    """G^T(p, X) = mg_diffusion_point_gradient_t, (N + 1)^3 nodes: the transpose of G in u.  With cotangent y: p_bar = G(y, X);
    X gets no derivative."""

    @staticmethod
    def forward(ctx, p, X, solver):
        ctx.solver = solver
        ctx.save_for_backward(p, X)
        Xc = _points(solver, X)
        return _point_launch(solver, solver.hierarchy.diffusion_point_gradient_t, solver.hierarchy.n_dofs(solver.top), Xc,
                             solver._holds(p, 3 * Xc.shape[0], "the point vectors").detach().contiguous())

    @staticmethod
    def backward(ctx, y):
        p, X = ctx.saved_tensors
        grad_p = _PointGrad.apply(y, X, ctx.solver).view(p.shape) if ctx.needs_input_grad[0] else None
        return grad_p, None, None


class LocatedPoints:
    """A point set located once on the solver's top level (`DiffusionSolver.locate`; `mg_points_create`): what `sample`,
    `point_load`, `sample_gradient` and their `_many` forms take in place of the (M, 3) tensor.  It remembers the tensor it was
    made from: that tensor receives the position derivatives if it requires grad, and once it has been written in place
    (its `_version` has moved: an optimiser stepped it) every use raises, because the located simplices are those of the old
    positions -- call `locate` again.  Closing it (or the solver) frees the device memory of the set."""

    def __init__(self, solver: "DiffusionSolver", points: torch.Tensor):
        X = _points(solver, points)
        self.solver, self.source, self.M = solver, points, X.shape[0]
        self._version = points._version
        torch.cuda.current_stream(solver.device).synchronize()      # the points are complete before the handle's stream copies them
        self.set = solver.hierarchy.points(solver.top, (X.data_ptr(), self.M))

    @property
    def info(self) -> dict:
        return self.set.info

    def close(self):
        self.set.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def fresh(self) -> "LocatedPoints":
        """Itself, or a RuntimeError if the tensor it was located from has been written since."""
        if self.source._version != self._version:
            raise RuntimeError("the tensor these points were located from has been modified in place since (version "
                               f"{self._version} -> {self.source._version}): the located simplices are stale; call locate again")
        return self


def _set_launch(P: LocatedPoints, method, V: torch.Tensor, n_in: int, n_out: int, what: str) -> torch.Tensor:
    """`method` (one of the `PointSet.*_many`) on the rows of the (B, n_in) `V`, at most MG_BATCH_MAX lanes per call in
    ascending chunks, into a fresh (B, n_out)."""
    from ._capi import MG_BATCH_MAX
    solver = P.fresh().solver
    if V.dtype != torch.float64 or V.device != solver.device or V.dim() != 2 or V.shape[0] < 1 or V.shape[1] != n_in:
        raise ValueError(f"{what} must hold B >= 1 rows of {n_in} float64 on {solver.device} (got {tuple(V.shape)} {V.dtype} on {V.device})")
    Vc = V.detach().contiguous()
    B = Vc.shape[0]
    out = torch.empty((B, n_out), dtype=torch.float64, device=solver.device)
    torch.cuda.current_stream(solver.device).synchronize()
    for b0 in range(0, B, MG_BATCH_MAX):
        lanes = range(b0, min(B, b0 + MG_BATCH_MAX))
        method([Vc.data_ptr() + 8 * n_in * b for b in lanes], [out.data_ptr() + 8 * n_out * b for b in lanes])
    return out


def _position_grad(ctx, weights: torch.Tensor, fields: torch.Tensor) -> Optional[torch.Tensor]:
    """The position derivative of S and S^T summed over the lanes: sum_b weights_b[:, None] * G(fields_b, X)."""
    if not ctx.needs_input_grad[1]:
        return None
    return (weights[:, :, None] * _SetGrad.apply(fields, ctx.P.source, ctx.P)).sum(0)


class _SetSample(torch.autograd.Function):
    """S(U, P) = mg_points_sample, (B, M): `_PointSample` for B fields on a located set.  X is the tensor the set was located
    from (it only receives the position derivative).  With cotangent Y: U_bar = S^T(Y, P), X_bar = sum_b Y_b[:, None] G(U_b, P)."""

    @staticmethod
    def forward(ctx, U, X, P):
        ctx.P = P
        ctx.save_for_backward(U)
        return _set_launch(P, P.set.sample_many, U, P.solver.hierarchy.n_dofs(P.solver.top), P.M, "the fields")

    @staticmethod
    def backward(ctx, Y):
        U, = ctx.saved_tensors
        grad_U = _SetLoad.apply(Y, ctx.P.source, ctx.P) if ctx.needs_input_grad[0] else None
        return grad_U, _position_grad(ctx, Y, U), None


class _SetLoad(torch.autograd.Function):
    """S^T(W, P) = mg_points_load, (B, nodes).  With cotangent Y: W_bar = S(Y, P), X_bar = sum_b W_b[:, None] G(Y_b, P)."""

    @staticmethod
    def forward(ctx, W, X, P):
        ctx.P = P
        ctx.save_for_backward(W)
        return _set_launch(P, P.set.load_many, W, P.M, P.solver.hierarchy.n_dofs(P.solver.top), "the point weights")

    @staticmethod
    def backward(ctx, Y):
        W, = ctx.saved_tensors
        grad_W = _SetSample.apply(Y, ctx.P.source, ctx.P) if ctx.needs_input_grad[0] else None
        return grad_W, _position_grad(ctx, W, Y), None


class _SetGrad(torch.autograd.Function):
    """G(U, P) = mg_points_gradient, (B, M, 3).  With cotangent Q: U_bar = G^T(Q, P); piecewise constant in the positions."""

    @staticmethod
    def forward(ctx, U, X, P):
        ctx.P = P
        return _set_launch(P, P.set.gradient_many, U, P.solver.hierarchy.n_dofs(P.solver.top), 3 * P.M, "the fields").view(-1, P.M, 3)

    @staticmethod
    def backward(ctx, Q):
        grad_U = _SetGradT.apply(Q.reshape(Q.shape[0], -1), ctx.P.source, ctx.P) if ctx.needs_input_grad[0] else None
        return grad_U, None, None


class _SetGradT(torch.autograd.Function):
    """G^T(Q, P) = mg_points_gradient_t, (B, nodes), Q (B, 3 M).  With cotangent Y: Q_bar = G(Y, P)."""

    @staticmethod
    def forward(ctx, Q, X, P):
        ctx.P = P
        return _set_launch(P, P.set.gradient_t_many, Q, 3 * P.M, P.solver.hierarchy.n_dofs(P.solver.top), "the point vectors")

    @staticmethod
    def backward(ctx, Y):
        grad_Q = _SetGrad.apply(Y, ctx.P.source, ctx.P).reshape(Y.shape[0], -1) if ctx.needs_input_grad[0] else None
        return grad_Q, None, None
