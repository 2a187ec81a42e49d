"""Host references and DiffusionSolver test bodies of tests/test_diffusion_robin.py: the Robin fields, the solve, the adjoint and
the four-solve Hessian-vector products of -div(kappa grad u) + sigma u = f with kappa du/dn + alpha (u - u_ext) = 0 on some
faces, built on scipy's sparse direct solves and the restatements of poisson.py.  The torch bodies run in a process of their own
that imports torch before libmg_hip.so is loaded (one HIP runtime for both); each prints its figures and ends with an "... ok"
line."""
import os
import sys

import numpy as np
import scipy.sparse.linalg as spl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests.diffusion_neumann_workers import free_mask, lifted_rhs  # noqa: E402
from tests.diffusion_reaction_workers import reaction_sigma  # noqa: E402

EPS = np.finfo(np.float64).eps

# (Dirichlet face set, Robin faces): (a) Dirichlet z-, Robin on z+ and x-; (b) Dirichlet x+ | z-, Robin on x- and y+ -- a
# Robin-Robin edge and corners that meet Dirichlet nodes; (c) Dirichlet x- only, Robin on the five other faces -- nodes on
# three field faces
CONFIGS = {"a": (16, (32, 1)), "b": (18, (1, 8)), "c": (1, (2, 4, 8, 16, 32))}


def robin_alpha(N, face, seed=0):
    """Log-uniform over six decades around the stiffness scale of a boundary row (alpha h from 1e-4 to 1e2 times kappa ~ 1),
    independent per face-cell, with a patch of zeros in one corner quarter."""
    z = np.random.default_rng(1000 * seed + face).random((N, N))
    alpha = float(N) * 10.0 ** (-4.0 + 6.0 * z)
    alpha[: max(1, N // 4), : max(1, N // 4)] = 0.0
    return np.ascontiguousarray(alpha.reshape(-1))


def robin_fields(N, faces, seed=0):
    return {face: robin_alpha(N, face, seed) for face in faces}


def _rel(x, y):
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


class HostOperator:
    """A(kappa) + R(sigma) + B(alpha) of the restated level, factorised once."""

    def __init__(self, N, kappa, sigma, robin, faces):
        self.N, self.kappa, self.sigma, self.robin, self.faces = N, kappa, sigma, robin, faces
        self.free = free_mask(N, faces)
        A = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=faces, sigma=sigma, robin=robin).A.tocsc()
        A.eliminate_zeros()
        self.lu = spl.splu(A, permc_spec="MMD_AT_PLUS_A")

    def solve(self, rhs):
        return self.lu.solve(np.asarray(rhs, dtype=np.float64).reshape(-1))

    def T(self, w, x, rows, cols):
        return poisson.diffusion_apply_dkappa(self.N, w, x, rows, cols, self.faces)

    def D(self, a, b, A, B):
        return poisson.diffusion_dkappa(self.N, a, b, A, B, self.faces)

    def Ds(self, a, b):
        return poisson.diffusion_dsigma(self.N, a, b, self.faces)

    def Tr(self, w, x):
        """sum over the field faces of T_alpha,F(w[F], x)"""
        return sum(poisson.diffusion_apply_drobin(self.N, face, w[face], x, self.faces) for face in w)

    def Dr(self, a, b):
        return {face: poisson.diffusion_drobin(self.N, face, a, b, self.faces) for face in self.robin}


def host_adjoint(op, f, g, d):
    """J = 1/2 ||u - d||^2 over all nodes: (J, u, dJ/dkappa, dJ/dalpha by face, dJ/dsigma, dJ/df, dJ/dg).  B is diagonal on free
    rows, so the lift and dJ/dg read no alpha, and dJ/dalpha_F = -D_alpha,F(lambda~, u)."""
    u = op.solve(lifted_rhs(op.N, op.kappa, f, g, op.faces))
    lam = op.solve(u - d)
    gk = -op.D(lam, u, "interior", "all")
    ga = {face: -x for face, x in op.Dr(lam, u).items()}
    gs = -op.Ds(lam, u)
    gg = np.where(op.free, 0.0, (u - d) - op.T(op.kappa, lam, "all", "interior"))
    return 0.5 * float(np.sum((u - d) ** 2)), u, gk, ga, gs, np.where(op.free, lam, 0.0), gg


def host_hessian_vector(op, f, g, d, vk, va):
    """With q = dJ/dkappa . vk + sum_F dJ/dalpha_F . va[F]: (dq/dkappa, dq/dalpha by face) in four solves; the operator's
    derivative along the direction is T(vk, .) + sum_F T_alpha,F(va[F], .)."""
    u = op.solve(lifted_rhs(op.N, op.kappa, f, g, op.faces))
    lam = op.solve(u - d)
    du = op.solve(-op.T(vk, u, "interior", "all") - op.Tr(va, u))
    dlam = op.solve(du - op.T(vk, lam, "interior", "interior") - op.Tr(va, lam))
    hk = -op.D(dlam, u, "interior", "all") - op.D(lam, du, "interior", "all")
    x, y = op.Dr(dlam, u), op.Dr(lam, du)
    return hk, {face: -x[face] - y[face] for face in x}


# Relative l2 distance between the DiffusionSolver results with Robin fields (mg_pcg at rtol 1e-12, V(2,2) Jacobi, N = 16, two
# levels) and the host references above (SuperLU).  The reference is the host adjoint; the limit is 8 x the largest figure
# measured once on an MI355X over configurations (a) and (b), both storages and the fields on the device and on the CPU: the
# margin REACTION_LIMIT (tests/diffusion_reaction_workers.py) gives for the run-to-run variation of the solves' residuals.  A
# figure above 1e-10 would be a defect, not a limit (_check_limit).
# Measured (stored and matrix-free, device and CPU fields alike to three digits; 18 to 19 iterations per solve), configuration
# (a): u 7.226e-13, J 1.132e-13, grad_kappa 5.252e-13, grad_sigma 6.954e-13, grad_f 3.074e-13, grad_g 3.123e-13, H_kk v 4.458e-13,
# H_ka v 4.712e-13, and per face (x-, z+) grad_alpha 6.805e-13, 8.561e-13, H_ak v 5.374e-13, 5.711e-13, H_aa v 5.505e-13,
# 6.305e-13; configuration (b): 4.260e-13, 3.438e-14, 3.717e-13, 4.561e-13, 3.083e-13, 3.169e-13, 3.184e-13, 4.500e-13, and per
# face (x-, y+) 5.937e-13, 8.225e-13, 5.169e-13, 6.002e-13, 5.810e-13, 6.657e-13.  8 x the largest:
ROBIN_MEASURED = 8.561e-13
ROBIN_LIMIT = 8 * ROBIN_MEASURED


# `tangent` with every direction at once (tangent_worker): u and du against the host, configuration (a), both storages, with
# g and without.  Measured once on an MI355X (stored and matrix-free alike to three digits): with g u 7.226e-13, du 4.491e-13;
# without g u 7.206e-13, du 4.502e-13; 19 iterations per solve.  8 x the largest, by the rule above:
TANGENT_MEASURED = 7.226e-13
TANGENT_LIMIT = 8 * TANGENT_MEASURED


def _case(config):
    from tests.diffusion_workers import lognormal_kappa
    N = 16
    faces, fields = CONFIGS[config]
    rng = np.random.default_rng(37)
    kappa = lognormal_kappa(N, 3, seed=4)
    n = (N + 1) ** 3
    f, d, g = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    vk = rng.standard_normal(N ** 3)
    robin = robin_fields(N, fields)
    va = {face: float(N) * rng.standard_normal(N ** 2) for face in fields}
    return N, faces, kappa, reaction_sigma(N), robin, f, d, g, vk, va


def _check_limit(worst, limit):
    print("largest discrepancy %.3e" % worst, flush=True)
    assert limit <= 1e-10, "a discrepancy above 1e-10 is a defect, not a limit"
    assert worst <= limit, (worst, limit)


def solver_worker():
    """u, J, the gradients with respect to kappa, alpha (every field face), sigma, f and g and the kappa-kappa, alpha-kappa,
    kappa-alpha and alpha-alpha blocks of Hessian-vector products against the host, configurations (a) and (b), both storages,
    the fields on the device and on the CPU; n_solves is 2 after the gradient, 4 after the first product and 6 after the
    second; one generation."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    dev = lambda x: torch.tensor(x, device="cuda")
    host = lambda t: t.detach().cpu().numpy()
    worst = 0.0
    for config in ("a", "b"):
        N, faces, kappa, sigma, robin, f, d, g, vk, va = _case(config)
        bits = sorted(robin)
        zero_a = {face: np.zeros(N ** 2) for face in bits}
        op = HostOperator(N, kappa, sigma, robin, faces)
        free = op.free
        J, u, gk, ga, gs, gf, gg = host_adjoint(op, f, g, d)
        hkk, hak = host_hessian_vector(op, f, g, d, vk, zero_a)
        hka, haa = host_hessian_vector(op, f, g, d, np.zeros(N ** 3), va)
        for name, min_rows in (("stored", None), ("matrix_free", 0)):
            for where in ("cuda", "cpu"):
                with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows, dirichlet_faces=faces) as solver:
                    k = torch.tensor(kappa, device=where, requires_grad=True)
                    s = torch.tensor(sigma, device=where, requires_grad=True)
                    al = {face: torch.tensor(robin[face], device=where, requires_grad=True) for face in bits}
                    ft, gt = dev(f).requires_grad_(), dev(g).requires_grad_()
                    ut = solver.solve(k, ft, gt, sigma=s, robin=al)
                    assert solver.last_generate == ("device" if where == "cuda" else "host"), solver.last_generate
                    assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
                    assert solver.hierarchy.level_robin(1) == sum(bits) and solver.hierarchy.level_robin(0) == sum(bits)
                    assert solver.hierarchy.diffusion_robin() == (sum(bits), N)
                    Jt = 0.5 * torch.sum((ut - dev(d)) ** 2)
                    alist = [al[face] for face in bits]
                    grads = torch.autograd.grad(Jt, [k, s, ft, gt] + alist, create_graph=True)
                    gkt, gst, gft, ggt, gat = grads[0], grads[1], grads[2], grads[3], grads[4:]
                    assert solver.n_solves == 2, solver.n_solves
                    prods = torch.autograd.grad(torch.sum(gkt * torch.tensor(vk, device=where)), [k] + alist, retain_graph=True)
                    pkk, pak = prods[0], prods[1:]
                    assert solver.n_solves == 4, solver.n_solves
                    q = sum(torch.sum(x * torch.tensor(va[face], device=where)) for face, x in zip(bits, gat))
                    prods = torch.autograd.grad(q, [k] + alist)
                    pka, paa = prods[0], prods[1:]
                    assert solver.n_solves == 6, solver.n_solves
                    assert solver.n_generations == 1
                    assert not host(ggt)[free].any() and not host(gft)[~free].any()
                    figures = [_rel(host(ut), u), abs(float(Jt.detach()) - J) / J, _rel(host(gkt), gk), _rel(host(gst), gs),
                               _rel(host(gft), gf), _rel(host(ggt), gg), _rel(host(pkk), hkk), _rel(host(pka), hka)]
                    for q, face in enumerate(bits):
                        figures += [_rel(host(gat[q]), ga[face]), _rel(host(pak[q]), hak[face]), _rel(host(paa[q]), haa[face])]
                    print(config, name, where, "iterations", solver.last_iterations, "rel l2: u %.3e  J %.3e  grad_kappa %.3e  "
                          "grad_sigma %.3e  grad_f %.3e  grad_g %.3e  H_kk v %.3e  H_ka v %.3e" % tuple(figures[:8]),
                          " per face (grad_alpha, H_ak v, H_aa v):", " ".join("%.3e" % x for x in figures[8:]), flush=True)
                    worst = max(worst, max(figures))
    _check_limit(worst, ROBIN_LIMIT)
    print("solver ok")


def host_tangent(op, f, g, dkappa, df, dg, dsigma, dalpha):
    """(u, du) in the direction (dkappa, df, dg, dsigma, dalpha by face, a subset of the field faces).  With g: the free rows of
    du's right-hand side are df - T(dkappa, u; interior, all) - T(kappa, dg_B; interior, all) - T_sigma(dsigma, u) -
    sum_F T_alpha,F(dalpha_F, u), dg_B = dg on the Dirichlet nodes and 0 on the free ones, and the Dirichlet rows are dg.
    Without g (f the full right-hand side, u_b = f_b): the columns are "interior", there is no dg term, and the Dirichlet rows
    are those of the full df, as tests/diffusion_tangent_workers.py has them."""
    free = op.free
    if g is None:
        u = op.solve(f)
        rhs = df - op.T(dkappa, u, "interior", "interior")
    else:
        u = op.solve(lifted_rhs(op.N, op.kappa, f, g, op.faces))
        rhs = df - op.T(dkappa, u, "interior", "all") - op.T(op.kappa, np.where(free, 0.0, dg), "interior", "all")
    rhs = rhs - poisson.diffusion_apply_dsigma(op.N, dsigma, u, op.faces) - op.Tr(dalpha, u)
    return u, op.solve(np.where(free, rhs, df if g is None else dg))


def tangent_worker():
    """`DiffusionSolver.tangent` with everything at once -- df, g and dg, sigma and dsigma, Robin fields on both field faces and
    a direction on one of them only -- and again with g = None, dg = None, configuration (a), both storages: u and du against
    the host, two solves and one generation per call (TANGENT_LIMIT holds the measured figure)."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, faces, kappa, sigma, robin, f, d, g, vk, va = _case("a")
    rng = np.random.default_rng(41)
    dg, dsigma = rng.standard_normal((N + 1) ** 3), rng.standard_normal(N ** 3)
    dkappa, df, dalpha = vk, d, {32: va[32]}
    dev = lambda x: torch.tensor(x, device="cuda")
    op = HostOperator(N, kappa, sigma, robin, faces)
    want = {True: host_tangent(op, f, g, dkappa, df, dg, dsigma, dalpha),
            False: host_tangent(op, f, None, dkappa, df, None, dsigma, dalpha)}
    worst = 0.0
    for name, min_rows in (("stored", None), ("matrix_free", 0)):
        with DiffusionSolver(N, 2, rtol=1e-12, matrix_free_min_rows=min_rows, dirichlet_faces=faces) as solver:
            fields = {face: dev(robin[face]) for face in robin}
            for with_g in (True, False):
                ut, dut = solver.tangent(dev(kappa), dev(f), dev(dkappa), dev(df), g=dev(g) if with_g else None,
                                         dg=dev(dg) if with_g else None, sigma=dev(sigma), dsigma=dev(dsigma), robin=fields,
                                         drobin={face: dev(x) for face, x in dalpha.items()})
                assert solver.hierarchy.level_matrix_free(1) == (name == "matrix_free")
                assert set(solver.last_iterations) == {"forward", "tangent"}
                figures = (_rel(ut.cpu().numpy(), want[with_g][0]), _rel(dut.cpu().numpy(), want[with_g][1]))
                print(name, "g" if with_g else "no g", "iterations", solver.last_iterations, "rel l2: u %.3e  du %.3e" % figures, flush=True)
                worst = max(worst, max(figures))
            assert solver.n_solves == 4 and solver.n_generations == 2, (solver.n_solves, solver.n_generations)
    _check_limit(worst, TANGENT_LIMIT)
    print("tangent ok")


def switch_worker():
    """On one solver with a device kappa: fields on (z+, x-), other values on the same faces, a field on z+ alone, none, and
    (z+, x-) again -- a change of WHICH faces hold a field generates ("device"), the same faces refresh; without fields the
    bits are those of a solver that never had one; same_operator reuses the operator; tangent with drobin against the host's
    A^-1 (-T_alpha(dalpha, u)); robin_apply against the restatement."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, faces, kappa, sigma, robin, f, d, g, vk, va = _case("a")
    dev = lambda x: torch.tensor(x, device="cuda")
    both = {face: dev(robin[face]) for face in robin}
    with DiffusionSolver(N, 2, rtol=1e-12, dirichlet_faces=faces) as plain, DiffusionSolver(N, 2, rtol=1e-12, dirichlet_faces=faces) as solver:
        w = np.random.default_rng(3).standard_normal(N ** 2)
        got = solver.robin_apply("z+", dev(w), dev(g)).cpu().numpy()
        assert got.tobytes() == poisson.diffusion_apply_drobin(N, "z+", w, g, faces).tobytes()
        want = plain.solve(dev(kappa), dev(f))
        seen = []
        for fields in (both, {face: 2.0 * x for face, x in both.items()}, {32: both[32]}, None, None, both):
            u = solver.solve(dev(kappa), dev(f), robin=fields)
            seen.append(solver.last_generate)
            assert solver.hierarchy.level_robin(1) == sum(fields or ())
            assert solver.hierarchy.diffusion_robin() == ((sum(fields), N) if fields else (0, 0))
            if fields is None:
                assert torch.equal(u, want)
        assert seen == ["device", "refresh", "device", "device", "refresh", "device"], seen
        assert solver.n_generations == 6
        again = solver.solve(dev(kappa), dev(f), robin=both, same_operator=True)
        assert solver.n_generations == 6 and torch.equal(again, u)
        try:
            solver.solve(dev(kappa), dev(f), robin={32: both[32]}, same_operator=True)
            raise AssertionError("same_operator with other field faces was accepted")
        except ValueError as exc:
            assert "Robin fields on the faces" in str(exc)
        try:
            solver.solve(dev(kappa), dev(f), robin={"z-": both[32]})
            raise AssertionError("a field on a Dirichlet face was accepted")
        except ValueError as exc:
            assert "Dirichlet face" in str(exc)
        # the forward-mode derivative along drobin against the host's A^-1 (-T_alpha(va, u)); both within the 1e-10 above which
        # _check_limit calls a discrepancy a defect
        dal = {32: dev(va[32])}
        ut, du = solver.tangent(dev(kappa), dev(f), torch.zeros(N ** 3, dtype=torch.float64, device="cuda"), robin=both, drobin=dal)
        op = HostOperator(N, kappa, None, robin, faces)
        uh = op.solve(f)
        duh = op.solve(-op.Tr({32: va[32]}, uh))
        print("tangent rel l2: u %.3e du %.3e" % (_rel(ut.cpu().numpy(), uh), _rel(du.cpu().numpy(), duh)), flush=True)
        assert _rel(ut.cpu().numpy(), uh) <= 1e-10 and _rel(du.cpu().numpy(), duh) <= 1e-10
    print("switch ok")
