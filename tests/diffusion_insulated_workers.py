"""Helpers and test bodies of tests/test_diffusion_insulated.py: the cases, the host figures, and the DiffusionSolver runs, which
need a process that imports torch first (see tests/test_diffusion_adjoint.py).  Each body prints what it measured and asserts."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests.diffusion_workers import lognormal_kappa  # noqa: E402

EPS = np.finfo(np.float64).eps
INS = poisson.INSULATED
RTOL = 1e-10

# the singular solves: (N, levels); the coarsest grids are 3^3 and 7^3 nodes
SINGULAR_CASES = ((16, 4), (12, 2))
# Relative l2 distance between the device's singular solve (mg_pcg at rtol 1e-10, V(2,2) Jacobi) and
# poisson.insulated_solve_reference.  The limit is 8 x the largest figure observed on an MI355X, stored and matrix-free alike:
# random load 3.958e-11 (N = 16, 16 iterations) and 4.427e-11 (N = 12, 15 iterations); source and sink pair 3.033e-11 (N = 16)
# and 2.987e-11 (N = 12); the closed-form cosine mode at N = 16 9.399e-12 (13 iterations)
SINGULAR_LIMIT = 8 * 4.427e-11
# backward at N = 8, two levels, rtol 1e-12 against the host formulas: grad_kappa 3.603e-13, grad_f 3.784e-13 observed
BACKWARD_LIMIT = 8 * 3.784e-13
# the regular cases at N = 12, rtol 1e-10 against the host reference: sigma > 0 1.664e-12, alpha > 0 on two faces 5.131e-13 observed
REGULAR_LIMIT = 8 * 1.664e-12
# Hessian-vector product and tangent at N = 8 against the host's projected solves: 4.788e-13 and 4.163e-13 observed (rtol 1e-12);
# the existing second-order tests' limit (tests/diffusion_tangent_workers.py, SECOND_ORDER_LIMIT) holds here unchanged
from tests.diffusion_tangent_workers import SECOND_ORDER_LIMIT  # noqa: E402


def _rel(x, y):
    return float(np.linalg.norm(np.asarray(x).reshape(-1) - np.asarray(y).reshape(-1)) / np.linalg.norm(y))


def lumped_mass(N):
    return poisson.reaction_diag(N, np.ones(N ** 3), INS)


def random_load(N, seed=5):
    """a random load whose sum is far from zero"""
    return np.random.default_rng(seed).standard_normal((N + 1) ** 3) + 0.25


SOURCE, SINK = (0.23, 0.31, 0.67), (0.81, 0.72, 0.28)       # off-grid for N = 8, 12, 16, 32
RECEIVERS = ((0.52, 0.18, 0.44), (0.37, 0.83, 0.59))


def pair_load(N):
    """a point source and an equal sink (sum zero)"""
    return poisson.diffusion_point_load(N, np.array([SOURCE, SINK]), np.array([1.0, -1.0]))


def cosine_mode(N):
    c = np.arange(N + 1) / N
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    return (np.cos(np.pi * X) * np.cos(2 * np.pi * Y) * np.cos(3 * np.pi * Z)).reshape(-1)


def cosine_eigenvalue(N):
    h = 1.0 / N
    return sum((2.0 / h ** 2) * (1.0 - np.cos(m * np.pi * h)) for m in (1, 2, 3))


def insulated_matrix(N, kappa):
    return poisson.diffusion_level(N, 3, kappa, dirichlet_faces=INS).A.tocsr()


@functools.lru_cache(maxsize=None)
def nonzero_condition(N, seed=3):
    """lambda_max / lambda_2 of the host matrix A(kappa) with the empty face set (lambda_1 = 0: the constants)"""
    from scipy.sparse.linalg import eigsh
    A = insulated_matrix(N, lognormal_kappa(N, 3, seed=seed)).tocsc()
    v0 = np.cos(np.arange(A.shape[0]) * 0.7311 + 0.3)
    hi = eigsh(A, k=1, which="LA", v0=v0, tol=1e-8, return_eigenvectors=False)[0]
    lo = np.sort(eigsh(A, k=2, sigma=-1e-3 * hi, which="LM", v0=v0, tol=1e-10, return_eigenvectors=False))
    assert abs(lo[0]) <= 1e-8 * hi < lo[1], lo
    return float(hi / lo[1])


def pairwise_bound(x, w=None):
    """What a pairwise (tree) sum of n terms may miss: (log2 n + 2) eps sum |t_i|, the terms t_i = w_i x_i rounded once (+1)
    and the division (+1); relative to the denominator."""
    t = np.abs(x) if w is None else np.abs(x * w)
    denom = x.size if w is None else float(np.sum(w))
    return (np.ceil(np.log2(max(2, x.size))) + 3) * EPS * float(np.sum(t)) / denom


def host_adjoint(N, kappa, f, d):
    """J = 1/2 ||u - d||^2 with u = S(kappa) f: (u, dJ/dkappa = -D(lambda, u), dJ/df = lambda), lambda = S (u - d)"""
    u = poisson.insulated_solve_reference(N, kappa, f)
    lam = poisson.insulated_solve_reference(N, kappa, u - d)
    return u, -poisson.diffusion_dkappa(N, lam, u, dirichlet_faces=INS), lam


def host_hessian_vector(N, kappa, f, d, v):
    """the kappa block of the Hessian of J applied to v: four projected solves (tests/diffusion_tangent_workers.py)"""
    S = lambda rhs: poisson.insulated_solve_reference(N, kappa, rhs)
    T = lambda w, x: poisson.diffusion_apply_dkappa(N, w, x, dirichlet_faces=INS)
    D = lambda a, b: poisson.diffusion_dkappa(N, a, b, dirichlet_faces=INS)
    u = S(f)
    lam = S(u - d)
    du = S(-T(v, u))
    dlam = S(du - T(v, lam))
    return -D(dlam, u) - D(lam, du)


# ---- bodies that need torch first ------------------------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")


def singular_worker():
    """N = 16 on four levels and N = 12 on two, stored and matrix-free, log-normal kappa: a random load with nonzero sum, a source
    and sink pair, and at N = 16 the cosine mode from the load A mode."""
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    worst = 0.0
    for N, levels in SINGULAR_CASES:
        kappa = lognormal_kappa(N, 3, seed=3)
        A, w = insulated_matrix(N, kappa), lumped_mass(N)
        s = float(w.sum())
        cond = nonzero_condition(N)
        loads = {"random": (kappa, random_load(N)), "pair": (kappa, pair_load(N))}
        if N == 16:
            ones = np.ones(N ** 3)
            loads["cosine"] = (ones, insulated_matrix(N, ones) @ cosine_mode(N))
        want = {name: (cosine_mode(N) if name == "cosine" else poisson.insulated_solve_reference(N, k, f)) for name, (k, f) in loads.items()}
        for store, min_rows in (("stored", None), ("matrix_free", 0)):
            with DiffusionSolver(N, levels, rtol=RTOL, dirichlet_faces=INS, matrix_free_min_rows=min_rows) as solver:
                for name, (k, f) in loads.items():
                    u = solver.solve(_dev(k), _dev(f)).cpu().numpy().reshape(-1)
                    h = solver.hierarchy
                    assert h.diffusion_nullspace() and h.diffusion_faces() == 0
                    assert all(h.level_matrix_free(l) == (store == "matrix_free") for l in range(1, levels))
                    Ak = A if name != "cosine" else insulated_matrix(N, k)
                    qf = f - w * (f.sum() / s)
                    res = np.linalg.norm(qf - Ak @ u) / np.linalg.norm(qf)
                    # MG_VEC_F holds the projected load, MG_VEC_R the residual against it
                    kept = h.get_vector(solver.top, "f").reshape(-1)
                    rel = _rel(u, want[name])
                    print(f"N={N} {store} {name}: iterations {solver.last_iterations['forward']}  ||Q^T f - A u|| / ||Q^T f|| {res:.3e}  "
                          f"|w.u| {abs(w @ u):.3e}  rel to reference {rel:.3e}  cond {cond:.3e}", flush=True)
                    assert _rel(kept, qf) <= 64 * EPS, _rel(kept, qf)
                    assert solver.last_residual["forward"] <= RTOL
                    assert res <= RTOL * (1 + 1e-3) + 64 * EPS * cond, res       # (the true residual: the recursion's plus rounding)
                    assert abs(w @ u) <= 64 * EPS * np.linalg.norm(w) * np.linalg.norm(u)
                    assert rel <= SINGULAR_LIMIT and rel <= cond * RTOL, (rel, cond * RTOL)
                    worst = max(worst, rel)
                    again = solver.solve(_dev(k), _dev(f)).cpu().numpy().reshape(-1)
                    assert again.tobytes() == u.tobytes()
    print("largest rel %.3e" % worst)
    print("singular ok")


def convergence_worker():
    """N = 32 on four levels: the insulated singular solve against one Dirichlet face on the same kappa at the same rtol"""
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 32
    kappa, f = lognormal_kappa(N, 3, seed=3), random_load(N)
    its = {}
    for name, faces in (("insulated", INS), ("x-", ("x-",))):
        with DiffusionSolver(N, 4, rtol=RTOL, dirichlet_faces=faces) as solver:
            ff = f if faces == INS else np.where(poisson.dirichlet_mask(N, faces), 0.0, f)
            solver.solve(_dev(kappa), _dev(ff))
            its[name] = solver.last_iterations["forward"]
    print("iterations", its, flush=True)
    assert its["insulated"] <= 2 * its["x-"] + 2, its
    print("convergence ok")


def capture_worker():
    """N = 32 on four levels: forward, backward and a Hessian-vector product with captured cycles and with "graph" 0"""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 32
    kappa, f = lognormal_kappa(N, 3, seed=3), random_load(N)
    v = np.random.default_rng(7).standard_normal(N ** 3)
    got = {}
    for graph in (1, 0):
        with DiffusionSolver(N, 4, rtol=RTOL, dirichlet_faces=INS) as solver:
            solver.hierarchy.set_tuning("graph", graph)
            k = _dev(kappa).requires_grad_(True)
            u = solver.solve(k, _dev(f))
            (g,) = torch.autograd.grad(0.5 * (u ** 2).sum(), k, create_graph=True)
            (hv,) = torch.autograd.grad((g * _dev(v)).sum(), k)
            replays = solver.hierarchy.counters()["graph_replays"]
            assert (replays > 0) == bool(graph), replays
            got[graph] = [x.detach().cpu().numpy().tobytes() for x in (u, g, hv)]
            assert solver.n_solves == 4
    assert got[0] == got[1]
    print("capture ok")


def derivatives_worker():
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 8
    rng = np.random.default_rng(21)
    kappa, f, d = lognormal_kappa(N, 3, seed=4), random_load(N, 6), rng.standard_normal((N + 1) ** 3)
    v, dkappa, df = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3), rng.standard_normal((N + 1) ** 3)
    u, gk, gf = host_adjoint(N, kappa, f, d)
    hk = host_hessian_vector(N, kappa, f, d, v)

    def gradient(solver, kap):
        k = _dev(kap).requires_grad_(True)
        J = 0.5 * torch.sum((solver.solve(k, _dev(f)) - _dev(d)) ** 2)
        return torch.autograd.grad(J, k)[0].cpu().numpy()

    with DiffusionSolver(N, 2, rtol=1e-12, dirichlet_faces=INS) as solver:
        k, ft = _dev(kappa).requires_grad_(True), _dev(f).requires_grad_(True)
        ut = solver.solve(k, ft)
        assert solver.n_solves == 1
        J = 0.5 * torch.sum((ut - _dev(d)) ** 2)
        g, glam = torch.autograd.grad(J, (k, ft), create_graph=True)
        assert solver.n_solves == 2, solver.n_solves
        figures = (_rel(g.detach().cpu().numpy(), gk), _rel(glam.detach().cpu().numpy(), gf))
        print("backward: rel l2 grad_kappa %.3e  grad_f %.3e" % figures, flush=True)
        assert max(figures) <= BACKWARD_LIMIT, figures
        (hv,) = torch.autograd.grad(torch.sum(g * _dev(v)), k)
        assert solver.n_solves == 4, solver.n_solves
        hv = hv.cpu().numpy()
        print("Hessian-vector product: rel l2 to the host's %.3e" % _rel(hv, hk), flush=True)
        assert _rel(hv, hk) <= SECOND_ORDER_LIMIT
        # ... and against central differences of device gradients: fd(t) misses by c t^2, so fd(t / 2) misses by a third of
        # fd(t) - fd(t / 2); the gradients' own error (about 1e-12 relative) divided by t is far below that
        t = 1e-2
        fd = {s: (gradient(solver, kappa + s * v * kappa.min()) - gradient(solver, kappa - s * v * kappa.min())) / (2 * s * kappa.min()) for s in (t, t / 2)}
        gap = np.linalg.norm(fd[t] - fd[t / 2])
        print("central differences: |hv - fd(t/2)| %.3e  |fd(t) - fd(t/2)| %.3e  |hv| %.3e" % (np.linalg.norm(hv - fd[t / 2]), gap, np.linalg.norm(hv)), flush=True)
        assert gap <= 1e-2 * np.linalg.norm(hv) and np.linalg.norm(hv - fd[t / 2]) <= gap
        # tangent against the directional derivative
        before = solver.n_solves
        u2, du = solver.tangent(_dev(kappa), _dev(f), _dev(dkappa), _dev(df))
        assert solver.n_solves == before + 2
        S = lambda kap, rhs: poisson.insulated_solve_reference(N, kap, rhs)
        du_host = S(kappa, df - poisson.diffusion_apply_dkappa(N, dkappa, u, dirichlet_faces=INS))
        print("tangent: rel l2 du %.3e" % _rel(du.cpu().numpy(), du_host), flush=True)
        assert _rel(du.cpu().numpy(), du_host) <= SECOND_ORDER_LIMIT
        step = 1e-4 * kappa.min() / np.abs(dkappa).max()
        quotient = (S(kappa + step * dkappa, f + step * df) - S(kappa - step * dkappa, f - step * df)) / (2 * step)
        assert _rel(du.cpu().numpy(), quotient) <= 1e-6, _rel(du.cpu().numpy(), quotient)
    print("derivatives ok")


def regular_worker():
    """sigma > 0, alpha > 0 on two faces, solve_many, implicit Euler steps"""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N, levels = 12, 2
    kappa, f, w = lognormal_kappa(N, 3, seed=3), random_load(N), lumped_mass(N)
    sigma = 1.0 + lognormal_kappa(N, 3, seed=8, sigma=0.5)
    robin = {"x-": np.full(N * N, 2.0), "z+": 0.5 + lognormal_kappa(N, 2, seed=9, sigma=0.5)}
    with DiffusionSolver(N, levels, rtol=RTOL, dirichlet_faces=INS) as solver:
        h = solver.hierarchy
        u = solver.solve(_dev(kappa), _dev(f), sigma=_dev(sigma)).cpu().numpy()
        assert not h.diffusion_nullspace() and h.diffusion_faces() == 0
        rel = _rel(u, poisson.insulated_solve_reference(N, kappa, f, sigma=sigma))
        print("sigma: rel %.3e" % rel, flush=True)
        assert rel <= REGULAR_LIMIT
        F = np.stack([random_load(N, s) for s in (1, 2, 3)])
        many = solver.solve_many(_dev(kappa), _dev(F), sigma=_dev(sigma), same_operator=True).cpu().numpy()
        for b in range(3):
            one = solver.solve(_dev(kappa), _dev(F[b]), sigma=_dev(sigma), same_operator=True).cpu().numpy()
            assert one.tobytes() == many[b].tobytes(), b
        lam, _ = solver.eigenpairs(_dev(kappa), 2, sigma=_dev(sigma), same_operator=True)
        assert float(lam[0]) > 0.0
        u = solver.solve(_dev(kappa), _dev(f), robin={k: _dev(a) for k, a in robin.items()}).cpu().numpy()
        assert not h.diffusion_nullspace() and solver.last_generate in ("host", "device")
        rel = _rel(u, poisson.insulated_solve_reference(N, kappa, f, robin=robin))
        print("robin on x- and z+: rel %.3e" % rel, flush=True)
        assert rel <= REGULAR_LIMIT
        # three implicit Euler steps of the insulated body with f = 0: (A + R(1 / dt)) u_new = R(1 / dt) u_old, and 1^T A = 0
        # gives w.u_new = w.u_old up to the solve's residual
        dt = 1e-2
        sig = _dev(np.full(N ** 3, 1.0 / dt))
        ut = _dev(1.0 + cosine_mode(N) + 0.3 * np.random.default_rng(2).standard_normal((N + 1) ** 3))
        heat = [float(w @ ut.cpu().numpy())]
        for step in range(3):
            ut = solver.solve(_dev(kappa), solver.reaction_apply(sig, ut), sigma=sig, same_operator=step > 0)
            heat.append(float(w @ ut.cpu().numpy().reshape(-1)))
        print("w.u over three steps", heat, flush=True)
        assert solver.last_generate is not None and not h.diffusion_nullspace()
        # each step's residual r has |1.r| <= sqrt(n) ||r|| <= sqrt(n) rtol ||rhs||, and w.u moves by dt (1.r)
        bound = 3 * dt * np.sqrt(w.size) * RTOL * np.linalg.norm(w / dt) * np.abs(ut.cpu().numpy()).max() * 4
        assert max(abs(x - heat[0]) for x in heat) <= bound, (heat, bound)
        u = solver.solve(_dev(kappa), _dev(f)).cpu().numpy()
        assert h.diffusion_nullspace()      # back to the singular case: the hierarchy was generated again
    print("regular ok")


def refusals_worker():
    import torch
    from multigrid_dolfinx_amd._capi import MgError
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver
    N = 8
    kappa, f = lognormal_kappa(N, 3, seed=3), random_load(N)
    with DiffusionSolver(N, 2, rtol=RTOL, dirichlet_faces=INS) as solver:
        h = solver.hierarchy
        first = solver.solve(_dev(kappa), _dev(f)).cpu().numpy().tobytes()
        generations = solver.n_generations

        def untouched():
            assert h.diffusion_faces() == 0 and h.diffusion_nullspace()
            assert solver.solve(_dev(kappa), _dev(f), same_operator=True).cpu().numpy().tobytes() == first
            assert solver.n_generations == generations

        def refused(call, exc, *words):
            try:
                call()
            except exc as e:
                assert all(word in str(e) for word in words), str(e)
            else:
                raise AssertionError("not refused: " + " ".join(words))
            untouched()

        g = torch.zeros((N + 1) ** 3, dtype=torch.float64, device="cuda")
        refused(lambda: solver.solve(_dev(kappa), _dev(f), g=g), ValueError, "insulated solver", "g must be None")
        refused(lambda: solver.tangent(_dev(kappa), _dev(f), _dev(kappa), g=g), ValueError, "insulated solver")
        refused(lambda: solver.solve_many(_dev(kappa), _dev(np.stack([f, f]))), ValueError, "solve_many", "singular")
        refused(lambda: solver.eigenpairs(_dev(kappa), 2), ValueError, "eigenpairs", "singular")
        x = torch.zeros(2, (N + 1) ** 3, dtype=torch.float64, device="cuda")
        rhs = torch.ones(2, (N + 1) ** 3, dtype=torch.float64, device="cuda")
        ptrs, fptrs = [x[b].data_ptr() for b in range(2)], [rhs[b].data_ptr() for b in range(2)]
        torch.cuda.synchronize()
        refused(lambda: h.pcg_batch(fptrs, ptrs, level=solver.top), MgError, "mg_pcg_batch", "mg_set_diffusion_insulated", "singular")
        refused(lambda: h.eigs(1, x_ptrs=ptrs[:1], block=1, level=solver.top), MgError, "mg_eigs", "singular")
        refused(lambda: h.fmg(1, top_level=solver.top), MgError, "mg_fmg", "singular")
        for smoother in ("chebyshev", "rbgs", "mcgs"):
            h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", smoother=smoother)
            try:
                h.set_vector(solver.top, "f", f)
                for call in (lambda: h.prepare_cycle(solver.top), lambda: h.vcycle(solver.top), lambda: h.pcg(level=solver.top)):
                    try:
                        call()
                    except MgError as e:
                        assert "singular" in str(e) and "Jacobi" in str(e), str(e)
                    else:
                        raise AssertionError("not refused: " + smoother)
            finally:
                h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose", smoother="jacobi")
            untouched()
        refused(lambda: h.set_diffusion_faces(0), MgError, "mg_set_diffusion_faces", "singular")
        refused(lambda: h.set_diffusion_faces(64), MgError, "is no face set")
        # a later valid set leaves the insulated state
        h.set_diffusion_faces(("x-",))
        assert h.diffusion_faces() == 1
        h.set_diffusion_insulated()
        untouched()
    with DeviceHierarchy(2, 0, 1, c=4) as h2:
        try:
            h2.set_diffusion_insulated()
        except MgError as e:
            assert "mg_set_diffusion_insulated" in str(e) and "2-D" in str(e), str(e)
        else:
            raise AssertionError("a 2-D handle was not refused")
        assert h2.diffusion_faces() == 63
    nothing = lambda *a: None
    with DeviceHierarchy(3, 0, 1, c=4) as slab:
        slab.set_comm_callbacks(0, 2, nothing, nothing, nothing)
        try:
            slab.set_diffusion_insulated()
        except MgError as e:
            assert "mg_set_diffusion_insulated" in str(e) and "whole (not slab) handle" in str(e), str(e)
        else:
            raise AssertionError("a slab handle was not refused")
        assert slab.diffusion_faces() == 63
    print("refusals ok")
