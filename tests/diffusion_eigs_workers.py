"""Helpers and test bodies of tests/test_diffusion_eigs.py: the handles, the longdouble restatements of the block kernels, and the
figures of an mg_eigs run against the closed form and against poisson.diffusion_eigs_reference (each prints what it measured, the
test asserts)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multigrid_dolfinx_amd import poisson  # noqa: E402
from tests.diffusion_reaction_workers import reaction_sigma  # noqa: E402
from tests.diffusion_robin_workers import robin_alpha  # noqa: E402
from tests.diffusion_workers import lognormal_kappa  # noqa: E402
from tests.pde_reference import sine_eigenvalue, sine_mode  # noqa: E402

EPS = np.finfo(np.float64).eps
ZPLUS = 32

# the heterogeneous cases: kappa = lognormal_kappa(N, 3, seed=3) everywhere
CASES = {
    "a": dict(N=16, levels=3, faces=63, k=4, block=6),
    "b": dict(N=16, levels=3, faces=3, k=3, block=5, sigma=True, robin=True),
    "c": dict(N=32, levels=4, faces=63, k=4, block=6, rho=True),
    "d": dict(N=16, levels=3, faces=63, k=1, block=1),
}


class Lanes:
    """Device copies of a list of host vectors, freed on exit."""

    def __init__(self, h, hosts):
        from multigrid_dolfinx_amd.hierarchy import _DeviceArray
        hosts = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in hosts]
        self.arrays = [_DeviceArray(h._lib, h.device, x.size, x) for x in hosts]
        self.ptrs = [a.ptr.value for a in self.arrays]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for a in self.arrays:
            a.free()

    def download(self):
        return [a.download() for a in self.arrays]


def level_handle(N):
    """Level 1 of a two-level handle with (N + 1)^3 rows: all the block kernels need is the level's size."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    h = DeviceHierarchy(3, 0, 1, c=N // 2)
    h.gen_diffusion_level(1, lognormal_kappa(N, 3, seed=3))
    return h


def longdouble_gram(a, b, d):
    bl = b.astype(np.longdouble) if d is None else b.astype(np.longdouble) * d.astype(np.longdouble)
    return (a.astype(np.longdouble) @ bl.T).astype(np.float64)


def gram_bound(a, b, d):
    """n eps sum |a_i d b_j| per pair"""
    return a.shape[1] * EPS * (np.abs(a) @ (np.abs(b) if d is None else np.abs(b) * np.abs(d)).T)


def case_fields(case):
    cs = CASES[case]
    N = cs["N"]
    return dict(kappa=lognormal_kappa(N, 3, seed=3), sigma=reaction_sigma(N) if cs.get("sigma") else None,
                robin={ZPLUS: robin_alpha(N, ZPLUS)} if cs.get("robin") else None,
                rho=lognormal_kappa(N, 3, seed=5, sigma=0.5) if cs.get("rho") else None)


def diffusion_hierarchy(N, levels, faces, kappa, matrix_free, sigma=None, robin=None):
    """A generated diffusion hierarchy, stored or with every level above the coarsest matrix-free; P1 transfers, Jacobi V(2,2)."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    top = levels - 1
    h = DeviceHierarchy(3, 0, top, c=N >> top)
    h.set_prolongation("p1")
    h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
    h.set_diffusion_faces(faces)
    if sigma is not None:
        h.set_diffusion_reaction(sigma)
    for face, alpha in (robin or {}).items():
        h.set_diffusion_robin(face, alpha)
    h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0 if matrix_free else None)
    assert all(h.level_matrix_free(l) == matrix_free for l in range(1, top + 1))
    return h


def eigs_hierarchy(case, matrix_free):
    cs, f = CASES[case], case_fields(case)
    return diffusion_hierarchy(cs["N"], cs["levels"], cs["faces"], f["kappa"], matrix_free, f["sigma"], f["robin"])


def _m_normalised(v, m):
    return v / np.sqrt(np.sum(m * v * v))


def closed_form_figures(matrix_free):
    N, levels, kappa, k, block = 16, 3, 1.7, 4, 6
    m = poisson.reaction_diag(N, np.ones(N ** 3))
    with diffusion_hierarchy(N, levels, 63, np.full(N ** 3, kappa), matrix_free) as h:
        out = h.eigs(k, block, rtol=1e-8, max_iter=100)
    lam, X = out["lambda"], out["x"]
    want = np.array([sine_eigenvalue(N, mode, kappa) for mode in ((1, 1, 1), (1, 1, 2), (1, 1, 2), (1, 1, 2))])
    fig = dict(iterations=out["iterations"], restarts=out["restarts"], resid=out["resid"])
    fig["lambda_rel"] = float((np.abs(lam[:k] - want) / want).max())
    s = _m_normalised(sine_mode(N, (1, 1, 1)), m)
    fig["vector_rel"] = float(min(np.linalg.norm(X[0] - s), np.linalg.norm(X[0] + s)) / np.linalg.norm(s))
    worst = 0.0
    for mode in ((2, 1, 1), (1, 2, 1), (1, 1, 2)):
        s = _m_normalised(sine_mode(N, mode), m)
        proj = sum((X[j] @ (m * s)) * X[j] for j in (1, 2, 3))
        worst = max(worst, float(np.linalg.norm(s - proj) / np.linalg.norm(s)))
    fig["cluster_rel"] = worst
    print("closed form, %s: iterations %d restarts %d lambda %.3e x[0] %.3e cluster %.3e resid %s"
          % ("matrix-free" if matrix_free else "stored", fig["iterations"], fig["restarts"], fig["lambda_rel"], fig["vector_rel"],
             fig["cluster_rel"], np.array2string(out["resid"], precision=2)), flush=True)
    return fig


_REFERENCE = {}


def reference(case):
    """(lambda, U) of the host reference, computed once per case"""
    if case not in _REFERENCE:
        cs, f = CASES[case], case_fields(case)
        _REFERENCE[case] = poisson.diffusion_eigs_reference(cs["N"], f["kappa"], cs["k"], rho=f["rho"], dirichlet_faces=cs["faces"],
                                                            sigma=f["sigma"], robin=f["robin"])
    return _REFERENCE[case]


def heterogeneous_figures(case, matrix_free):
    cs, f = CASES[case], case_fields(case)
    N, k, block = cs["N"], cs["k"], cs["block"]
    n = (N + 1) ** 3
    m = poisson.reaction_diag(N, np.ones(N ** 3) if f["rho"] is None else f["rho"], cs["faces"])
    want = reference(case)[0]
    with eigs_hierarchy(case, matrix_free) as h, Lanes(h, [np.full(n, np.nan)] * block + [m]) as X:
        out = h.eigs(k, block, rho=f["rho"], x_ptrs=X.ptrs[:block], rtol=1e-8, max_iter=100)
        G = h.block_gram(X.ptrs[:block], X.ptrs[:block], X.ptrs[block])
        x = np.stack(X.download()[:block])
    fig = dict(iterations=out["iterations"], restarts=out["restarts"], resid=out["resid"])
    fig["lambda_rel"] = float((np.abs(out["lambda"][:k] - want) / want).max())
    fig["orthonormality_over_bound"] = float((np.abs(G - np.eye(block)) / gram_bound(x, x, m)).max())
    dirichlet = poisson.dirichlet_mask(N, cs["faces"])
    fig["dirichlet_bytes_zero"] = x[:, dirichlet].tobytes() == np.zeros((block, int(dirichlet.sum()))).tobytes()
    print("case %s, %s: iterations %d restarts %d lambda %.3e |X^T M X - I| / bound %.3e lambda %s resid %s"
          % (case, "matrix-free" if matrix_free else "stored", fig["iterations"], fig["restarts"], fig["lambda_rel"],
             fig["orthonormality_over_bound"], np.array2string(out["lambda"], precision=6), np.array2string(out["resid"], precision=2)), flush=True)
    return fig


# ---- DiffusionSolver.eigenpairs: runs in a process of its own that imports torch before libmg_hip.so is loaded ------------------------
def eigenpairs_worker(lambda_limit, gradient_limit):
    """N = 16 on two levels, rtol 1e-10, Dirichlet everywhere but z+ (a Robin face), a reaction field, a non-constant rho, k = 4:
    lam against the host reference, the sign rule of U, the gradients of lambda_1 and of the sum of the four against the host
    formulas at the reference's eigenvectors, a warm start, NotConverged, and the refusal of a second differentiation."""
    import torch
    from multigrid_dolfinx_amd.torch_diffusion import DiffusionSolver, NotConverged
    N, k, faces = 16, 4, 63 - ZPLUS
    dev = lambda x: torch.tensor(x, device="cuda")
    host = dict(kappa=lognormal_kappa(N, 3, seed=3), sigma=reaction_sigma(N), alpha=robin_alpha(N, ZPLUS), rho=lognormal_kappa(N, 3, seed=5, sigma=0.5))
    lam_ref, U_ref = poisson.diffusion_eigs_reference(N, host["kappa"], k, rho=host["rho"], dirichlet_faces=faces, sigma=host["sigma"],
                                                      robin={ZPLUS: host["alpha"]})
    print("reference lambda", lam_ref, flush=True)
    d = dict(kappa=lambda u: poisson.diffusion_dkappa(N, u, u, dirichlet_faces=faces), sigma=lambda u: poisson.diffusion_dsigma(N, u, u, dirichlet_faces=faces),
             alpha=lambda u: poisson.diffusion_drobin(N, ZPLUS, u, u, dirichlet_faces=faces))
    names = ("kappa", "sigma", "alpha", "rho")

    def want(name, j):
        return -lam_ref[j] * d["sigma"](U_ref[j]) if name == "rho" else d[name](U_ref[j])

    with DiffusionSolver(N, 2, matrix_free_min_rows=0, dirichlet_faces=faces) as solver:
        leaf = {name: dev(host[name]).requires_grad_() for name in names}
        lam, U = solver.eigenpairs(leaf["kappa"], k, rho=leaf["rho"], sigma=leaf["sigma"], robin={ZPLUS: leaf["alpha"]}, rtol=1e-10)
        print("iterations", solver.last_iterations["eigs"], "residual", solver.last_residual["eigs"], flush=True)
        assert lam.shape == (k,) and U.shape == (k, N + 1, N + 1, N + 1) and not U.requires_grad and lam.requires_grad
        rel = float(np.abs(lam.detach().cpu().numpy() - lam_ref).max() / lam_ref.min())
        print("lam: largest relative discrepancy %.3e (limit %.3e)" % (rel, lambda_limit), flush=True)
        assert rel <= lambda_limit
        flat = U.reshape(k, -1).cpu().numpy()
        for j in range(k):
            at = int(np.argmax(np.abs(flat[j])))
            assert flat[j, at] > 0.0 and not np.any(np.abs(flat[j, :at]) == abs(flat[j, at])), (j, at)
        worst = 0.0
        for what, J, members in (("lambda_1", lam[0], (0,)), ("sum of 4", lam.sum(), range(k))):
            grads = torch.autograd.grad(J, [leaf[name] for name in names], retain_graph=True)
            for name, got in zip(names, grads):
                ref = sum(want(name, j) for j in members)
                rel = float(np.linalg.norm(got.cpu().numpy().reshape(-1) - ref) / np.linalg.norm(ref))
                worst = max(worst, rel)
                print("d %s / d %s: relative l2 discrepancy %.3e" % (what, name, rel), flush=True)
        print("gradients: largest relative l2 discrepancy %.3e (limit %.3e)" % (worst, gradient_limit), flush=True)
        assert worst <= gradient_limit
        # second derivatives are not provided: they must raise, not return a number
        (g1,) = torch.autograd.grad(lam[0], leaf["kappa"], create_graph=True)
        try:
            torch.autograd.grad(g1.sum(), leaf["kappa"])
        except RuntimeError as e:
            print("second differentiation raised:", str(e)[:80], flush=True)
        else:
            raise AssertionError("a second differentiation returned a number")
        # a warm start from U on the same operator: no iteration, no generation
        generations = solver.n_generations
        lam2, U2 = solver.eigenpairs(leaf["kappa"].detach(), k, rho=leaf["rho"].detach(), sigma=leaf["sigma"].detach(), robin={ZPLUS: leaf["alpha"].detach()},
                                     rtol=1e-8, x0=U, same_operator=True)
        print("warm start iterations", solver.last_iterations["eigs"], flush=True)
        assert solver.n_generations == generations and solver.last_iterations["eigs"] <= 2
        assert float(((lam2 - lam.detach()).abs() / lam.detach()).max()) <= 1e-9
        try:
            solver.eigenpairs(leaf["kappa"].detach(), k, rho=leaf["rho"].detach(), sigma=leaf["sigma"].detach(), robin={ZPLUS: leaf["alpha"].detach()},
                              rtol=1e-10, max_iter=1, same_operator=True)
        except NotConverged as e:
            print("NotConverged:", str(e)[:100], flush=True)
        else:
            raise AssertionError("max_iter = 1 did not raise NotConverged")
    print("eigenpairs ok")
