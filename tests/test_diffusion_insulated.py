"""Insulated bodies: diffusion solves with no Dirichlet node (mg_set_diffusion_insulated, mg_diffusion_nullspace, mg_remove_mean,
poisson.INSULATED, poisson.insulated_solve_reference, DiffusionSolver(dirichlet_faces="insulated")).

CPU: the header, the binding and the library agree on the entries; the spelling and what it gives the host functions; the host
matrix of the empty face set; the host reference against its definition, against a closed form and against central differences;
the new kernels in the code object.
GPU: the mean-removal kernels; the operator on constants; the singular solve against the host reference, stored and matrix-free;
its iteration count against one Dirichlet face; determinism and captured cycles; derivatives; the regular case; refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from multigrid_dolfinx_amd import _capi, poisson
from tests.diffusion_insulated_workers import (EPS, INS, cosine_eigenvalue, cosine_mode, host_adjoint, insulated_matrix, lumped_mass,
                                               pairwise_bound, random_load)
from tests.diffusion_workers import lognormal_kappa
from tests.test_diffusion_batch import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multigrid_dolfinx_amd", "libmg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
ENTRIES = ("mg_set_diffusion_insulated", "mg_diffusion_nullspace", "mg_remove_mean")


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_insulated_entries():
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _capi.SIGNATURES and getattr(lib, name).argtypes == _capi.SIGNATURES[name], name
    p, i = C.c_void_p, C.c_int
    assert _capi.SIGNATURES["mg_set_diffusion_insulated"] == [p]
    assert _capi.SIGNATURES["mg_diffusion_nullspace"] == [p, i, C.POINTER(C.c_int)]
    assert _capi.SIGNATURES["mg_remove_mean"] == [p, p, p, C.c_int64, C.POINTER(C.c_double)]


def test_the_spelling_and_what_the_host_functions_make_of_it():
    assert poisson.INSULATED == "insulated" and poisson.face_set("insulated") == 0
    assert poisson.face_set(poisson.face_set("insulated")) == 0         # what face_set gave, handed on
    for bad in (0, 64, -1, np.int64(0), ("insulate",), "insulate", ()):
        with pytest.raises(ValueError):
            poisson.face_set(bad)
    assert poisson.free_box(8, "insulated") == ([0, 0, 0], [8, 8, 8])
    assert not poisson.dirichlet_mask(8, "insulated").any()
    N = 4
    x = np.random.default_rng(0).standard_normal((N + 1) ** 3)
    kappa = lognormal_kappa(N, 3, seed=1)
    A = insulated_matrix(N, kappa)
    # the sensitivity restatements take it: T(kappa, x) = A x, D(a, b) . dkappa = a^T T(dkappa, b), and the diagonals
    assert np.abs(poisson.diffusion_apply_dkappa(N, kappa, x, dirichlet_faces=INS) - A @ x).max() <= 64 * EPS * np.abs(A).sum(axis=1).max() * np.abs(x).max()
    d = np.random.default_rng(1).standard_normal(N ** 3)
    lhs = poisson.diffusion_dkappa(N, x, x, dirichlet_faces=INS) @ d
    assert abs(lhs - x @ poisson.diffusion_apply_dkappa(N, d, x, dirichlet_faces=INS)) <= 1e-12 * abs(lhs)
    assert np.all(poisson.reaction_diag(N, np.ones(N ** 3), INS) > 0.0)
    alpha = {"x-": np.ones(N * N), "y+": np.ones(N * N), "z+": np.ones(N * N)}     # any of the six faces
    assert abs(poisson.robin_diag(N, alpha, INS).sum() - 3.0) <= 64 * EPS
    assert poisson.diffusion_dsigma(N, x, x, INS).shape == (N ** 3,) and poisson.diffusion_drobin(N, "y+", x, x, INS).shape == (N * N,)


@pytest.mark.parametrize("N", [8, 12])
def test_host_matrix_of_the_empty_set_has_the_constants_as_null_space(N):
    A = insulated_matrix(N, lognormal_kappa(N, 3, seed=3))
    scale = np.abs(A).sum(axis=1).max()
    ones = np.ones(A.shape[0])
    assert np.abs(A @ ones).max() <= 16 * EPS * scale and np.abs(A.T @ ones).max() <= 16 * EPS * scale
    assert abs(A - A.T).max() == 0.0
    w = lumped_mass(N)
    assert abs(w.sum() - 1.0) <= 16 * EPS and np.all(w > 0.0)


@pytest.mark.parametrize("N", [8, 12])
def test_reference_solves_the_projected_system(N):
    """log-normal kappa, a random f with nonzero sum: A u + (1.f / s) w = f, w.u = 0, and S symmetric"""
    kappa = lognormal_kappa(N, 3, seed=3)
    A, w = insulated_matrix(N, kappa), lumped_mass(N)
    s = w.sum()
    f, g = random_load(N, 5), random_load(N, 6)
    assert abs(f.sum()) > 1.0
    u, v = poisson.insulated_solve_reference(N, kappa, f), poisson.insulated_solve_reference(N, kappa, g)
    # a backward-stable solve: the residual is eps (||A|| ||u|| + ||f||) with a modest factor
    bound = 256 * EPS * (np.abs(A).sum(axis=1).max() * np.abs(u).max() + np.abs(f).max())
    assert np.abs(A @ u + (f.sum() / s) * w - f).max() <= bound
    assert abs(w @ u) <= 64 * EPS * np.linalg.norm(w) * np.linalg.norm(u)
    assert abs(f @ v - g @ u) <= 1e-10 * abs(f @ v)
    # the regular cases are plain solves
    sigma = np.full(N ** 3, 2.0)
    us = poisson.insulated_solve_reference(N, kappa, f, sigma=sigma)
    As = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=INS, sigma=sigma).A
    assert np.abs(As @ us - f).max() <= bound
    robin = {"x-": np.ones(N * N), 32: np.ones(N * N)}
    ur = poisson.insulated_solve_reference(N, kappa, f, robin=robin)
    Ar = poisson.diffusion_level(N, 3, kappa, dirichlet_faces=INS, robin=robin).A
    assert np.abs(Ar @ ur - f).max() <= 256 * EPS * (np.abs(Ar).sum(axis=1).max() * np.abs(ur).max() + np.abs(f).max())


@pytest.mark.parametrize("N", [8, 16])
def test_reference_returns_the_cosine_mode(N):
    """kappa = 1 and the mode cos(pi x) cos(2 pi y) cos(3 pi z) at the nodes, lambda_h = sum_d (2 / h^2)(1 - cos(m_d pi h)).

    Checked first, on the host matrix: A mode = lambda_h w * mode holds to rounding in every row of a node that lies on at most
    one face of the cube -- there the uniform Kuhn mesh gives the seven-point operator and its half-weight face rows -- and does
    NOT hold on the cube's twelve edges and eight corners, where the weights of the natural rows and of w depend on how the
    Kuhn simplices sit in the corner (largest miss 2.05e-2 at N = 8, 2.75e-3 at N = 16; with that load the solve misses the
    mode by 0.38 and 0.14).  So the load of the closed form is A mode, from the host matrix, which is the seven-point closed
    form wherever that one holds: w.mode = 0, the load is consistent, and the solve must return the mode."""
    h = 1.0 / N
    ones = np.ones(N ** 3)
    A, w, mode, lam = insulated_matrix(N, ones), lumped_mass(N), cosine_mode(N), cosine_eigenvalue(N)
    c = np.arange(N + 1)
    on = ((c == 0) | (c == N)).astype(int)
    faces_at = (on[:, None, None] + on[None, :, None] + on[None, None, :]).reshape(-1)
    miss = np.abs(A @ mode - lam * w * mode)
    assert miss[faces_at <= 1].max() <= 64 * EPS * lam * h ** 3
    assert miss[faces_at >= 2].max() > 1e-3
    assert abs(w @ mode) <= 16 * EPS
    u = poisson.insulated_solve_reference(N, ones, A @ mode)
    print("N = %d: largest |u - mode| %.3e" % (N, np.abs(u - mode).max()))
    assert np.abs(u - mode).max() <= 1e-12


def test_host_gradient_formulas_against_central_differences():
    """J = 1/2 ||u - t||^2 at N = 6: grad_kappa = -D(lambda, u) and grad_f = lambda, lambda = S (u - t), against central differences
    along random directions; the miss falls by a factor between 3 and 5 when the step halves (kappa), and J is exactly
    quadratic in f (no truncation: the miss is the quotient's rounding)."""
    N = 6
    rng = np.random.default_rng(4)
    kappa, f, t = lognormal_kappa(N, 3, seed=2), random_load(N, 3), rng.standard_normal((N + 1) ** 3)
    J = lambda k, ff: 0.5 * float(np.sum((poisson.insulated_solve_reference(N, k, ff) - t) ** 2))
    u, gk, gf = host_adjoint(N, kappa, f, t)
    for seed in (0, 1):
        d = np.random.default_rng(seed).uniform(-1.0, 1.0, N ** 3) * kappa
        miss = [abs((J(kappa + e * d, f) - J(kappa - e * d, f)) / (2 * e) - gk @ d) for e in (0.01, 0.005)]
        print("kappa direction %d: miss %.3e, %.3e of %.3e" % (seed, miss[0], miss[1], abs(gk @ d)))
        assert 3.0 <= miss[0] / miss[1] <= 5.0 and miss[1] <= 1e-3 * abs(gk @ d), miss
        df = np.random.default_rng(seed + 10).standard_normal((N + 1) ** 3)
        e = 1e-3
        quotient = (J(kappa, f + e * df) - J(kappa, f - e * df)) / (2 * e)
        assert abs(quotient - gf @ df) <= 1e-10 * J(kappa, f) / e, (quotient, gf @ df)
    # a uniform load is projected away: no gradient along it, and none along the constants either
    assert abs(gf.sum()) <= 1e-10 * np.abs(gf).sum() or abs(gf @ lumped_mass(N)) <= 1e-12 * np.abs(gf).max()


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_nullspace_kernels_are_in_the_code_object_within_their_resources():
    notes = _kernel_notes()
    found = {}
    for name, res in notes.items():
        m = re.match(r"mgk::(ns_partial|ns_subtract|ns_pin_dense|ns_unpin_inverse)\(", name)
        if m:
            found[m.group(1)] = res
    assert sorted(found) == ["ns_partial", "ns_pin_dense", "ns_subtract", "ns_unpin_inverse"], sorted(found)
    for key, (spilled, scratch, group, vgpr) in sorted(found.items()):
        print(key, "vgpr", vgpr, "lds", group)
        assert spilled == 0 and scratch == 0, (key, spilled, scratch)
        assert vgpr <= 64, (key, vgpr)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [100, 2048, 4096, 2049, 12289])
def test_mean_removal_kernels(n):
    """ns_partial / ns_subtract through mg_remove_mean, with and without weights: a length below one workgroup tile (2048 rows),
    one and two tiles exactly, and odd lengths past a tile.  The mean agrees with a longdouble sum within the bound of a pairwise
    sum of that length (the kernels' tree is at least as deep as pairwise only across lanes; a thread adds at most 8 terms in a
    row, which the bound's + 3 levels cover), every entry is x - mean rounded once, and a second run gives the same bits."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    from tests.diffusion_eigs_workers import Lanes
    rng = np.random.default_rng(n)
    x, w = rng.standard_normal(n) + 0.5, rng.uniform(0.5, 1.5, n)
    with DeviceHierarchy(3, 0, 1, c=2) as h:
        with Lanes(h, [x]) as lanes:        # the partial sums and their total are the handle's, and counted
            before = h.memory_bytes()
            h.remove_mean(lanes.ptrs[0], n)
            assert h.memory_bytes() - before == 8 * ((n + 2047) // 2048 + 1)
        for weights in (None, w):
            out = []
            for run in range(2):
                with Lanes(h, [x] + ([weights] if weights is not None else [])) as lanes:
                    mean = h.remove_mean(lanes.ptrs[0], n, lanes.ptrs[1] if weights is not None else None)
                    out.append((mean, lanes.download()[0]))
            xl = x.astype(np.longdouble)
            want = float((xl * weights).sum() / weights.astype(np.longdouble).sum()) if weights is not None else float(xl.sum() / n)
            bound = pairwise_bound(x, weights) + (8 * EPS * abs(want) if weights is not None else 0.0)    # (+ the weights' own sum)
            print("n = %d weights %s: mean off by %.3e, bound %.3e" % (n, weights is not None, abs(out[0][0] - want), bound))
            assert abs(out[0][0] - want) <= bound
            assert np.array_equal(out[0][1], x - out[0][0])
            assert out[0][0] == out[1][0] and out[0][1].tobytes() == out[1][1].tobytes()
            if weights is not None:
                with Lanes(h, [x, weights[:-1]]) as lanes:       # a misaligned weight pointer is refused by name
                    with pytest.raises(_capi.MgError, match="16-byte aligned"):
                        h.remove_mean(lanes.ptrs[0], n - 1, lanes.ptrs[1] + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("N,levels", [(8, 3), (12, 2)])
@pytest.mark.parametrize("matrix_free", [False, True])
def test_operator_annihilates_the_constants(N, levels, matrix_free):
    """R = F - A V with V = c and F = 0 on the top level of an insulated hierarchy: zero to rounding, c times 16 eps times the
    largest absolute row sum"""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    kappa = lognormal_kappa(N, 3, seed=3)
    top = levels - 1
    scale = np.abs(insulated_matrix(N, kappa)).sum(axis=1).max()
    with DeviceHierarchy(3, 0, top, c=N >> top) as h:
        h.set_prolongation("p1")
        h.set_params(2, 2, 2.0 / 3.0, restriction="p1_transpose")
        h.set_diffusion_insulated()
        assert h.diffusion_faces() == 0
        h.gen_diffusion_hierarchy(kappa, matrix_free_min_rows=0 if matrix_free else None)
        assert h.level_matrix_free(top) == matrix_free and h.diffusion_nullspace(top) and h.diffusion_nullspace(0)
        n = (N + 1) ** 3
        h.set_vector(top, "v", np.full(n, 3.0))
        h.set_vector(top, "f", np.zeros(n))
        h.residual(top)
        r = h.get_vector(top, "r").reshape(-1)
        print("largest |A c| %.3e" % np.abs(r).max())
        assert np.abs(r).max() <= 3.0 * 16 * EPS * scale
        # cycles work on such a handle, captured and prepared: a consistent load, two cycles, the residual falls
        f = random_load(N)
        f -= f.mean()
        h.set_vector(top, "f", f)
        h.zero_vector(top, "v")
        h.prepare_cycle(top)
        hist = h.vcycle(top, 3, residuals=True)
        print("V-cycle residuals", hist)
        assert hist[2] < 0.2 * hist[0]


def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_insulated_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_singular_solve_against_the_host_reference():
    """N = 16 on four levels (a coarsest grid of 3^3 nodes) and N = 12 on two, stored and matrix-free, log-normal kappa; a random
    load with nonzero sum, a source and sink pair, the cosine mode: the residual against the projected load, |w.u|, the distance
    to `insulated_solve_reference` (SINGULAR_LIMIT holds the observed figures; and below cond rtol), the same bytes twice
    (`singular_worker`)."""
    assert "singular ok" in _torch_first("singular_worker")


@pytest.mark.gpu
def test_singular_solve_converges_like_one_dirichlet_face():
    """N = 32 on four levels, rtol 1e-10: at most twice the iterations of dirichlet_faces=("x-",) plus two (`convergence_worker`;
    observed 17 against 19).  A coarse correction that mishandles the constants leaves the smoother's convergence."""
    assert "convergence ok" in _torch_first("convergence_worker")


@pytest.mark.gpu
def test_captured_cycles_give_the_bytes_of_eager_ones():
    """N = 32 on four levels: forward, backward and a Hessian-vector product with "graph" 0 and with captured cycles
    (`capture_worker`)"""
    assert "capture ok" in _torch_first("capture_worker")


@pytest.mark.gpu
def test_derivatives_of_the_singular_solve():
    """N = 8: backward against the host formulas, the Hessian-vector product against the host's and against central differences
    of device gradients, `tangent` against the host's and the directional derivative; n_solves grows by 1, 2 and 4
    (`derivatives_worker`)"""
    assert "derivatives ok" in _torch_first("derivatives_worker")


@pytest.mark.gpu
def test_regular_case_is_an_ordinary_solve():
    """sigma > 0; alpha > 0 on two faces only; `diffusion_nullspace` reports False; `solve_many` gives the bits of three solves;
    three implicit Euler steps with f = 0 conserve w.u (`regular_worker`)"""
    assert "regular ok" in _torch_first("regular_worker")


@pytest.mark.gpu
def test_refusals_leave_the_handle_untouched():
    """g given; solve_many, eigenpairs, mg_pcg_batch, mg_eigs, mg_fmg, Chebyshev and Gauss-Seidel in the singular case;
    set_diffusion_faces(0) on an insulated handle; 2-D and slab handles: each refused by name, and the next solve gives the bytes
    of the first (`refusals_worker`)"""
    assert "refusals ok" in _torch_first("refusals_worker")
