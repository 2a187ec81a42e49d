"""Smallest eigenpairs of the diffusion operator by multigrid LOBPCG (mg_eigs, mg_block_gram, mg_block_combine,
poisson.diffusion_eigs_reference).

CPU: the header, the binding and the library agree on the entries; the code object holds every block_gram and block_combine
instance the host can dispatch, without spills or scratch; csrc/mg_dense_eig.h under the sanitizers as a program of its own; the
host reference against the closed-form sine eigenvalues; the first-order formulas for d lambda / d(kappa, sigma, alpha, rho)
against central differences of the reference.
GPU: the bits and values of the two block kernels; mg_eigs against the closed form and against the host reference on
heterogeneous operators, stored and matrix-free; determinism, warm starts, the handle afterwards and the ledger."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from multigrid_dolfinx_amd import _capi, poisson
from tests.diffusion_eigs_workers import (CASES, EPS, closed_form_figures, eigs_hierarchy, gram_bound, heterogeneous_figures,
                                          level_handle, Lanes, longdouble_gram)
from tests.diffusion_reaction_workers import reaction_sigma
from tests.diffusion_robin_workers import robin_alpha
from tests.diffusion_workers import lognormal_kappa
from tests.pde_reference import sine_eigenvalue
from tests.test_diffusion_batch import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multigrid_dolfinx_amd", "libmg_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
ENTRIES = ("mg_eigs", "mg_block_gram", "mg_block_combine", "mg_eigs_info", "mg_release_eigs")

# 8 x the largest relative discrepancy the closed-form test observes (N = 16, kappa = 1.7, stored and matrix-free): the
# eigenvalues 5.9e-15, x[0] against the sine mode 1.1e-13, the (1,1,2) modes against their projection onto span(x[1:4]) 1.1e-9
CLOSED_LAMBDA_LIMIT = 8 * 5.9e-15
CLOSED_VECTOR_LIMIT = 8 * 1.1e-13
CLOSED_CLUSTER_LIMIT = 8 * 1.1e-9
# 8 x the largest relative discrepancy of lambda the heterogeneous cases observe against poisson.diffusion_eigs_reference
# (a: 1.1e-15, b: 1.7e-15, c: 4.7e-15, d: 3.4e-16)
HETEROGENEOUS_LAMBDA_LIMIT = 8 * 4.7e-15


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_eigs_entries():
    header = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _capi.SIGNATURES and getattr(lib, name).argtypes == _capi.SIGNATURES[name], name
    assert re.search(r"#define\s+MG_EIGS_MAX\s+8\b", code) and _capi.MG_EIGS_MAX == 8
    p, i, d = C.c_void_p, C.c_int, C.c_double
    assert _capi.SIGNATURES["mg_eigs"] == [p, i, i, i, p, p, i, d, i, p, p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert _capi.SIGNATURES["mg_block_gram"] == [p, i, i, p, i, p, p, p]
    assert _capi.SIGNATURES["mg_block_combine"] == [p, i, i, p, i, p, p]
    assert _capi.SIGNATURES["mg_eigs_info"] == [p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"), reason="needs the built library and ROCm's LLVM tools")
def test_block_kernels_are_in_the_code_object_within_their_resources():
    """block_gram<NA, NB, WEIGHTED> for NA, NB in 1..4 with and without the weight, block_combine<NS, NO> for NS in 1..24 and NO in
    1..8 -- what mg_block_gram / mg_block_combine dispatch over: no spilled VGPR, no scratch."""
    gram, combine = {}, {}
    for name, res in _kernel_notes().items():
        m = re.match(r"void mgk::block_gram<(\d+), (\d+), (true|false)>\(mgk::GramArgs\)", name)
        if m:
            gram[int(m.group(1)), int(m.group(2)), m.group(3) == "true"] = res
        m = re.match(r"void mgk::block_combine<(\d+), (\d+)>\(mgk::CombineArgs\)", name)
        if m:
            combine[int(m.group(1)), int(m.group(2))] = res
    assert sorted(gram) == sorted((a, b, w) for a in range(1, 5) for b in range(1, 5) for w in (False, True)), sorted(gram)
    assert sorted(combine) == sorted((s, o) for s in range(1, 25) for o in range(1, 9)), sorted(combine)
    for key, (spilled, scratch, group, vgpr) in sorted(gram.items()) + sorted(combine.items()):
        print(("block_gram" if len(key) == 3 else "block_combine"), key, "vgpr", vgpr, "lds", group)
        assert spilled == 0 and scratch == 0, (key, spilled, scratch)
        assert group <= 64 and vgpr <= 256, (key, group, vgpr)


def test_dense_eigen_solver_is_clean_under_sanitizers(tmp_path):
    """tests/host/dense_eig_check.cpp over csrc/mg_dense_eig.h, built and run as tests/test_devbuf_host.py builds and runs its
    program: the sanitizer runtime linked into the program, nothing preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "dense_eig_check")
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *static, "-o", exe,
                            os.path.join(ROOT, "tests", "host", "dense_eig_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dense eigen-solver clean" in run.stdout and "reported as failed" in run.stdout
    for case in ("order 1", "order 2", "order 3", "order 12", "order 24", "diagonal pair", "triple eigenvalue", "Gram pair 24"):
        assert case in run.stdout, case


def test_reference_equals_the_closed_form_sine_eigenvalues():
    """N = 8, kappa = 1.7, all six faces Dirichlet, k = 8: (1,1,1), the three permutations of (1,1,2), the three of (1,2,2) and
    (1,1,3), within 64 eps relative."""
    N, kappa = 8, 1.7
    lam, U = poisson.diffusion_eigs_reference(N, np.full(N ** 3, kappa), 8)
    want = np.array([sine_eigenvalue(N, m, kappa) for m in ((1, 1, 1), (1, 1, 2), (1, 1, 2), (1, 1, 2), (1, 2, 2), (1, 2, 2), (1, 2, 2), (1, 1, 3))])
    assert np.all(np.diff(want) >= 0.0)
    rel = np.abs(lam - want) / want
    print("largest relative difference %.3e" % rel.max())
    assert rel.max() <= 64 * EPS, rel
    m = poisson.reaction_diag(N, np.ones(N ** 3))
    gram = np.einsum("in,n,jn->ij", U, m, U)
    assert np.abs(gram - np.eye(8)).max() <= 1e-12 and not U[:, poisson.dirichlet_mask(N)].any()


def test_first_order_formulas_against_central_differences_of_the_reference():
    """d lambda_j = D(u_j, u_j) . dkappa, D_sigma(u_j, u_j) . dsigma, D_F(u_j, u_j) . dalpha, -lambda_j D_sigma(u_j, u_j) . drho for
    u^T M u = 1, for J = lambda_1 and J = sum_{j <= 4} lambda_j, N = 8, one Robin face (z+), a reaction field, a non-constant rho.

    Reference: central differences of `diffusion_eigs_reference` along one random direction per field, field + t * field * r with
    r uniform in [-1, 1], at t = 2e-2, 1e-2 and 5e-3.  Their truncation error is c t^2 (+ O(t^4)), their rounding error about
    eps |lambda| / t times a modest constant of the eigensolver (64 here): 1e-11 at these steps against 1e-5 of truncation, so
    the steps sit far on the truncation side of the balance t ~ eps^(1/3), on purpose -- the second-order behaviour is then
    visible and Richardson's extrapolation removes it: R(t) = (4 fd(t / 2) - fd(t)) / 3 is off by O(t^4).  Checked first:
    (fd(t) - fd(t/2)) / (fd(t/2) - fd(t/4)) within [3, 5] (4 for a pure t^2 term).  Then the formula against R(t / 2) with the
    limit |R(t) - R(t / 2)| + 64 eps |J| / (t / 4): the first term is 15 / 16 of R(t)'s own error and so bounds the sixteen times
    smaller error of R(t / 2) with a margin of 15."""
    N, faces, bit = 8, 63 - 32, 32
    rng = np.random.default_rng(11)
    base = {"kappa": lognormal_kappa(N, 3, seed=3), "sigma": reaction_sigma(N), "alpha": robin_alpha(N, bit),
            "rho": lognormal_kappa(N, 3, seed=5, sigma=0.5)}

    def eig(f):
        return poisson.diffusion_eigs_reference(N, f["kappa"], 4, rho=f["rho"], dirichlet_faces=faces, sigma=f["sigma"], robin={bit: f["alpha"]})

    lam, U = eig(base)
    formulas = {
        "kappa": lambda j: poisson.diffusion_dkappa(N, U[j], U[j], dirichlet_faces=faces),
        "sigma": lambda j: poisson.diffusion_dsigma(N, U[j], U[j], dirichlet_faces=faces),
        "alpha": lambda j: poisson.diffusion_drobin(N, bit, U[j], U[j], dirichlet_faces=faces),
        "rho": lambda j: -lam[j] * poisson.diffusion_dsigma(N, U[j], U[j], dirichlet_faces=faces),
    }
    for name in ("kappa", "sigma", "alpha", "rho"):
        d = base[name] * rng.uniform(-1.0, 1.0, base[name].size)
        fd = {}
        for t in (2e-2, 1e-2, 5e-3):
            lp, lm = eig(dict(base, **{name: base[name] + t * d}))[0], eig(dict(base, **{name: base[name] - t * d}))[0]
            fd[t] = (lp - lm) / (2 * t)
        for what, pick in (("lambda_1", lambda v: v[0]), ("sum of 4", lambda v: v.sum())):
            got = sum(float(formulas[name](j) @ d) for j in (range(1) if what == "lambda_1" else range(4)))
            f1, f2, f4 = pick(fd[2e-2]), pick(fd[1e-2]), pick(fd[5e-3])
            order = (f1 - f2) / (f2 - f4)
            r1, r2 = (4 * f2 - f1) / 3, (4 * f4 - f2) / 3
            limit = abs(r1 - r2) + 64 * EPS * abs(pick(lam)) / 5e-3
            print("%-5s %-9s formula %+.12e extrapolated %+.12e discrepancy %.3e limit %.3e order ratio %.3f"
                  % (name, what, got, r2, abs(got - r2), limit, order))
            assert 3.0 <= order <= 5.0, (name, what, order)
            assert abs(got - r2) <= limit, (name, what, got, r2, limit)


# ---- GPU: the two kernels -------------------------------------------------------------------------------------------------------
KERNEL_N = (8, 16, 32)          # 729 and 4913 rows are odd (the scalar tail), 35937 rows take more than one block


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
def test_block_gram_bits_and_values(N):
    """(na, nb) in {(1,1), (4,4), (5,3), (9,9) symmetric}, with and without the weight: every entry has the bits of the 1 x 1 call
    on that pair, the mirrored entries of the symmetric call equal the computed ones, two calls give the same bytes, and every
    entry is within n eps sum |a_i d b_j| of a longdouble dot."""
    n = (N + 1) ** 3
    rng = np.random.default_rng(N)
    vec = rng.standard_normal((12, n))
    weight = rng.uniform(0.5, 2.0, n)
    with level_handle(N) as h, Lanes(h, list(vec) + [weight]) as V:
        for weighted in (False, True):
            d_ptr, d = (V.ptrs[12], weight) if weighted else (None, None)
            pair = {}

            def single(i, j):
                if (i, j) not in pair:
                    pair[i, j] = h.block_gram([V.ptrs[i]], [V.ptrs[j]], d_ptr, level=1)[0, 0]
                return pair[i, j]

            for rows, cols in (([0], [1]), ([0, 1, 2, 3], [4, 5, 6, 7]), ([0, 1, 2, 3, 4], [5, 6, 7]), (list(range(9)), list(range(9)))):
                G = h.block_gram([V.ptrs[i] for i in rows], [V.ptrs[j] for j in cols], d_ptr, level=1)
                assert G.tobytes() == h.block_gram([V.ptrs[i] for i in rows], [V.ptrs[j] for j in cols], d_ptr, level=1).tobytes()
                symmetric = rows == cols
                want = longdouble_gram(vec[rows], vec[cols], d)
                bound = gram_bound(vec[rows], vec[cols], d)
                worst = float((np.abs(G - want) / bound).max())
                print("N %d weighted %s shape %s: largest error / bound %.3e" % (N, weighted, (len(rows), len(cols)), worst))
                assert worst <= 1.0, (N, weighted, rows, cols, worst)
                for a, i in enumerate(rows):
                    for b, j in enumerate(cols):
                        if symmetric and a > b:
                            assert G[a, b].tobytes() == G[b, a].tobytes(), (N, weighted, a, b)
                        else:
                            assert G[a, b].tobytes() == single(i, j).tobytes(), (N, weighted, len(rows), len(cols), a, b)
        for got, host in zip(V.download(), list(vec) + [weight]):
            assert got.tobytes() == host.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("N", KERNEL_N)
def test_block_combine_values_and_in_place(N):
    """(ns, no) in {(2,1), (12,4), (18,6), (24,8)}: within ns eps sum_i |c_i s_i| per entry of a longdouble restatement; with every
    output aliased to one of the inputs the bytes of the out-of-place call."""
    n = (N + 1) ** 3
    rng = np.random.default_rng(100 + N)
    src = rng.standard_normal((24, n))
    with level_handle(N) as h:
        for ns, no in ((2, 1), (12, 4), (18, 6), (24, 8)):
            coeff = rng.standard_normal((ns, no))
            want = (coeff.astype(np.longdouble).T @ src[:ns].astype(np.longdouble))
            bound = ns * EPS * (np.abs(coeff).T @ np.abs(src[:ns]))
            with Lanes(h, list(src[:ns])) as S, Lanes(h, [np.full(n, np.nan)] * no) as O:
                h.block_combine(S.ptrs, coeff, O.ptrs, level=1)
                out = np.stack(O.download())
                for got, host in zip(S.download(), src[:ns]):
                    assert got.tobytes() == host.tobytes()
                worst = float((np.abs(out - want) / bound).max())
                print("N %d (ns, no) = (%d, %d): largest error / bound %.3e" % (N, ns, no, worst))
                assert worst <= 1.0, (N, ns, no, worst)
                # output o is input (3 o + 1) % ns: in place
                alias = [(3 * o + 1) % ns for o in range(no)]
                assert len(set(alias)) == no
                h.block_combine(S.ptrs, coeff, [S.ptrs[i] for i in alias], level=1)
                after = S.download()
                for o, i in enumerate(alias):
                    assert after[i].tobytes() == out[o].tobytes(), (N, ns, no, o)
                for i in set(range(ns)) - set(alias):
                    assert after[i].tobytes() == src[i].tobytes()


@pytest.mark.gpu
def test_block_kernel_refusals():
    N = 8
    n = (N + 1) ** 3
    with level_handle(N) as h, Lanes(h, [np.ones(n + 2)] * 3) as V:
        with pytest.raises(_capi.MgError, match="16-byte aligned"):
            h.block_gram([V.ptrs[0] + 8], [V.ptrs[1]], level=1)
        with pytest.raises(_capi.MgError, match="not device memory|null pointer"):
            h.block_gram([V.ptrs[0]], [0], level=1)
        with pytest.raises(_capi.MgError, match=r"1\.\.24"):
            h.block_gram([V.ptrs[0]] * 25, [V.ptrs[1]], level=1)
        with pytest.raises(_capi.MgError, match=r"1\.\.8"):
            h.block_combine([V.ptrs[0]], np.ones((1, 9)), [V.ptrs[1]] * 9, level=1)
        with pytest.raises(_capi.MgError, match="overlaps s_dev"):
            h.block_combine([V.ptrs[0]], np.ones((1, 1)), [V.ptrs[0] + 16], level=1)
        with pytest.raises(_capi.MgError, match="overlaps out_dev"):
            h.block_combine([V.ptrs[0]], np.ones((1, 2)), [V.ptrs[1], V.ptrs[1]], level=1)


# ---- GPU: mg_eigs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("matrix_free", [False, True], ids=["stored", "matrix-free"])
def test_eigs_against_the_closed_form(matrix_free):
    """kappa = 1.7, N = 16 on three levels, all six faces Dirichlet, k = 4, block = 6, rtol 1e-8, Jacobi V(2,2), P1 transfers:
    lambda[0:4] against `sine_eigenvalue` of (1,1,1) and the triple (1,1,2), x[0] against the M-normalised sine mode up to sign,
    each (1,1,2) sine mode against its M-orthogonal projection onto span(x[1:4]).

    Observed on the MI355X (stored and matrix-free alike, 19 iterations, no restart): eigenvalues 5.9e-15 relative (5.806e-15),
    x[0] 1.1e-13 (1.026e-13), the cluster 1.1e-9 (1.093e-9: the vectors stop at residuals of 1e-9 .. 3e-9); the limits are 8 x
    these."""
    fig = closed_form_figures(matrix_free)
    assert fig["resid"][:4].max() <= 1e-8 and fig["iterations"] < 100, fig
    assert fig["lambda_rel"] <= 1e-10, "an eigenvalue discrepancy above 1e-10 is a defect: %r" % fig
    assert fig["lambda_rel"] <= CLOSED_LAMBDA_LIMIT, fig
    assert fig["vector_rel"] <= CLOSED_VECTOR_LIMIT, fig
    assert fig["cluster_rel"] <= CLOSED_CLUSTER_LIMIT, fig


@pytest.mark.gpu
@pytest.mark.parametrize("case,matrix_free", [("a", False), ("a", True), ("b", True), ("c", True), ("d", True)],
                         ids=["a-stored", "a-matrix-free", "b", "c", "d"])
def test_eigs_against_the_host_reference(case, matrix_free):
    """lognormal_kappa(N, 3, seed=3) in the four settings of CASES against `poisson.diffusion_eigs_reference`: the first k
    residuals <= rtol = 1e-8 in fewer than 100 iterations (observed: 22, 22, 22 and 21, no restart), lambda within 8 x the largest
    relative discrepancy observed (4.7e-15: a 1.018e-15, b 1.684e-15, c 4.662e-15, d 3.346e-16),
    |X^T M X - I| over the whole block (by block_gram) within the rounding bound n eps sum |x_i m x_j|, every vector exactly +0.0
    on the Dirichlet nodes."""
    fig = heterogeneous_figures(case, matrix_free)
    k = CASES[case]["k"]
    assert fig["resid"][:k].max() <= 1e-8 and fig["iterations"] < 100, fig
    assert fig["lambda_rel"] <= HETEROGENEOUS_LAMBDA_LIMIT, fig
    assert fig["orthonormality_over_bound"] <= 1.0, fig
    assert fig["dirichlet_bytes_zero"], fig


@pytest.mark.gpu
def test_eigs_is_deterministic_and_leaves_the_handle_as_it_was():
    """Case a twice from a cold start: the same bytes of lambda and X.  A third call warm from the result: 0 iterations, lambda
    within 4 ulp.  mg_pcg afterwards: the bytes of a handle that never ran mg_eigs.  The ledger: up by the work vectors (and the
    lanes), back after release_eigs (and release_batch)."""
    cs = CASES["a"]
    N, top = cs["N"], cs["levels"] - 1
    n = (N + 1) ** 3
    rhs = np.random.default_rng(5).standard_normal(n)

    def plain_pcg(h):
        h.set_vector(top, "f", rhs)
        h.zero_vector(top, "v")
        hist = h.pcg(1e-9, 40, top)
        return hist.tobytes(), h.get_vector(top, "v").tobytes()

    with eigs_hierarchy("a", True) as fresh, eigs_hierarchy("a", True) as h:
        want = plain_pcg(fresh)
        assert plain_pcg(h) == want
        before = h.memory_bytes()
        assert h.eigs_info() == {"block": 0, "bytes": 0}
        with Lanes(h, [np.full(n, np.nan)] * cs["block"]) as X:
            first = h.eigs(cs["k"], cs["block"], x_ptrs=X.ptrs, rtol=1e-8, max_iter=100, level=top)
            x1 = X.download()
            info, lanes = h.eigs_info(), h.batch_info()
            assert info["block"] == cs["block"] and info["bytes"] > 0 and lanes["lanes"] == cs["block"] - 1
            assert h.memory_bytes() == before + info["bytes"] + lanes["bytes"], (before, info, lanes, h.memory_bytes())
            with Lanes(h, [np.full(n, np.nan)] * cs["block"]) as Y:
                second = h.eigs(cs["k"], cs["block"], x_ptrs=Y.ptrs, rtol=1e-8, max_iter=100, level=top)
                x2 = Y.download()
            assert first["lambda"].tobytes() == second["lambda"].tobytes() and first["iterations"] == second["iterations"]
            assert all(a.tobytes() == b.tobytes() for a, b in zip(x1, x2))
            assert h.eigs_info() == info
            third = h.eigs(cs["k"], cs["block"], x_ptrs=X.ptrs, warm=True, rtol=1e-8, max_iter=100, level=top)
            ulps = np.abs(third["lambda"][:cs["k"]] - second["lambda"][:cs["k"]]) / np.spacing(second["lambda"][:cs["k"]])
            print("warm: iterations", third["iterations"], "ulps", ulps, "cold iterations", first["iterations"], "restarts", first["restarts"])
            assert third["iterations"] == 0 and ulps.max() <= 4, (third, ulps)
        assert plain_pcg(h) == want
        h.release_eigs()
        assert h.eigs_info() == {"block": 0, "bytes": 0} and h.memory_bytes() == before + h.batch_info()["bytes"]
        h.release_batch()
        assert h.memory_bytes() == before
        assert plain_pcg(h) == want


@pytest.mark.gpu
def test_eigs_refusals_leave_the_handle_as_it_was():
    cs = CASES["a"]
    N, top = cs["N"], cs["levels"] - 1
    n = (N + 1) ** 3
    with eigs_hierarchy("a", True) as h, Lanes(h, [np.zeros(n + 4)] * 3) as X:
        before = h.memory_bytes()
        rho = np.ones(N ** 3)
        rho[(2 * N + 1) * N + 3] = 0.0
        for kwargs, text in ((dict(k=0, block=2), "k = 0"), (dict(k=3, block=2), "k = 3"), (dict(k=1, block=9), "MG_EIGS_MAX"),
                             (dict(k=1, block=2, rtol=0.0, max_iter=0), "nothing would stop"),
                             (dict(k=1, block=2, level=0), "level 0"),
                             (dict(k=1, block=2, rho=rho), r"rho must be finite and positive: cell \(3, 1, 2\)"),
                             (dict(k=1, block=2, rho=np.where(rho > 0, rho, np.nan)), r"cell \(3, 1, 2\)")):
            kw = dict(dict(level=top), **kwargs)
            with pytest.raises(_capi.MgError, match=text):
                h.eigs(kw.pop("k"), kw.pop("block"), x_ptrs=X.ptrs[:kwargs["block"]] if kwargs["block"] <= 3 else [X.ptrs[0]] * 9, **kw)
        with pytest.raises(_capi.MgError, match="overlaps"):
            h.eigs(1, 2, x_ptrs=[X.ptrs[0], X.ptrs[0] + 8], level=top)
        with pytest.raises(_capi.MgError, match="not device memory|null pointer"):
            h.eigs(1, 2, x_ptrs=[X.ptrs[0], 0], level=top)
        assert h.memory_bytes() == before and h.eigs_info() == {"block": 0, "bytes": 0} and h.batch_info()["lanes"] == 0


# ---- GPU: DiffusionSolver.eigenpairs (torch in a worker process, as the other diffusion tests run it) -------------------------------
# 8 x the largest relative discrepancies the worker observes: lam against the host reference 4.2e-15 (4.193e-15), the gradients of
# lambda_1 (3.6e-14 and below) and of the sum of four (7.7e-12: 7.613e-12 for kappa, 5.1e-12 .. 5.9e-12 for the others; the sum's
# vectors stop at residuals of 1e-11 .. 1e-10) against the host formulas at the reference's eigenvectors, relative l2
EIGENPAIRS_LAMBDA_LIMIT = 8 * 4.2e-15
EIGENPAIRS_GRADIENT_LIMIT = 8 * 7.7e-12


@pytest.mark.gpu
def test_eigenpairs_values_signs_and_first_order_gradients():
    """N = 16 on two levels, rtol 1e-10, one Robin face, a reaction field, a non-constant rho: lam and the sign rule of U, the
    gradients of lambda_1 and of the sum of four with respect to kappa, sigma, alpha(z+) and rho against the host formulas evaluated
    with `diffusion_eigs_reference`; a second differentiation raises; a warm start; NotConverged."""
    import sys
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_eigs_workers as w; w.eigenpairs_worker(%r, %r)" % (
        ROOT, EIGENPAIRS_LAMBDA_LIMIT, EIGENPAIRS_GRADIENT_LIMIT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert "eigenpairs ok" in out.stdout
