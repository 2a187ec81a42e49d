"""Dirichlet data as a differentiable input of the diffusion solves: the sensitivity operators with a node set per side,
T(w, x; rows, cols) = M_rows A^(w) M_cols x (mg_diffusion_apply_dkappa_ex) and D(a, b; A, B) = d/dw (M_A a)^T A^(w) (M_B b)
(mg_diffusion_dkappa_ex), their host restatements and the natural matrix A^ of poisson.py, and DiffusionSolver.solve /
tangent with g against host references built on scipy's spsolve (tests/diffusion_dirichlet_workers.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from multigrid_dolfinx_amd import poisson
from tests.diffusion_dirichlet_workers import (PAIRS, boundary_part, host_adjoint_g, host_hessian_vector_g, host_solve_g, inner_mask,
                                               mask_of, natural_row_bound, natural_row_terms)
from tests.diffusion_workers import lognormal_kappa

EPS = np.finfo(np.float64).eps
SETS = {"interior": 0, "all": 1}


def _within(bound, got, want, what):
    """|got - want| <= bound per row; prints the largest ratio of error to bound."""
    err = np.abs(got - want)
    some = bound > 0.0
    print(what, "largest error / bound", float((err[some] / bound[some]).max()) if some.any() else 0.0, "largest error", float(err.max()),
          "rows with a bound", int(some.sum()))
    assert np.all(err <= bound), (what, int(np.argmax(err - bound)))


def _t_identity(N, w, y, x, rows, cols, Tyx, Txy, what):
    """y . T(w, x; R, C) = x . T(w, y; C, R) to 64 eps times the sum of the absolute values of the terms of both sides."""
    lhs, rhs = float(y @ Tyx), float(x @ Txy)
    bound = 64 * EPS * (float((np.abs(y) * np.abs(natural_row_terms(N, w, x, rows, cols))).sum()) +
                        float((np.abs(x) * np.abs(natural_row_terms(N, w, y, cols, rows))).sum()))
    print(what, rows, cols, "lhs", lhs, "rhs", rhs, "difference", abs(lhs - rhs), "bound", bound)
    assert abs(lhs - rhs) <= bound, (what, rows, cols)


def _d_identity(N, w, D, a, x, T, a_nodes, b_nodes, what):
    """w . D(a, x; A, B) = (M_A a) . T(w, x; A, B) to the 64 eps bound of test_diffusion_tangent._adjoint_identity: the cells'
    products on the left, the products of the rows' entries on the right."""
    am = a * mask_of(N, a_nodes)
    lhs_terms = w * D
    lhs, rhs = float(lhs_terms.sum()), float(am @ T)
    bound = 64 * EPS * (float(np.abs(lhs_terms).sum()) + float((np.abs(am) * np.abs(natural_row_terms(N, w, x, a_nodes, b_nodes))).sum()))
    print(what, a_nodes, b_nodes, "lhs", lhs, "rhs", rhs, "difference", abs(lhs - rhs), "bound", bound)
    assert abs(lhs - rhs) <= bound, (what, a_nodes, b_nodes)


# ---- host --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 8])
def test_host_operators_against_the_natural_matrix(N):
    """For all four pairs, standard-normal w, a, x with non-zero boundary entries: T(w, x; R, C) = M_R A^(w) M_C x within the
    per-row bound and w . D(a, x; A, B) = (M_A a) . A^(w) (M_B x) to 64 eps times the sum of the absolute terms; A^ 1 = 0."""
    rng = np.random.default_rng(60 + N)
    w, a, x = rng.standard_normal(N ** 3), rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    A = poisson.diffusion_natural_matrix(N, w)
    assert A.shape == ((N + 1) ** 3,) * 2 and A.has_sorted_indices and abs(A - A.T).max() == 0.0
    for rows, cols in PAIRS:
        T = poisson.diffusion_apply_dkappa(N, w, x, rows, cols)
        _within(natural_row_bound(N, w, x, rows, cols), T, mask_of(N, rows) * (A @ (mask_of(N, cols) * x)), f"T {rows} {cols}")
        if rows == "interior":
            assert not T[~inner_mask(N)].any()
        D = poisson.diffusion_dkappa(N, a, x, rows, cols)
        am, xm = a * mask_of(N, rows), x * mask_of(N, cols)
        rhs = float(am @ (A @ xm))
        bound = 64 * EPS * (float(np.abs(w * D).sum()) + float(np.abs(am) @ (abs(A) @ np.abs(xm))))
        print("D", rows, cols, "difference", abs(float(w @ D) - rhs), "bound", bound)
        assert abs(float(w @ D) - rhs) <= bound
    ones = np.ones((N + 1) ** 3)
    _within(natural_row_bound(N, w, ones, "all", "all"), A @ ones, np.zeros_like(ones), "A^ 1")
    _within(natural_row_bound(N, w, ones, "all", "all"), poisson.diffusion_apply_dkappa(N, w, ones, "all", "all"), np.zeros_like(ones), "T(w, 1)")


@pytest.mark.parametrize("N", [6, 8])
def test_host_defaults_and_node_set_names(N):
    """The keywords default to (interior, interior), which ignores the boundary entries; any other name is refused."""
    rng = np.random.default_rng(70 + N)
    w, a, x = rng.standard_normal(N ** 3), rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    inner = inner_mask(N)
    assert poisson.diffusion_dkappa(N, a, x).tobytes() == poisson.diffusion_dkappa(N, a, x, "interior", "interior").tobytes()
    assert poisson.diffusion_dkappa(N, a, x).tobytes() == poisson.diffusion_dkappa(N, a * inner, x * inner, "all", "all").tobytes()
    assert poisson.diffusion_apply_dkappa(N, w, x).tobytes() == poisson.diffusion_apply_dkappa(N, w, x, rows="interior", cols="interior").tobytes()
    for call in (lambda: poisson.diffusion_dkappa(N, a, x, "boundary", "all"), lambda: poisson.diffusion_dkappa(N, a, x, "all", 1),
                 lambda: poisson.diffusion_apply_dkappa(N, w, x, "inner", "all"), lambda: poisson.diffusion_apply_dkappa(N, w, x, cols=None)):
        with pytest.raises(ValueError, match="'interior' or 'all'"):
            call()


@pytest.mark.parametrize("N", [6, 8])
def test_natural_matrix_and_lift_against_the_assembled_level(N):
    """A^(kappa)'s interior block is diffusion_level's to 4 eps max |a_ij| (the adds come in another order), and the lift of
    boundary_data is what diffusion_level folds into its right-hand side: source_term h^3 - b on interior rows, within the
    row bound."""
    kappa = lognormal_kappa(N, 3, seed=N)
    lev = poisson.diffusion_level(N, 3, kappa)
    inner = inner_mask(N)
    I = np.flatnonzero(inner)
    A = poisson.diffusion_natural_matrix(N, kappa)
    diff = abs(A[I][:, I] - lev.A[I][:, I]).max()
    print("interior block: largest difference", diff, "limit", 4 * EPS * abs(lev.A).max())
    assert diff <= 4 * EPS * abs(lev.A[I][:, I]).max()
    g = poisson.boundary_data(lev.coords, 3)
    lift = poisson.diffusion_lift(N, kappa, g)
    assert not lift[~inner].any()
    want = np.where(inner, poisson.source_term(3) * lev.h ** 3 - lev.b.reshape(-1), 0.0)
    _within(natural_row_bound(N, kappa, boundary_part(N, g), "interior", "all"), lift, want, "lift against the level's right-hand side")
    # only the boundary entries of g are read
    assert poisson.diffusion_lift(N, kappa, boundary_part(N, g)).tobytes() == lift.tobytes()


def _host_case():
    N = 6
    rng = np.random.default_rng(3)
    kappa = np.exp(rng.standard_normal(N ** 3))
    f, d, g = (rng.standard_normal((N + 1) ** 3) for _ in range(3))
    return N, kappa, f, d, g


def _relative_direction(kappa, seed):
    v = np.random.default_rng(seed).standard_normal(kappa.size) * kappa
    return v / np.abs(v / kappa).max()


def test_host_adjoint_gradient_with_dirichlet_data_against_finite_differences():
    """J = 1/2 ||u - d||^2 at N = 6 with spsolve of the lifted system, random f and g.  Along three directions that move kappa
    (relative, |v / kappa| <= 1) and the boundary data together the discrepancy between (dJ/dkappa, dJ/dg) . direction and central
    differences falls by a factor between 3 and 5 from step 0.01 to 0.005, the band of
    test_host_adjoint_gradient_against_finite_differences; so it does along kappa alone.  J is exactly quadratic in g, so along g
    alone central differences have no truncation error and the discrepancy is the round-off of the quotient: at most
    1e-10 J / step (the solve's relative error, about cond(A) eps = 1e-13, with a margin of 1000).  The gradient with both
    arguments masked, -D(lambda~, u~), misses the true one by more than 1 % in l2: the test cannot pass without the lift."""
    N, kappa, f, d, g = _host_case()
    eps = 0.01
    J = lambda k, gv: 0.5 * float(np.sum((host_solve_g(N, k, f, gv) - d) ** 2))
    J0, u, gk, _, gg, lam = host_adjoint_g(N, kappa, f, g, d)
    assert not gg[inner_mask(N)].any()
    for t in range(3):
        v = _relative_direction(kappa, 10 + t)
        vg = boundary_part(N, np.random.default_rng(20 + t).standard_normal((N + 1) ** 3))
        for what, (sk, sg) in (("kappa and g", (1.0, 1.0)), ("kappa", (1.0, 0.0))):
            want = sk * (gk @ v) + sg * (gg @ vg)
            err = [abs((J(kappa + sk * s * v, g + sg * s * vg) - J(kappa - sk * s * v, g - sg * s * vg)) / (2 * s) - want) for s in (eps, eps / 2)]
            print("direction", t, what, "gradient . direction", want, "discrepancies", err, "ratio", err[0] / err[1])
            assert 3.0 <= err[0] / err[1] <= 5.0, (t, what, err)
        for s in (eps, eps / 2):
            err = abs((J(kappa, g + s * vg) - J(kappa, g - s * vg)) / (2 * s) - gg @ vg)
            print("direction", t, "g alone, step", s, "dJ/dg . direction", gg @ vg, "discrepancy", err, "limit", 1e-10 * J0 / s)
            assert err <= 1e-10 * J0 / s, (t, s, err)
    masked = -poisson.diffusion_dkappa(N, lam, u)
    miss = float(np.linalg.norm(masked - gk) / np.linalg.norm(gk))
    print("both arguments masked: relative l2 distance to the gradient", miss)
    assert miss > 0.01
    # the interior entries of g do not count
    assert host_solve_g(N, kappa, f, boundary_part(N, g)).tobytes() == u.tobytes()


def test_host_hessian_vector_product_with_dirichlet_data_against_finite_differences():
    """The four-solve product of host_hessian_vector_g at N = 6 against central differences of host_adjoint_g's gradients along
    three relative directions of kappa: the kappa, f and g blocks each fall by a factor between 3 and 5 from step 0.01 to 0.005."""
    N, kappa, f, d, g = _host_case()
    eps = 0.01
    grads = lambda k: host_adjoint_g(N, k, f, g, d)[2:5]
    for t in range(3):
        v = _relative_direction(kappa, 10 + t)
        blocks = host_hessian_vector_g(N, kappa, f, g, d, v)
        fd = {s: [(p - m) / (2 * s) for p, m in zip(grads(kappa + s * v), grads(kappa - s * v))] for s in (eps, eps / 2)}
        for name, want, i in (("kappa", blocks[0], 0), ("f", blocks[1], 1), ("g", blocks[2], 2)):
            err = [float(np.linalg.norm(fd[s][i] - want)) for s in (eps, eps / 2)]
            print("direction", t, name, "block", float(np.linalg.norm(want)), "discrepancies", err, "ratio", err[0] / err[1])
            assert 3.0 <= err[0] / err[1] <= 5.0, (t, name, err)


# ---- device: the kernels --------------------------------------------------------------------------------------------------------
SHAPES = [8, 36, 64, 128]       # less than a tile; partial tiles; the boundary column alone in a second tile column; several z segments


@functools.lru_cache(maxsize=None)
def _kernel_case(N):
    """Operands with non-zero boundary entries and the host restatements for every pair, computed once."""
    rng = np.random.default_rng(300 + N)
    x, a = rng.standard_normal((N + 1) ** 3), rng.standard_normal((N + 1) ** 3)
    w = rng.standard_normal(N ** 3)
    w[rng.random(N ** 3) < 0.1] = 0.0
    kappa = lognormal_kappa(N, 3, seed=1)
    case = {"w": w, "x": x, "a": a, "kappa": kappa,
            "T": {p: poisson.diffusion_apply_dkappa(N, w, x, *p) for p in PAIRS},
            "D": {p: poisson.diffusion_dkappa(N, a, x, *p) for p in PAIRS}}
    for v in (w, x, a, kappa, *case["T"].values(), *case["D"].values()):
        v.setflags(write=False)
    return case


def _levels(N, kappa):
    from tests.test_diffusion_tangent import _levels as levels
    return levels(N, kappa)


class _Device:
    """Device copies of host arrays on a handle and the four entries by pointer; frees what it allocated."""

    def __init__(self, h):
        self.h, self.held = h, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.held:
            b.free()

    def array(self, n, host=None):
        from multigrid_dolfinx_amd.hierarchy import _DeviceArray
        self.held.append(_DeviceArray(self.h._lib, self.h.device, n, None if host is None else np.ascontiguousarray(host, dtype=np.float64)))
        return self.held[-1]

    def T_ex(self, w, x, rows, cols):
        """mg_diffusion_apply_dkappa_ex itself, (interior, interior) included."""
        from multigrid_dolfinx_amd._capi import check
        out = self.array(self.h.n_dofs(1))
        check(self.h._lib.mg_diffusion_apply_dkappa_ex(self.h._h, self.h._idx(1), w.ptr, x.ptr, SETS[rows], SETS[cols], out.ptr))
        return out.download()

    def D_ex(self, a, b, a_nodes, b_nodes):
        from multigrid_dolfinx_amd._capi import check
        out = self.array(self.h.elements(1) ** 3)
        check(self.h._lib.mg_diffusion_dkappa_ex(self.h._h, self.h._idx(1), a.ptr, SETS[a_nodes], b.ptr, SETS[b_nodes], out.ptr))
        return out.download()


@pytest.mark.gpu
@pytest.mark.parametrize("N", SHAPES)
def test_interior_sets_through_the_new_entries_are_the_old_entries(N):
    """(interior, interior) through mg_diffusion_apply_dkappa_ex and mg_diffusion_dkappa_ex (march and gather) equals
    mg_diffusion_apply_dkappa and mg_diffusion_dkappa byte for byte, on a stored, a matrix-free and a grid-only level."""
    case = _kernel_case(N)
    for name, h in _levels(N, case["kappa"]):
        with _Device(h) as dev:
            w, x, a = dev.array(N ** 3, case["w"]), dev.array((N + 1) ** 3, case["x"]), dev.array((N + 1) ** 3, case["a"])
            assert dev.T_ex(w, x, "interior", "interior").tobytes() == h.diffusion_apply_dkappa(1, case["w"], case["x"]).tobytes(), name
            for gather in (0, 1):
                h.set_tuning("dkappa_gather", gather)
                assert dev.D_ex(a, x, "interior", "interior").tobytes() == h.diffusion_dkappa(1, case["a"], case["x"]).tobytes(), (name, gather)
                assert dev.D_ex(a, a, "interior", "interior").tobytes() == h.diffusion_dkappa(1, case["a"], case["a"]).tobytes(), (name, gather)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SHAPES)
def test_sensitivity_with_node_sets_carries_the_bits_of_the_restatement(N):
    """D for every pair equals poisson.diffusion_dkappa byte for byte, as the plane march and as the gather, whatever the
    level's kind; one device pointer passed as a and b with the sets (interior, all) gives what two buffers give."""
    case = _kernel_case(N)
    aa = poisson.diffusion_dkappa(N, case["a"], case["a"], "interior", "all")
    assert aa.tobytes() != poisson.diffusion_dkappa(N, case["a"], case["a"]).tobytes()
    for name, h in _levels(N, case["kappa"]):
        for gather in (0, 1):
            h.set_tuning("dkappa_gather", gather)
            for pair in PAIRS:
                got = h.diffusion_dkappa(1, case["a"], case["x"], a_nodes=pair[0], b_nodes=pair[1])
                bad = np.flatnonzero(got != case["D"][pair])
                assert got.tobytes() == case["D"][pair].tobytes(), (name, gather, pair, bad[:5], bad.size)
            a = case["a"]
            one_pointer = h.diffusion_dkappa(1, a, a, a_nodes="interior", b_nodes="all")
            two_buffers = h.diffusion_dkappa(1, a, a.copy(), a_nodes="interior", b_nodes="all")
            assert one_pointer.tobytes() == two_buffers.tobytes() == aa.tobytes(), (name, gather)
            assert h.diffusion_dkappa(1, a, a, a_nodes="all", b_nodes="all").tobytes() == \
                poisson.diffusion_dkappa(N, a, a, "all", "all").tobytes(), (name, gather)


@pytest.mark.gpu
@pytest.mark.parametrize("N", SHAPES)
def test_tangent_with_node_sets(N):
    """T for every pair: within the row bound of the restatement; rows outside `rows` exactly +0.0 although x is not;
    T(-w, x) = -T(w, x) to the bit; the level's kind does not matter; T(w, 1; all, all) within the bound of 0."""
    case = _kernel_case(N)
    w, x = case["w"], case["x"]
    assert np.all(x != 0.0)
    inner = inner_mask(N)
    ones = np.ones((N + 1) ** 3)
    first = {}
    for name, h in _levels(N, case["kappa"]):
        for pair in PAIRS:
            T = h.diffusion_apply_dkappa(1, w, x, rows=pair[0], cols=pair[1])
            assert np.array_equal(h.diffusion_apply_dkappa(1, -w, x, rows=pair[0], cols=pair[1]), -T), (name, pair)
            if pair not in first:
                first[pair] = T
                _within(natural_row_bound(N, w, x, *pair), T, case["T"][pair], f"device against the restatement {pair} N {N}")
                if pair[0] == "interior":
                    assert T[~inner].tobytes() == np.zeros(int((~inner).sum())).tobytes(), pair
                else:       # (cols = interior: only a face's inner nodes have an interior neighbour)
                    filled = 6 * (N - 1) ** 2 if pair[1] == "interior" else int((~inner).sum())
                    assert 0.9 * filled <= np.count_nonzero(T[~inner]) <= filled, pair
            assert T.tobytes() == first[pair].tobytes(), (name, pair)
        if name == "poisson":
            _within(natural_row_bound(N, w, ones, "all", "all"), h.diffusion_apply_dkappa(1, w, ones, rows="all", cols="all"),
                    np.zeros_like(ones), f"T(w, 1; all, all) N {N}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", SHAPES)
def test_adjoint_identities_on_the_device(N):
    """w . D(a, x; A, B) = (M_A a) . T(w, x; A, B) and y . T(w, x; R, C) = x . T(w, y; C, R) with both sides from the device, to
    the 64 eps bound of test_diffusion_tangent._adjoint_identity."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    case = _kernel_case(N)
    w, x, a = case["w"], case["x"], case["a"]
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_poisson_level(1)
        for pair in PAIRS:
            T = h.diffusion_apply_dkappa(1, w, x, rows=pair[0], cols=pair[1])
            _d_identity(N, w, h.diffusion_dkappa(1, a, x, a_nodes=pair[0], b_nodes=pair[1]), a, x, T, pair[0], pair[1], f"device N {N}")
            _t_identity(N, w, a, x, pair[0], pair[1], T, h.diffusion_apply_dkappa(1, w, a, rows=pair[1], cols=pair[0]), f"device N {N}")


@pytest.mark.gpu
@pytest.mark.parametrize("N", SHAPES)
def test_lift_against_the_generated_right_hand_side(N):
    """T(kappa, g_B; interior, all) with g = boundary_data equals source_term h^3 - MG_VEC_F of mg_gen_diffusion_level with that
    kappa on interior rows, within the row bound: the level's right-hand side comes from gen_diffusion / gen_diffusion_rhs,
    which share no code with the tangent march."""
    kappa = _kernel_case(N)["kappa"]
    n1 = N + 1
    idx = np.arange(n1 ** 3)
    coords = np.stack([idx % n1, (idx // n1) % n1, idx // (n1 * n1)], axis=1) / N
    g_b = boundary_part(N, poisson.boundary_data(coords, 3))
    inner = inner_mask(N)
    bound = natural_row_bound(N, kappa, g_b, "interior", "all")
    for name, h in _levels(N, kappa):
        if name == "poisson":
            continue
        F = h.get_vector(1, "f").reshape(-1)
        assert np.array_equal(F[~inner], g_b[~inner]), name
        lift = h.diffusion_apply_dkappa(1, kappa, g_b, rows="interior", cols="all")
        _within(bound, lift, np.where(inner, poisson.source_term(3) * (1.0 / N) ** 3 - F, 0.0), f"lift against MG_VEC_F, {name} N {N}")


@pytest.mark.gpu
def test_refusals_of_the_new_entries_name_their_cause():
    """Every refusal of the two entries without node sets, and a node set other than 0 or 1, by message; nothing is launched:
    the handle's vectors and counters are unchanged."""
    from multigrid_dolfinx_amd._capi import MgError, check
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 32
    n = (N + 1) ** 3
    with DeviceHierarchy(3, 0, 1, c=16) as h, _Device(h) as dev:
        h.gen_diffusion_level(1, np.ones(N ** 3), matrix_free=True)
        k, p, o = (dev.array(m, np.zeros(m)).ptr.value for m in (n, n, 2 * n))
        host = np.zeros(n).ctypes.data
        h.set_vector(1, "v", np.arange(n, dtype=np.float64))
        before = h.get_vector(1, "v").copy()
        counters = h.counters()
        T = lambda hh, level, w, x, out, rows=1, cols=1: check(hh._lib.mg_diffusion_apply_dkappa_ex(
            hh._h, hh._idx(level), C.c_void_p(w), C.c_void_p(x), rows, cols, C.c_void_p(out)))
        D = lambda hh, level, a, b, out, a_nodes=1, b_nodes=1: check(hh._lib.mg_diffusion_dkappa_ex(
            hh._h, hh._idx(level), C.c_void_p(a), a_nodes, C.c_void_p(b), b_nodes, C.c_void_p(out)))
        for entry, who in ((T, "mg_diffusion_apply_dkappa_ex"), (D, "mg_diffusion_dkappa_ex")):
            for args in ((host, p, o), (k, host, o), (k, p, host)):
                with pytest.raises(MgError, match=who + ".*not device memory"):
                    entry(h, 1, *args)
            for args in ((0, p, o), (k, 0, o), (k, p, 0)):
                with pytest.raises(MgError, match=who + ".*null pointer"):
                    entry(h, 1, *args)
            for sets in ((2, 0), (0, 2), (-1, 1), (1, 7)):
                with pytest.raises(MgError, match=who + ".*" + str(sets[0] if sets[0] not in (0, 1) else sets[1]) + " is no node set"):
                    entry(h, 1, k, p, o, *sets)
            with DeviceHierarchy(2, 0, 1, c=16) as h2:
                h2.gen_poisson_level(1)
                with pytest.raises(MgError, match=who + ".*2-D"):
                    entry(h2, 1, k, p, o)
            with DeviceHierarchy(3, 0, 1, c=16) as hs:
                nothing = lambda *a: None
                hs.set_comm_callbacks(0, 2, nothing, nothing, nothing, replicate_below=0)
                with pytest.raises(MgError, match=who + ".*slab"):
                    entry(hs, 1, k, p, o)
            with DeviceHierarchy(3, 0, 0, c=16) as hf:
                hf.set_flat_level(poisson.lexicographic_level(4, 2).A)
                with pytest.raises(MgError, match=who + ".*flat"):
                    entry(hf, 0, k, p, o)
        # out on x, out beginning inside x, x beginning inside out; and out on the direction
        for args in ((k, p, p), (k, o, o + 8 * (n - 1)), (k, o + 8 * (n - 1), o)):
            with pytest.raises(MgError, match="mg_diffusion_apply_dkappa_ex: out overlaps x"):
                T(h, 1, *args)
        with pytest.raises(MgError, match="mg_diffusion_apply_dkappa_ex: out overlaps dkappa"):
            T(h, 1, k, p, k)
        assert h.counters() == counters
        assert h.get_vector(1, "v").tobytes() == before.tobytes()
        T(h, 1, k, o + 8 * n, o)        # next to each other is not overlapping
        # the wrapper refuses a name that is no node set before anything reaches the library
        for call in (lambda: h.diffusion_apply_dkappa(1, k, p, o, rows="boundary"), lambda: h.diffusion_dkappa(1, k, p, o, b_nodes=1)):
            with pytest.raises(ValueError, match="'interior' or 'all'"):
                call()


@pytest.mark.gpu
def test_timing_names_run_the_entries_with_all_nodes():
    """ "apply_dkappa:all" and "dkappa:all" take the operands of "apply_dkappa" and "dkappa" and leave in R what the entries
    return with both node sets "all"."""
    from multigrid_dolfinx_amd.hierarchy import DeviceHierarchy
    N = 36
    case = _kernel_case(N)
    w, x, a = case["w"], case["x"], case["a"]
    cells, n = N ** 3, (N + 1) ** 3
    with DeviceHierarchy(3, 0, 1, c=N // 2) as h:
        h.gen_diffusion_level(1, case["kappa"], matrix_free=True)
        want = h.diffusion_apply_dkappa(1, w, x, rows="all", cols="all")
        assert want.tobytes() != h.diffusion_apply_dkappa(1, w, x).tobytes()
        h.set_vector(1, "v", x)
        h.set_vector(1, "f", np.concatenate([w, np.full(n - cells, np.nan)]))
        h.set_vector(1, "r", np.full(n, np.nan))
        assert h.time_kernel("apply_dkappa:all", 1, reps=2) > 0.0
        assert h.get_vector(1, "r").reshape(-1).tobytes() == want.tobytes()
        want = h.diffusion_dkappa(1, x, a, a_nodes="all", b_nodes="all")
        assert want.tobytes() != h.diffusion_dkappa(1, x, a).tobytes()
        h.set_vector(1, "f", a)
        h.set_vector(1, "r", np.full(n, np.nan))
        assert h.time_kernel("dkappa:all", 1, reps=2) > 0.0
        assert h.get_vector(1, "r").reshape(-1)[:cells].tobytes() == want.tobytes()


# ---- DiffusionSolver: in a process of its own that imports torch FIRST (see tests/test_diffusion_adjoint.py) --------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_first(worker):
    code = "import torch, sys; sys.path.insert(0, %r); import tests.diffusion_dirichlet_workers as w; w.%s()" % (ROOT, worker)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_solution_and_gradients_with_dirichlet_data_against_the_host():
    """N = 16, two levels, rtol 1e-12, stored and matrix-free: u against spsolve of the lifted system, the gradients with respect
    to kappa (a CPU and a device tensor), f and g against the host adjoint; two solves and one generation per backward
    (`gradient_worker`, whose DIRICHLET_LIMIT holds the measured figures)."""
    assert "gradient ok" in _torch_first("gradient_worker")


@pytest.mark.gpu
def test_tangent_with_dirichlet_direction_against_the_host():
    """`tangent` with g and dg against the host tangent solve, and with df = dg = None (`tangent_worker`)."""
    assert "tangent ok" in _torch_first("tangent_worker")


@pytest.mark.gpu
def test_hessian_vector_product_with_dirichlet_data_against_the_host():
    """grad(J, kappa, create_graph=True), then grad(g . v, (kappa, f, g)): the kappa-kappa, f-kappa and g-kappa blocks against the
    host's four-solve product; two solves for the gradient, four in all, one generation (`hessian_worker`)."""
    assert "hessian ok" in _torch_first("hessian_worker")


@pytest.mark.gpu
def test_without_dirichlet_data_nothing_moves():
    """solve, backward and tangent with g = None give the bytes and leave the counters of the calls without the keyword
    (`without_g_worker`)."""
    assert "without g ok" in _torch_first("without_g_worker")
