"""NumPy flexible conjugate gradients preconditioned by one V-cycle of the CPU oracle: the recurrence of `mg_pcg`
(multigrid_dolfinx_amd/csrc/mg_capi.hip, fcg_solve) step for step, for the tests to compare against.

    x = x0; r = b - A x; z = M r; p = z; rz = r.z
    loop: q = A p; alpha = rz / p.q; x += alpha p; r -= alpha q; stop if ||r|| <= rtol ||b||
          z = M r; beta = -alpha (z.q) / rz; rz = r.z; p = z + beta p

M r is one V(mu1, mu2) cycle of `Oracle.v_cycle` from a zero guess (flexible Polak-Ribiere form: the injection cycle and
the Gauss-Seidel smoothers are not symmetric)."""
import numpy as np


def fcg(orc, b, rtol=1e-11, max_iter=200, x0=None, level=None, restriction="direct", smoother="jacobi"):
    """Returns (x, history of ||r_k||_2 after every iteration)."""
    level = orc.finest_level if level is None else level
    A = orc.A_sp_dict[level][0]
    b = np.asarray(b, dtype=np.float64).reshape(-1, 1)

    def prec(r):
        return orc.v_cycle(orc.A_jacobi_sp_dict[level], np.zeros_like(r), r, restriction=restriction, smoother=smoother)

    x = np.zeros_like(b) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(-1, 1).copy()
    r = b - A.dot(x)
    tol = rtol * float(np.linalg.norm(b)) if rtol > 0 else -1.0
    hist = []
    rn = float(np.linalg.norm(r))
    if max_iter <= 0 or rn <= tol or rn == 0.0:
        return x, np.array(hist)
    z = prec(r)
    p = z.copy()
    rz = float(r.ravel() @ z.ravel())
    while True:
        q = A.dot(p)
        alpha = rz / float(p.ravel() @ q.ravel())
        x = x + alpha * p
        r = r - alpha * q
        rn = float(np.linalg.norm(r))
        hist.append(rn)
        if rn <= tol or rn == 0.0 or len(hist) >= max_iter:
            break
        z = prec(r)
        beta = -alpha * float(z.ravel() @ q.ravel()) / rz
        rz = float(r.ravel() @ z.ravel())
        p = z + beta * p
    return x, np.array(hist)
