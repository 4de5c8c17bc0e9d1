"""numpy restatement of the device-resident CG (mfgpu_cg) for the tests: SolverCG::solve of
host/mfgpu_shim_poisson.h -- zero start, absolute tolerance on sqrt(r.r) -- with the sums in float64 and alpha, beta
rounded to the vectors' type before use, and the Chebyshev sweep of PreconditionChebyshev::run_fused from the same
scalars.  Host only."""
import numpy as np


def chebyshev_scalars(degree, lambda_max, smoothing_range):
    """f[0] = 1 / theta, then (f1, f2) per inner step k = 1 .. degree - 1 (PreconditionChebyshev::run_fused)"""
    lambda_min = lambda_max / smoothing_range
    theta, delta = 0.5 * (lambda_max + lambda_min), 0.5 * (lambda_max - lambda_min)
    sigma = theta / delta
    rho = 1.0 / sigma
    f = [1.0 / theta]
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        f += [rho_new * rho, 2.0 * rho_new / delta]
        rho = rho_new
    return np.array(f)


def chebyshev(matvec, dinv, f, dt):
    """z = p(A) r, zero start: the preconditioner MFGPU_CG_CHEBYSHEV applies"""
    f = np.asarray(f).astype(dt)
    degree = (len(f) + 1) // 2

    def apply(r):
        rc = r.copy()
        upd = (f[0] * rc) * dinv
        z = upd.copy()
        for k in range(1, degree):
            rc = rc - matvec(upd)
            upd = f[2 * k - 1] * upd + (f[2 * k] * rc) * dinv
            z = z + upd
        return z

    return apply


def dot(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


def cg(matvec, b, prec, dt, tolerance, max_iterations):
    """generator: (iterations, status, residual, x) after begin and after every iteration until the status leaves 0
    (1 converged, 2 max iterations, 3 breakdown)"""
    b = np.asarray(b, dtype=dt)
    x, r = np.zeros_like(b), b.copy()
    res = np.sqrt(dot(r, r))
    it = 0
    status = 1 if res <= tolerance else 2 if max_iterations == 0 else 0
    yield it, status, res, x
    if status:
        return
    z = prec(r)
    p, rz = z.copy(), dot(r, z)
    while True:
        q = matvec(p)
        pq = dot(p, q)
        if not (pq > 0 and np.isfinite(pq)):
            yield it, 3, res, x
            return
        alpha = dt(rz / pq)
        x = x + alpha * p
        r = r - alpha * q
        it += 1
        res = np.sqrt(dot(r, r))
        status = 1 if res <= tolerance else 2 if it >= max_iterations else 0
        yield it, status, res, x
        if status:
            return
        z = prec(r)
        rz_new = dot(r, z)
        p = z + dt(rz_new / rz) * p
        rz = rz_new


def preconditioner(kind, matvec, dinv, dt, cheb=None):
    """kind: 'none', 'jacobi' or 'chebyshev' (cheb = (degree, lambda_max, smoothing_range))"""
    if kind == "none":
        return lambda r: r.copy()
    if kind == "jacobi":
        return lambda r: dinv * r
    return chebyshev(matvec, dinv, chebyshev_scalars(*cheb), dt)
