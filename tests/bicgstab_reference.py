"""numpy restatement of the device-resident BiCGStab (mfgpu_bicgstab) for the tests: the
recurrence of SolverBicgstab::solve (host/mfgpu_shim_qop.h) and of qop_reference.bicgstab -- right-preconditioned, zero
start, r0 = b, a half-step exit on |s| <= tolerance after x += alpha y, a full-step exit on |r| <= tolerance -- as a
generator over the iterations, on vectors of a given dtype with the sums in float64 and alpha, omega, beta rounded to
that dtype before any element-wise use.  The dot product is injectable, so that the sensitivity of the iterates to the
summation order can be measured (test_bicgstab_host.py).  Host only."""
import numpy as np


def dot(a, b):
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


def strided_dot(ways):
    """a dot product that sums `ways` interleaved subsequences first: another summation order than np.dot's"""
    def f(a, b):
        prod = a.astype(np.float64) * b.astype(np.float64)
        return float(sum(float(prod[k::ways].sum()) for k in range(ways)))

    return f


def usable(v):
    return v != 0.0 and np.isfinite(v)


def bicgstab(matvec, b, prec, dt, tolerance, max_iterations, dot=dot):
    """generator: (iterations, status, residual, x) after begin and after every iteration until the status leaves 0
    (1 converged, 2 max iterations, 3 breakdown: r0.v, t.t or rho zero or not finite).  A half-step exit in iteration k
    yields (k, 1, |s|, x + alpha y); a breakdown yields the last count and residual with x at the last complete
    update.  prec: callable z = M^-1 r."""
    b = np.asarray(b, dtype=dt)
    x, r = np.zeros_like(b), b.copy()
    r0 = r.copy()
    v, p = np.zeros_like(b), np.zeros_like(b)
    rho = alpha = omega = 1.0
    res = np.sqrt(dot(r, r))
    it = 0
    rho_new = dot(r0, r)
    while True:
        status = 1 if res <= tolerance else 2 if it >= max_iterations else 0 if usable(rho_new) else 3
        yield it, status, res, x
        if status:
            return
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = r + dt(beta) * (p - dt(omega) * v)
        y = prec(p)
        v = matvec(y)
        r0v = dot(r0, v)
        if not usable(r0v):
            yield it, 3, res, x
            return
        alpha = rho / r0v
        s = r - dt(alpha) * v
        x = x + dt(alpha) * y
        ss = np.sqrt(dot(s, s))
        if ss <= tolerance:
            yield it + 1, 1, ss, x
            return
        z = prec(s)
        t = matvec(z)
        ts, tt = dot(t, s), dot(t, t)
        if not usable(tt):
            yield it, 3, res, x
            return
        omega = ts / tt
        x = x + dt(omega) * z
        r = s - dt(omega) * t
        it += 1
        res = np.sqrt(dot(r, r))
        rho_new = dot(r0, r)


def history(matvec, b, prec, dt, tolerance, max_iterations, dot=dot):
    """the same with the half steps visible: a list of (iteration, 'half' | 'full', norm) up to the exit"""
    out = []

    def spy(a, c):
        d = dot(a, c)
        if a is c:
            out.append(np.sqrt(d))
        return d

    steps = list(bicgstab(matvec, b, prec, dt, tolerance, max_iterations, spy))
    # squares arrive as r_0.r_0, then per iteration s.s and, unless the half step ended the solve, t.t and r.r
    kinds = ("half", None, "full")
    names = [(0, "full")] + [(k // 3 + 1, kinds[k % 3]) for k in range(len(out) - 1)]
    return [(it, kind, n) for (it, kind), n in zip(names, out) if kind], steps


def preconditioner(kind, dinv):
    """kind: 'none' or 'jacobi'"""
    if kind == "none":
        return lambda r: r.copy()
    return lambda r: dinv * r
