"""Stream ordering and graph capture (tests/stream_harness.py, as tests/test_gpu_streams_qop.py) of
mfgpu_vqop_set_coefficients -> mfgpu_vqop_vmult, of the inverse diagonal, and of mfgpu_bicgstab_begin + _iterate on a
VectorQpOperator: each call runs behind a delay on a non-blocking stream, and is captured once (after the harness's warm
call) and replayed on other data -- the replays fold and apply different coefficient arrays.  3D p = 2 on the three mesh
kinds of test_gpu_poisson.small_mesh."""
import functools

import numpy as np
import pytest

import bicgstab_reference as br
import pymfgpu as mf
import stream_harness as sh
import vqop_reference as vr
from stream_harness import Case, sets
from test_gpu import rel
from test_gpu_poisson import close
from test_gpu_streams import integrator

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = {}
KINDS = ("cube", "hanging", "ball")
K = 3


def case(name):
    def register(build):
        CASES[name] = functools.lru_cache(maxsize=None)(lambda: build(name))
        return build
    return register


def positive(mesh, seed):
    return sets(lambda rng: rng.uniform(0.5, 2.0, mesh.n_cells * mesh.nd), seed)


def _cases(kind):
    tag = f"{kind}_3d_p2"

    @case(f"vqop_set_coefficients-vmult-isotropic-mass-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        q = mf.VectorQpOperator(it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
        co = {"lam": positive(mesh, 400), "mu": positive(mesh, 401), "mass": positive(mesh, 402)}
        x = sets(lambda rng: rng.standard_normal(3 * mesh.n_dofs), 403)

        def call(b, s):
            q.set_coefficients(lam=b["lam"], mu=b["mu"], mass=b["mass"], stream=s)
            q.vmult(b["dst"], b["x"], stream=s)

        def check(k, got, ret):
            close(got["dst"], vr.apply(cells, x[k], **{t: a[k] for t, a in co.items()}), 1e-12)
        return Case(name, dict(co, x=x), {"dst": (np.float64, 3 * mesh.n_dofs)}, call, check)

    @case(f"vqop_set_coefficients-vmult-tensor4-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        q = mf.VectorQpOperator(it, mf.VQOP_TENSOR4)
        npts = mesh.n_cells * mesh.nd
        c4 = sets(lambda rng: rng.standard_normal((npts, 3, 3, 3, 3)) + 3.0 * vr.isotropic_tensor(0.0, 0.5, 3), 410)
        x = sets(lambda rng: rng.standard_normal(3 * mesh.n_dofs), 411)

        def call(b, s):
            q.set_coefficients(tensor=b["tensor"], stream=s)
            q.vmult(b["dst"], b["x"], stream=s)

        def check(k, got, ret):
            close(got["dst"], vr.apply(cells, x[k], tensor=c4[k]), 1e-12)
        return Case(name, {"tensor": c4, "x": x}, {"dst": (np.float64, 3 * mesh.n_dofs)}, call, check)

    @case(f"vqop_set_coefficients-inverse_diagonal-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        q = mf.VectorQpOperator(it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
        co = {"lam": positive(mesh, 420), "mu": positive(mesh, 421), "mass": positive(mesh, 422)}

        def call(b, s):
            q.set_coefficients(lam=b["lam"], mu=b["mu"], mass=b["mass"], stream=s)
            q.inverse_diagonal(b["dinv"], s)

        def check(k, got, ret):
            close(got["dinv"], vr.inverse_diagonal(cells, **{t: a[k] for t, a in co.items()}), 1e-12)
        return Case(name, co, {"dinv": (np.float64, 3 * mesh.n_dofs)}, call, check)

    @case(f"bicgstab_begin_iterate{K}-vqop-jacobi-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        q = mf.VectorQpOperator(it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
        co = {t: positive(mesh, 430 + i)[0] for i, t in enumerate(("lam", "mu", "mass"))}
        keep = {t: torch.from_numpy(a).to("cuda:0") for t, a in co.items()}
        q.set_coefficients(**keep)
        n = 3 * mesh.n_dofs
        dinv = torch.empty(n, dtype=torch.float64, device="cuda:0")
        q.inverse_diagonal(dinv)
        torch.cuda.synchronize()
        dinv_h = dinv.cpu().numpy()
        solver = mf.BiCGStab(q, mf.CG_JACOBI, dinv)
        con = vr.constrained_flags(cells)
        b = sets(lambda rng: np.where(con, 0.0, rng.standard_normal(n)), 434)

        def call(bufs, s):
            solver.begin(bufs["x"], bufs["b"], 0.0, 1000, s)
            solver.iterate(K, s)

        def check(k, got, ret):
            rows = br.bicgstab(lambda v: vr.apply(cells, v, **co), b[k], lambda r: dinv_h * r, np.float64, 0.0, 1000)
            want = list(zip(range(K + 1), rows))[-1][1]
            assert want[:2] == (K, 0)
            err = rel(got["x"], want[3])
            print(f"{name} value set {k}: rel l2 {err:.3e}")
            assert err <= 1e-12
            assert solver.status().as_tuple()[:2] == (K, 0)
        c = Case(name, {"b": b}, {"x": (np.float64, n)}, call, check)
        c.keep = (keep, dinv)
        return c


for _kind in KINDS:
    _cases(_kind)

NAMES = sorted(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_ordered_on_a_nonblocking_stream(name):
    sh.check_ordered(CASES[name]())


@pytest.mark.parametrize("name", NAMES)
def test_captured_once_replayed_on_new_data(name):
    sh.check_graph(CASES[name]())
