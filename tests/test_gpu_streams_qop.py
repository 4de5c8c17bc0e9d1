"""Stream ordering and graph capture (tests/stream_harness.py, as tests/test_gpu_streams.py) of
mfgpu_integrator_integrate, mfgpu_qop_set_coefficients, mfgpu_qop_vmult and mfgpu_qop_compute_inverse_diagonal: each call
runs behind a delay on a non-blocking stream, and is captured once and replayed on other data -- the replays fold and
apply different coefficient arrays.  3D p = 2 on the three mesh kinds of test_gpu_poisson.small_mesh."""
import functools

import numpy as np
import pytest

import pymfgpu as mf
import qop_reference as qr
import stream_harness as sh
from stream_harness import Case, sets
from test_gpu_poisson import close
from test_gpu_streams import integrator

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = {}
TERMS = mf.QOP_DIFFUSION_TENSOR | mf.QOP_CONVECTION | mf.QOP_FLUX | mf.QOP_REACTION
KINDS = ("cube", "hanging", "ball")


def case(name):
    def register(build):
        CASES[name] = functools.lru_cache(maxsize=None)(lambda: build(name))
        return build
    return register


def coefficient_sets(mesh, seed):
    npts = mesh.n_cells * mesh.nd
    return {"diffusion": sets(lambda rng: rng.standard_normal((npts, 3, 3)) + 3.0 * np.eye(3), seed),
            "convection": sets(lambda rng: rng.standard_normal((npts, 3)), seed + 1),
            "flux": sets(lambda rng: rng.standard_normal((npts, 3)), seed + 2),
            "reaction": sets(lambda rng: rng.uniform(0.5, 2.0, npts), seed + 3)}


def _cases(kind):
    tag = f"{kind}_3d_p2"

    @case(f"integrator_integrate-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        npts = mesh.n_cells * mesh.nd
        v = sets(lambda rng: rng.standard_normal(npts), 300)
        g = sets(lambda rng: rng.standard_normal(3 * npts), 301)

        def check(k, got, ret):
            close(got["dst"], qr.integrate(cells, v[k], g[k]), 1e-12)
        return Case(name, {"v": v, "g": g}, {"dst": (np.float64, mesh.n_dofs)},
                    lambda b, s: it.integrate(b["dst"], b["v"], b["g"], s), check)

    @case(f"qop_set_coefficients-vmult-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        q = mf.QpOperator(it, TERMS)
        co = coefficient_sets(mesh, 310)
        x = sets(lambda rng: rng.standard_normal(mesh.n_dofs), 315)

        def call(b, s):
            q.set_coefficients(b["diffusion"], b["convection"], b["flux"], b["reaction"], s)
            q.vmult(b["dst"], b["x"], stream=s)

        def check(k, got, ret):
            close(got["dst"], qr.apply(cells, x[k], **{t: a[k] for t, a in co.items()}), 1e-12)
        return Case(name, dict(co, x=x), {"dst": (np.float64, mesh.n_dofs)}, call, check)

    @case(f"qop_vmult-transpose-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        q = mf.QpOperator(it, TERMS)
        co = {t: a[0] for t, a in coefficient_sets(mesh, 320).items()}
        keep = {t: torch.from_numpy(a.reshape(-1)).to("cuda:0") for t, a in co.items()}
        q.set_coefficients(**keep)
        x = sets(lambda rng: rng.standard_normal(mesh.n_dofs), 325)

        def check(k, got, ret):
            close(got["dst"], qr.apply(cells, x[k], transpose=True, **co), 1e-12)
        return Case(name, {"x": x}, {"dst": (np.float64, mesh.n_dofs)},
                    lambda b, s: q.vmult(b["dst"], b["x"], transpose=True, stream=s), check)

    @case(f"qop_set_coefficients-inverse_diagonal-{tag}")
    def _(name):
        it, cells, mesh = integrator(kind)
        q = mf.QpOperator(it, TERMS)
        co = coefficient_sets(mesh, 330)

        def call(b, s):
            q.set_coefficients(b["diffusion"], b["convection"], b["flux"], b["reaction"], s)
            q.inverse_diagonal(b["dinv"], s)

        def check(k, got, ret):
            close(got["dinv"], qr.inverse_diagonal(cells, **{t: a[k] for t, a in co.items()}), 1e-12)
        return Case(name, co, {"dinv": (np.float64, mesh.n_dofs)}, call, check)


for _kind in KINDS:
    _cases(_kind)

NAMES = sorted(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_ordered_on_a_nonblocking_stream(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sh.check_ordered(CASES[name]())


@pytest.mark.parametrize("name", NAMES)
def test_captured_once_replayed_on_new_data(name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sh.check_graph(CASES[name]())
