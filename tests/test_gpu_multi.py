"""mfgpu_vmult_multi on the GPU: the operator applied to several vectors in one call, in fused groups of 3 and 2 vectors
on the 3D general-geometry path (apply_batches_g + reduce_classes at width 2 or 3) and one by one everywhere else.

Every vector of every call is compared with oracle.mf_oracle.vmult / vmult_add on the same arrays AND with mfgpu_vmult of
the same handle.  Tolerances are those of this path (tests/test_gpu_ball.py): relative l2 <= 1e-12 in double, 2e-5 in
float, per vector.  No bit equality with the single apply on the non-mass path (its cross-wave lds_add order is not
fixed); with a mass term two fused calls on the same inputs give equal bits, as the single kernel does.

Layout of a call: vector k starts at element k * stride.  dst is pre-filled with 7.0 (the call must overwrite), the
stride - n_dofs padding entries of every dst vector hold a sentinel that must survive, src must come back unchanged."""
import copy
import functools

import numpy as np
import pytest

import helmholtz_reference as hr
import pymfgpu as mf
from oracle import mf_oracle as o
from test_gpu import gpu_vmult, rel
from util import deform, deformed_oracle_desc, desc_from_oracle, oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

TOL = {mf.F64: 1e-12, mf.F32: 2e-5}
SENTINEL = -3.5
NV_MAX = 7
GROUPINGS = (2, 3, 5, 7)  # 2, 3, 3 + 2, 3 + 3 + 1


def vectors(n, nt, seed, count=NV_MAX):
    """`count` distinct random vectors, rounded to the number type, as doubles"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((count, n)).astype(mf.np_dtype(nt)).astype(np.float64)


def run_multi(op, X, nt, stride=None, mode=mf.MULTI_FUSED, Y0=None):
    """dst vectors [k][n_dofs] of one vmult_multi call on the rows of X (Y0: vmult_add onto its rows)"""
    k, n = X.shape
    stride = n if stride is None else stride
    hs = np.full((k, stride), SENTINEL)
    hs[:, :n] = X
    hd = np.full((k, stride), SENTINEL)
    hd[:, :n] = 7.0 if Y0 is None else Y0
    src, dst = mf.DeviceVector(k * stride, nt), mf.DeviceVector(k * stride, nt)
    src.from_host(hs)
    dst.from_host(hd)
    op.vmult_multi(dst, src, k, stride, add=Y0 is not None, mode=mode)
    mf.synchronize()
    out = dst.to_host().reshape(k, stride)
    np.testing.assert_array_equal(src.to_host().reshape(k, stride), hs.astype(mf.np_dtype(nt)))  # src untouched
    np.testing.assert_array_equal(out[:, n:], np.full((k, stride - n), SENTINEL, dtype=out.dtype))  # padding untouched
    return out[:, :n].astype(np.float64)


def check_rows(got, refs, tol, what):
    for k in range(got.shape[0]):
        for name, ref in refs.items():
            e = rel(got[k], ref[k])
            print(f"{what} vector {k} vs {name}: {e:.3e}")
            assert e <= tol, (what, k, name, e)


def check_fused(op, X, nt, ref, single, constrained=None, strides=(0, 37), groupings=GROUPINGS):
    """every grouping and stride, MFGPU_MULTI_FUSED, against the oracle rows `ref` and the single applies `single`"""
    n = X.shape[1]
    for k in groupings:
        for pad in strides:
            got = run_multi(op, X[:k], nt, n + pad)
            check_rows(got, {"oracle": ref, "mfgpu_vmult": single}, TOL[nt], f"n_vectors={k} stride=n+{pad}")
            if constrained is not None:  # Dirichlet rows are identity rows in every vector
                np.testing.assert_array_equal(got[:, constrained], X[:k][:, constrained])


def singles(op, X, nt, Y0=None):
    return np.stack([gpu_vmult(op, X[k], nt, y0=None if Y0 is None else Y0[k]).astype(np.float64)
                     for k in range(X.shape[0])])


BALL = [(1, 2, 0, mf.F64), (2, 1, 0, mf.F64), (2, 2, 16, mf.F64), (3, 1, 8, mf.F64), (4, 1, 0, mf.F64),
        (4, 2, 27, mf.F64), (6, 0, 0, mf.F64), (4, 1, 8, mf.F32)]


@functools.lru_cache(maxsize=None)
def ball_case(p, n_ref, nt):
    """mesh, oracle description, the vectors and their oracle images (computed once, shared, read-only)"""
    mesh = mf.Mesh.ball(3, p, n_ref, number_type=nt)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    X = vectors(mesh.n_dofs, nt, 100 * p + n_ref)
    Y0 = vectors(mesh.n_dofs, nt, 100 * p + n_ref + 50)
    ref = np.stack([o.vmult(od, x) for x in X])
    ref_add = np.stack([o.vmult_add(od, y, x) for x, y in zip(X, Y0)])
    for a in (X, Y0, ref, ref_add):
        a.setflags(write=False)
    return mesh, od, X, Y0, ref, ref_add


def ball_operator(p, n_ref, cells, nt, max_workgroups=0):
    mesh, od, X, Y0, ref, ref_add = ball_case(p, n_ref, nt)
    mesh.desc.max_cells_per_batch = cells
    mesh.desc.max_workgroups = max_workgroups
    op = mf.Operator(mesh.desc, mesh)
    mesh.desc.max_cells_per_batch = mesh.desc.max_workgroups = 0
    assert op.kernel_name() == "apply_batches_g"
    return op, mesh, od, X, Y0, ref, ref_add


@pytest.mark.parametrize("p,n_ref,cells,nt", BALL)
def test_ball_fused_groups_match_oracle_and_single_applies(p, n_ref, cells, nt):
    op, mesh, od, X, Y0, ref, ref_add = ball_operator(p, n_ref, cells, nt)
    assert op.multi_width() == 3
    check_fused(op, X, nt, ref, singles(op, X, nt), constrained=mesh.arrays()["constrained_dofs"])


@pytest.mark.parametrize("p,n_ref,cells,nt", [BALL[2], BALL[4], BALL[5], BALL[7]])
def test_ball_fused_add(p, n_ref, cells, nt):
    """MFGPU_MULTI_ADD: dst_k += A src_k, and dst_c += src_c on constrained rows, against o.vmult_add"""
    op, mesh, od, X, Y0, ref, ref_add = ball_operator(p, n_ref, cells, nt)
    single = singles(op, X, nt, Y0)
    n = X.shape[1]
    c = mesh.arrays()["constrained_dofs"]
    for k in GROUPINGS:
        got = run_multi(op, X[:k], nt, n + 37, Y0=Y0[:k])
        check_rows(got, {"oracle": ref_add, "mfgpu_vmult_add": single}, TOL[nt], f"add n_vectors={k}")
        np.testing.assert_array_equal(got[:, c].astype(mf.np_dtype(nt)), (Y0[:k][:, c] + X[:k][:, c]).astype(mf.np_dtype(nt)))


@pytest.mark.parametrize("max_workgroups", [1, 2])
def test_one_workgroup_walks_many_batches(max_workgroups):
    """persistent workgroups: with 1 or 2 of them each walks many batches with the next batch's loads in flight"""
    op, mesh, od, X, Y0, ref, ref_add = ball_operator(4, 2, 27, mf.F64, max_workgroups=max_workgroups)
    assert op.plan_stats()["n_batches"] > 4 * max_workgroups
    single = singles(op, X[:3], mf.F64)
    check_fused(op, X, mf.F64, ref, single, strides=(37,), groupings=(2, 3))
    got = run_multi(op, X[:3], mf.F64, Y0=Y0[:3])
    check_rows(got, {"oracle": ref_add}, 1e-12, "add")


@pytest.mark.parametrize("p,n", [(2, 4), (4, 2), (5, 2)])
def test_deformed_cubes(p, n):
    od = deformed_oracle_desc(p, n, seed=p * 10 + n)
    desc, keep = desc_from_oracle(od)
    op = mf.Operator(desc, keep)
    assert op.kernel_name() == "apply_batches_g" and op.multi_width() == 3
    X = vectors(od.n_dofs, mf.F64, p)
    ref = np.stack([o.vmult(od, x) for x in X])
    check_fused(op, X, mf.F64, ref, singles(op, X, mf.F64), constrained=od.constrained)


@pytest.mark.parametrize("p,n_ref", [(2, 4), (4, 4)])
def test_adaptive_mesh_full_jacobian_hanging_nodes(p, n_ref):
    mesh = mf.Mesh.adaptive(3, p, n_ref)
    od = deform(oracle_desc_from_mesh(mesh, dtype=np.float64), seed=n_ref)
    assert od.constraint_mask is not None and od.constraint_mask.any() and not od.uniform_j0
    desc, keep = desc_from_oracle(od)
    op = mf.Operator(desc, keep)
    assert op.kernel_name() == "apply_batches_g" and op.multi_width() == 3
    X = vectors(od.n_dofs, mf.F64, 11)
    Y0 = vectors(od.n_dofs, mf.F64, 12, 3)
    ref = np.stack([o.vmult(od, x) for x in X])
    check_fused(op, X, mf.F64, ref, singles(op, X, mf.F64), strides=(37,))
    got = run_multi(op, X[:3], mf.F64, Y0=Y0)
    check_rows(got, {"oracle": np.stack([o.vmult_add(od, y, x) for x, y in zip(X[:3], Y0)])}, 1e-12, "add")


@pytest.mark.parametrize("p,n_ref", [(2, 1), (4, 1)])
def test_mass_term_and_equal_bits(p, n_ref):
    mesh = mf.Mesh.ball(3, p, n_ref)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    c = np.random.default_rng(p).uniform(0.5, 1.5, (od.n_cells, od.nd))
    mesh.set_mass_coefficient(c)
    op = mf.Operator(mesh.desc, mesh)
    assert op.kernel_name() == "apply_batches_g" and op.multi_width() == 3
    X = vectors(od.n_dofs, mf.F64, 5)
    Y0 = vectors(od.n_dofs, mf.F64, 6, 3)
    ref = np.stack([hr.vmult(od, c, x) for x in X])
    check_fused(op, X, mf.F64, ref, singles(op, X, mf.F64), constrained=mesh.arrays()["constrained_dofs"], strides=(37,))
    got = run_multi(op, X[:3], mf.F64, Y0=Y0)
    check_rows(got, {"reference": np.stack([hr.vmult_add(od, c, y, x) for x, y in zip(X[:3], Y0)])}, 1e-12, "add")
    for k in (2, 3, 5):  # fixed summation order of the MASS instantiations
        np.testing.assert_array_equal(run_multi(op, X[:k], mf.F64), run_multi(op, X[:k], mf.F64))


def test_updated_coefficients():
    """after mfgpu_update_coefficients the fused apply is that of a handle created from the new values"""
    mesh = mf.Mesh.ball(3, 2, 1)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    rng = np.random.default_rng(3)
    c0, c1 = (rng.uniform(0.5, 1.5, (od.n_cells, od.nd)) for _ in range(2))

    def make(coef, updatable):
        d = copy.copy(od)
        d.coefficient = coef
        desc, keep = desc_from_oracle(d)
        if updatable:
            desc.flags |= mf.UPDATABLE_COEFFICIENTS
        return mf.Operator(desc, keep), d

    h1, _ = make(c0, True)
    X = vectors(od.n_dofs, mf.F64, 8, 3)
    before = run_multi(h1, X, mf.F64)
    dc = mf.DeviceVector(c1.size)
    dc.from_host(c1.reshape(-1))
    h1.update_coefficients(dc, None)
    mf.synchronize()
    h2, od1 = make(c1, False)
    ref = np.stack([o.vmult(od1, x) for x in X])
    got1, got2 = run_multi(h1, X, mf.F64), run_multi(h2, X, mf.F64)
    check_rows(got1, {"oracle": ref, "fresh handle": got2}, 1e-12, "updated")
    assert rel(before[0], ref[0]) > 1e-3  # (the update changed the operator)


def fallback_handles():
    yield "cube_3d_p4_n3", mf.Mesh.uniform(3, 4, 3), False
    yield "cube_2d_p2_n8_twopass", mf.Mesh.uniform(2, 2, 8), False
    yield "cube_2d_p2_n8_colored", mf.Mesh.uniform(2, 2, 8), True
    yield "ball_2d_p2", mf.Mesh.ball(2, 2, 2), False


@pytest.mark.parametrize("which", range(4))
def test_handles_without_fused_instantiation_fall_back(which):
    name, mesh, colored = list(fallback_handles())[which]
    if colored:
        mesh.desc.flags |= mf.COLORED_SCATTER
    op = mf.Operator(mesh.desc, mesh)
    if which == 0:
        assert op.kernel_name().startswith("apply_planes")
    assert op.multi_width() == 1
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    X = vectors(mesh.n_dofs, mf.F64, which, 3)
    Y0 = vectors(mesh.n_dofs, mf.F64, which + 9, 3)
    single, single_add = singles(op, X, mf.F64), singles(op, X, mf.F64, Y0)
    ref = np.stack([o.vmult(od, x) for x in X])
    for mode in (None, mf.MULTI_LOOP):
        got = run_multi(op, X, mf.F64, mesh.n_dofs + 37, mode=mode)
        check_rows(got, {"oracle": ref, "mfgpu_vmult": single}, 1e-12, f"{name} mode={mode}")
        got = run_multi(op, X, mf.F64, mode=mode, Y0=Y0)
        check_rows(got, {"mfgpu_vmult_add": single_add}, 1e-12, f"{name} add mode={mode}")
    dst, src = mf.DeviceVector(3 * mesh.n_dofs), mf.DeviceVector(3 * mesh.n_dofs)
    dst.fill(7.0)
    src.from_host(X.reshape(-1))
    with pytest.raises(mf.MfgpuError) as e:
        op.vmult_multi(dst, src, 3, mode=mf.MULTI_FUSED)
    assert e.value.code == mf.EUNSUPPORTED
    mf.synchronize()
    np.testing.assert_array_equal(dst.to_host(), 7.0)


def test_default_and_loop_modes_on_a_fused_handle():
    """whatever the dispatch table says for the degree, the default mode and MFGPU_MULTI_LOOP compute the same operator"""
    op, mesh, od, X, Y0, ref, ref_add = ball_operator(2, 2, 16, mf.F64)
    single = singles(op, X[:5], mf.F64)
    for mode in (None, mf.MULTI_LOOP):
        got = run_multi(op, X[:5], mf.F64, X.shape[1] + 37, mode=mode)
        check_rows(got, {"oracle": ref, "mfgpu_vmult": single}, 1e-12, f"mode={mode}")
    got = run_multi(op, X[:1], mf.F64, mode=None)  # one vector: a single apply, any stride
    check_rows(got, {"oracle": ref}, 1e-12, "one vector")


def test_invalid_arguments_write_nothing():
    op, mesh, od, X, Y0, ref, ref_add = ball_operator(2, 1, 0, mf.F64)
    n = mesh.n_dofs
    buf = mf.DeviceVector(8 * n)
    host = np.full(8 * n, 7.0)
    host[:3 * n] = X[:3].reshape(-1)
    buf.from_host(host)
    src, dst = buf.ptr, buf.ptr + 4 * n * 8

    def refused(*args, **kw):
        with pytest.raises(mf.MfgpuError) as e:
            op.vmult_multi(*args, **kw)
        assert e.value.code == mf.EINVAL, e.value
        mf.synchronize()
        np.testing.assert_array_equal(buf.to_host(), host)

    refused(dst, src, 0)                                             # n_vectors == 0
    refused(dst, src, 2, stride=n - 1)                               # stride < n_dofs with more than one vector
    refused(dst, src, 2, mode=mf.MULTI_LOOP | mf.MULTI_FUSED)        # both modes
    refused(src + 8 * (2 * n + 5), src, 3)                           # dst starts inside the src range
    refused(src, src + 8 * (2 * n + 5), 3)                           # src starts inside the dst range
    refused(src + 8 * (n + 5), src, 2, stride=2 * n)                 # interleaved ranges overlap as ranges
    refused(src, src, 1)
    op.vmult_multi(dst, src, 1, stride=0)                            # one vector: the stride is not used
    mf.synchronize()
    assert rel(buf.to_host()[4 * n:5 * n], ref[0]) <= 1e-12


def test_halo_buffers_are_counted_and_freed():
    mesh, od, X, Y0, ref, ref_add = ball_case(2, 2, mf.F64)

    def cycle():
        op = mf.Operator(mesh.desc, mesh)
        width = op.multi_width()
        assert width == 3
        halo_bytes = (op.plan_stats()["rmw_adds_or_halo_slots"] + 1) * 8  # partial sums + the always-zero slot
        m0 = op.memory_consumption()
        run_multi(op, X[:2], mf.F64, mode=mf.MULTI_LOOP)
        assert op.memory_consumption() == m0            # looping allocates nothing
        run_multi(op, X[:2], mf.F64)
        m1 = op.memory_consumption()
        assert m1 - m0 == (width - 1) * halo_bytes, (m0, m1, halo_bytes)
        run_multi(op, X[:7], mf.F64)
        assert op.memory_consumption() == m1            # later calls allocate nothing
        op.clear()
        mf.synchronize()

    cycle()  # (the first use of a kernel loads its code object: not the handle's memory)
    free0, _ = mf.device_memory_info()
    cycle()
    free1, _ = mf.device_memory_info()
    assert free1 == free0, (free0, free1)
