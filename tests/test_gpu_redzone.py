"""Every operator entry point on vectors that sit inside red zones (tests/redzone.py): vmult, vmult_add,
compute_inverse_diagonal, set_constrained_values, update_coefficients and vmult_multi with ALL caller-owned device arrays
as payloads between two zones of 4096 NaN elements, once 16-byte aligned and once one element further, in double and in
float.  The payload is compared with the reference and the tolerance the entry point's own test file uses (TOL of
test_gpu.py for the applies, TOL of test_gpu_aux.py for the inverse diagonal); every zone must keep its bits, every input
too, and the vectors a call overwrites start as NaN.  The control at the top shows that the helper reports a store one
element past either end.  The transfers, the level operator and the index pairs are in test_gpu_redzone_transfer.py, the
integrator, the slab exchange, the vector operations and the solver objects in test_gpu_redzone_solvers.py.

The rows are the smallest shapes of the existing tests at which the named structure exists; the path is asserted where a
row names one.  On the ragged mesh (row k) the dofs of the dropped cells are touched by no cell and are not constrained:
their diagonal is 0, the reference's inverse is not finite there and those entries are not compared."""
import functools

import numpy as np
import pytest

import helmholtz_reference as hr
import pymfgpu as mf
from oracle import mf_oracle as o
from redzone import ZONE, Zoned, bits, pattern
from test_gpu import TOL, rel
from test_gpu_aux import TOL as DIAG_TOL
from test_gpu_helmholtz import _rounded, random_c
from test_gpu_update_coefficients import positive, with_coefficient
from util import deform, deformed_oracle_desc, desc_from_oracle, oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
NTNAME = {F64: "f64", F32: "f32"}
ALIGN = pytest.mark.parametrize("offset_one", [False, True], ids=["aligned", "offset"])
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["f64", "f32"])


def typed(a, nt):
    return np.asarray(a).astype(mf.np_dtype(nt)).astype(np.float64)


# ---- the control: the helper sees a store one element past either end, without a fault


@TYPES
@ALIGN
def test_control_one_element_overruns_are_reported(nt, offset_one):
    n = 1000
    x = np.random.default_rng(0).standard_normal(n)
    z = Zoned(x, nt, offset_one)
    np.testing.assert_array_equal(bits(z.unchanged()), bits(x.astype(mf.np_dtype(nt))))
    z.view(0, n + 1).fill(0.0)  # one element into the back zone, still inside the allocation
    with pytest.raises(AssertionError, match=r"back zone touched: 1 element\(s\), the first at offset \+0 behind"):
        z.result()
    z = Zoned(n, nt, offset_one)
    assert np.array_equal(bits(z.result()), bits(pattern(n, nt)))  # an untouched output payload is the NaN pattern
    z.view(-1, n + 1).fill(0.0)  # one element in front
    with pytest.raises(AssertionError, match=r"front zone touched: 1 element\(s\), the nearest at offset -1 in front"):
        z.result()
    assert z.before.size == 2 * ZONE + n + (1 if offset_one else 0)
    with pytest.raises(AssertionError, match="inside its allocation"):
        z.view(0, n + ZONE + 1)


# ---- the operator rows


def _mesh_row(make_mesh, colored=False, renumber=False, **knobs):
    """build(nt, mass, updatable) -> (operator, oracle description in double, c or None)"""
    def build(nt, mass, updatable):
        mesh = make_mesh(nt)
        if renumber:
            mesh.renumber(mesh.suggest_renumbering())
        od = oracle_desc_from_mesh(mesh, dtype=np.float64)
        c = random_c(od.n_cells, od.nd, nt, seed=5) if mass else None
        if mass:
            mesh.set_mass_coefficient(c)
        for k, v in knobs.items():
            setattr(mesh.desc, k, v)
        if colored:
            mesh.desc.flags |= mf.COLORED_SCATTER
        if updatable:
            mesh.desc.flags |= mf.UPDATABLE_COEFFICIENTS
        od.keep = mesh  # (its arrays are views into the mesh)
        return mf.Operator(mesh.desc, mesh), od, c
    return build


def _oracle_row(make_od, colored=False, **knobs):
    def build(nt, mass, updatable):
        od = make_od()
        c = random_c(od.n_cells, od.nd, nt, seed=5) if mass else None
        desc, keep = desc_from_oracle(od, number_type=nt, colored=colored, mass_coefficient=c, **knobs)
        if updatable:
            desc.flags |= mf.UPDATABLE_COEFFICIENTS
        ref = _rounded(od, nt)  # the description a float operator sees, as doubles
        ref.keep_od = od  # (its index arrays may be views into a mesh that od keeps alive)
        return mf.Operator(desc, keep), ref, c
    return build


def _ragged():
    """the mesh of test_gpu.py::test_ragged_mesh_with_orphans"""
    od = o.uniform_mesh_desc(2, 2, 4)
    cells = np.array([0, 1, 2, 5, 10, 15])
    return o.Desc(2, 2, od.n_dofs, od.loc2glob[cells], od.JxW[cells], od.inv_jac[cells], od.coefficient[cells],
                  od.constrained)


def _deformed_adaptive(dim, p, nref):
    def make():
        mesh = mf.Mesh.adaptive(dim, p, nref)
        od = deform(oracle_desc_from_mesh(mesh, dtype=np.float64), seed=nref)
        od.keep = mesh
        assert od.constraint_mask is not None and od.constraint_mask.any() and not od.uniform_j0
        return od
    return make


def _uniform(dim, p, n):
    return lambda nt: mf.Mesh.uniform(dim, p, n, number_type=nt)


def _adaptive(dim, p, nref):
    return lambda nt: mf.Mesh.adaptive(dim, p, nref, number_type=nt)


def _ball(dim, p, nref):
    return lambda nt: mf.Mesh.ball(dim, p, nref, number_type=nt)


def _name(want):
    return lambda op, st: op.kernel_name() == want


def _multi_chunk(p):
    return lambda op, st: st["n_batches"] >= 2 and st["max_batch_cells"] > 256 // (p + 1) ** 2


def _all(*checks):
    return lambda op, st: all(c(op, st) for c in checks)


def _hanging(op, st):
    return st["n_orphans"] > 0  # the hanging dofs


# (id, build, path check or None, marks: M = again with a mass coefficient, U = again through update_coefficients)
ROWS = [
    ("a-cube_p2_n5", _mesh_row(_uniform(3, 2, 5)),
     _all(_name("apply_batches_x"), lambda op, st: st["max_batch_cells"] == 1), "MU"),
    ("b-cube_p4_n7", _mesh_row(_uniform(3, 4, 7)),
     _all(_name("apply_planes3"), lambda op, st: st["index_records"] == "expanded"), "MU"),
    ("c-cube_p4_n12_shared", _mesh_row(_uniform(3, 4, 12)),
     _all(_name("apply_planes3"), lambda op, st: st["index_records"] == "shared" and st["pass2_records"] == "shared"), ""),
    ("d-cube_p3_n6_2w", _mesh_row(_uniform(3, 3, 6), kernel=mf.KERNEL_PLANES_2W), _name("apply_planes4"), ""),
    ("d-cube_p5_n4", _mesh_row(_uniform(3, 5, 4)), _name("apply_planes4"), ""),
    ("d-cube_p6_n3", _mesh_row(_uniform(3, 6, 3)), _name("apply_planes4"), ""),
    ("e-adaptive_p4_r4", _mesh_row(_adaptive(3, 4, 4)), _all(_name("apply_planes3"), _hanging), "M"),
    ("e-adaptive_p2_r4", _mesh_row(_adaptive(3, 2, 4)), _all(_name("apply_batches_x"), _hanging), ""),
    ("e-adaptive_2d_p4_r4", _mesh_row(_adaptive(2, 4, 4)), _hanging, ""),
    ("f-pencils_p2_n10", _mesh_row(_uniform(3, 2, 10), kernel=mf.KERNEL_PENCILS, max_cells_per_batch=256),
     _all(_name("apply_batches"), _multi_chunk(2)), ""),
    ("f-pencils_x_p4_n6", _mesh_row(_uniform(3, 4, 6), kernel=mf.KERNEL_PENCILS_X, max_cells_per_batch=27),
     _all(_name("apply_batches_x"), _multi_chunk(4)), ""),
    ("g-cube_2d_p3_n5", _mesh_row(_uniform(2, 3, 5)), None, ""),
    ("g-cube_2d_p3_n5_colored", _mesh_row(_uniform(2, 3, 5), colored=True), None, ""),
    ("g-cube_2d_p6_n3", _mesh_row(_uniform(2, 6, 3)), None, ""),
    ("g-cube_p4_n3_colored", _mesh_row(_uniform(3, 4, 3), colored=True), None, ""),
    ("h-deformed_p2_n4", _oracle_row(lambda: deformed_oracle_desc(2, 4, seed=24)), _name("apply_batches_g"), "MU"),
    ("h-deformed_p4_n6_cells27", _oracle_row(lambda: deformed_oracle_desc(4, 6, seed=4), max_cells_per_batch=27),
     _all(_name("apply_batches_g"), _multi_chunk(4)), ""),
    ("h-deformed_adaptive_p2_r4", _oracle_row(_deformed_adaptive(3, 2, 4)), _name("apply_batches_g"), ""),
    ("i-deformed_2d_p4_n6", _oracle_row(lambda: deform(o.uniform_mesh_desc(2, 4, 6), eps=0.15, seed=46)),
     _name("apply_batches_g2"), "M"),
    ("i-deformed_adaptive_2d_p2_r5", _oracle_row(_deformed_adaptive(2, 2, 5), max_cells_per_batch=12),
     _name("apply_batches_g2"), ""),
    ("j-ball_p2_r1", _mesh_row(_ball(3, 2, 1)), _name("apply_batches_g"), ""),
    ("j-ball_2d_p2_r2", _mesh_row(_ball(2, 2, 2)), _name("apply_batches_g2"), ""),
    ("k-ragged_orphans", _oracle_row(_ragged, max_cells_per_batch=3), lambda op, st: st["n_orphans"] > 0, ""),
    ("k-ragged_orphans_colored", _oracle_row(_ragged, colored=True, max_cells_per_batch=3),
     lambda op, st: st["n_orphans"] > 0, ""),
    ("l-segments2_wgs3", _mesh_row(_uniform(3, 4, 6), cell_loop_segments=2, max_workgroups=3),
     _all(_name("apply_planes3"), lambda op, st: st["n_batches"] >= 9), ""),
    ("m-renumbered_p4_n6", _mesh_row(_uniform(3, 4, 6), renumber=True), _name("apply_planes3"), ""),
]
MODES = {"laplace": (False, False), "mass": (True, False), "updated": (True, True)}
OPERATOR_CASES = [pytest.param(i, mode, id=f"{row[0]}-{mode}") for i, row in enumerate(ROWS)
                  for mode in MODES if mode == "laplace" or {"mass": "M", "updated": "U"}[mode] in row[3]]


@functools.lru_cache(maxsize=None)
def _vectors(n, nt):
    """(x, y0) that the number type holds, as doubles; shared and never modified"""
    rng = np.random.default_rng(n)
    x, y0 = typed(rng.standard_normal(n), nt), typed(rng.standard_normal(n), nt)
    x.setflags(write=False)
    y0.setflags(write=False)
    return x, y0


_reference_cache = {}


def _reference(key, od, c, x, y0):
    """(vmult, vmult_add, inverse diagonal) of the row, computed once for both alignments"""
    if key not in _reference_cache:
        if c is None:
            ref = (o.vmult(od, x), o.vmult_add(od, y0, x), o.compute_inverse_diagonal(od))
        else:
            ref = (hr.vmult(od, c, x), hr.vmult_add(od, c, y0, x), hr.inverse_diagonal(od, c))
        _reference_cache[key] = ref
    return _reference_cache[key]


@ALIGN
@TYPES
@pytest.mark.parametrize("i,mode", OPERATOR_CASES)
def test_operator_entry_points(i, mode, nt, offset_one):
    name, build, path, _ = ROWS[i]
    mass, updated = MODES[mode]
    op, od, c = build(nt, mass, updated)
    st = op.plan_stats()
    print(name, mode, NTNAME[nt], op.kernel_name(), st)
    if path is not None:
        assert path(op, st), (op.kernel_name(), st)
    n = od.n_dofs
    assert op.n() == n
    if updated:  # new a and c from zoned device arrays; the reference is the operator created from them
        a1, c1 = positive(od, nt, 21), positive(od, nt, 22)
        za, zc = Zoned(a1, nt, offset_one), Zoned(c1, nt, offset_one)
        op.update_coefficients(za.vec, zc.vec)
        za.unchanged()
        zc.unchanged()
        od, c = with_coefficient(od, a1), c1
    x, y0 = _vectors(n, nt)
    want_y, want_add, want_diag = _reference((i, mode, nt), od, c, x, y0)

    src, dst = Zoned(x, nt, offset_one), Zoned(n, nt, offset_one)
    op.vmult(dst.vec, src.vec)
    y = dst.result()
    src.unchanged()
    e = rel(y, want_y)  # (a NaN left in the payload makes this NaN, and the comparison false)
    assert e <= TOL[nt], ("vmult", e, int(np.isnan(y).sum()))

    acc = Zoned(y0, nt, offset_one)
    op.vmult_add(acc.vec, src.vec)
    e = rel(acc.result(), want_add)
    src.unchanged()
    assert e <= TOL[nt], ("vmult_add", e)

    d = Zoned(n, nt, offset_one)
    op.compute_inverse_diagonal(d.vec)
    got = d.result()
    fin = np.isfinite(want_diag)
    assert fin.all() or name.startswith("k-")  # (the ragged mesh: dofs no cell touches, see the docstring)
    assert np.isfinite(got[fin]).all()
    np.testing.assert_allclose(got[fin], want_diag[fin], rtol=DIAG_TOL[nt])

    v = Zoned(x, nt, offset_one)
    op.set_constrained_values(v.vec, -3.5)
    want = x.astype(mf.np_dtype(nt))
    want[od.constrained] = -3.5
    np.testing.assert_array_equal(v.result(), want)


# ---- vmult_multi: the whole block of vectors with their inter-vector padding between two zones


@ALIGN
@TYPES
@pytest.mark.parametrize("add", [False, True], ids=["vmult", "add"])
def test_vmult_multi_block_in_zones(add, nt, offset_one):
    """3 vectors at stride n + 5 on the ball (test_gpu_multi.py keeps its sentinel in the padding; here the padding and
    both ends of the block are NaN patterns that must keep their bits)"""
    mesh = mf.Mesh.ball(3, 2, 1, number_type=nt)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    op = mf.Operator(mesh.desc, mesh)
    assert op.kernel_name() == "apply_batches_g"
    n, k = mesh.n_dofs, 3
    stride = n + 5
    rng = np.random.default_rng(k)
    X, Y0 = typed(rng.standard_normal((k, n)), nt), typed(rng.standard_normal((k, n)), nt)
    hs = pattern(k * stride, nt).reshape(k, stride)
    hs[:, :n] = X
    hd = pattern(k * stride, nt).reshape(k, stride)
    if add:
        hd[:, :n] = Y0
    for mode in (mf.MULTI_FUSED, mf.MULTI_LOOP):
        src, dst = Zoned(hs, nt, offset_one), Zoned(hd, nt, offset_one)
        op.vmult_multi(dst.vec, src.vec, k, stride, add=add, mode=mode)
        out = dst.result().reshape(k, stride)
        src.unchanged()
        np.testing.assert_array_equal(bits(out[:, n:]), bits(hd[:, n:]))  # the padding keeps its bits
        for j in range(k):
            want = o.vmult_add(od, Y0[j], X[j]) if add else o.vmult(od, X[j])
            assert rel(out[j, :n], want) <= TOL[nt], (mode, j)
