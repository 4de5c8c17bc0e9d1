"""The shared form of the plane kernels' index records on the GPU (apply_planes3<.., SH>, reduce_owner_batches;
mfgpu_plan.cpp share_plane_records, share_pass2_records): the same records read through a per-batch table instead of
from per-batch copies.  Same arithmetic
in the same order, so the result equals the expanded form's (flag MFGPU_NO_SHARED_RECORDS) BIT FOR BIT -- anything else
is a bug, not rounding -- and the usual oracle tolerance holds.  Degrees whose kernel has no shared-form instantiation
(p = 5, 6: apply_planes4w) read the expanded form either way and are held to the same two checks."""
import numpy as np
import pytest

import pymfgpu as mf
from oracle import mf_oracle as o
from test_gpu import TOL, gpu_vmult, rel
from util import oracle_desc_from_mesh

pytestmark = pytest.mark.gpu


def make_ops(mesh, **knobs):
    """(operator in the form the plan chooses, operator forced to the expanded form)"""
    for k, v in knobs.items():
        setattr(mesh.desc, k, v)
    flags = mesh.desc.flags
    assert not flags & mf.NO_SHARED_RECORDS
    op = mf.Operator(mesh.desc, mesh)
    mesh.desc.flags = flags | mf.NO_SHARED_RECORDS
    op_x = mf.Operator(mesh.desc, mesh)
    mesh.desc.flags = flags
    assert op_x.plan_stats()["index_records"] == "expanded" and op_x.plan_stats()["pass2_records"] == "expanded"
    return op, op_x


# (p, cells per direction, max_workgroups): meshes the box batches tile and meshes they do not; few workgroups walk
# many batches (the table entries three batches ahead, the previous batch's base in the deferred scatter)
CASES = [(4, 6, 0), (4, 12, 0), (4, 12, 3), (4, 18, 7), (4, 11, 2), (4, 16, 0), (3, 12, 0), (3, 12, 2), (2, 12, 3),
         (5, 10, 0), (5, 10, 3), (6, 9, 0), (6, 9, 2)]


@pytest.mark.parametrize("p,n,wgs", CASES)
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_shared_records_equal_expanded_bit_for_bit(p, n, wgs, nt):
    mesh = mf.Mesh.uniform(3, p, n, number_type=nt)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    kern = mf.KERNEL_PLANES if p <= 3 else mf.KERNEL_AUTO  # (p = 2, 3: the plane kernel on request)
    op, op_x = make_ops(mesh, max_workgroups=wgs, kernel=kern)
    st = op.plan_stats()
    if wgs:
        assert st["n_batches"] >= 3 * wgs, st
    if op.kernel_name() == "apply_planes3" and mf.Plan(mesh.desc, mesh).shares_records:
        assert st["index_records"] == "shared", st
        assert st["index_record_bytes"] < op_x.plan_stats()["index_record_bytes"]
        assert op.memory_consumption() < op_x.memory_consumption()
    if p == 4 and n in (12, 18):  # (n = 6: 18 batches, 18 records -- nothing to share)
        assert st["index_records"] == "shared" and st["distinct_dof_records"] <= 27 and st["distinct_index_records"] <= 27
    if mf.Plan(mesh.desc, mesh).shares_pass2_records:  # (pass 2 of p = 5, 6 shares too: it does not depend on the kernel)
        assert st["pass2_records"] == "shared", st
    if (p, n) in ((4, 12), (4, 18), (3, 12), (5, 10)):  # (meshes the box batches tile, enough batches to share)
        assert st["pass2_records"] == "shared", st
    rng = np.random.default_rng(100 * p + n + wgs)
    x, y0 = rng.standard_normal(mesh.n_dofs), rng.standard_normal(mesh.n_dofs)
    xt, y0t = (v.astype(mf.np_dtype(nt)).astype(np.float64) for v in (x, y0))
    y, y_x = gpu_vmult(op, x, nt), gpu_vmult(op_x, x, nt)
    np.testing.assert_array_equal(y, y_x)
    assert rel(y, o.vmult(od, xt)) <= TOL[nt]
    z, z_x = gpu_vmult(op, x, nt, y0=y0), gpu_vmult(op_x, x, nt, y0=y0)
    np.testing.assert_array_equal(z, z_x)
    assert rel(z, o.vmult_add(od, y0t, xt)) <= TOL[nt]
    # chained applies (bmop.cu:134-146): a workgroup's state does not leak from one launch to the next
    outs = []
    for q in (op, op_x):
        a, b = mf.DeviceVector(mesh.n_dofs, nt), mf.DeviceVector(mesh.n_dofs, nt)
        b.fill(0.1)
        for _ in range(3):
            a, b = b, a
            q.vmult(b, a)
        mf.synchronize()
        outs.append(b.to_host())
    np.testing.assert_array_equal(outs[0], outs[1])


@pytest.mark.parametrize("p,n,world", [(4, 24, 3), (4, 12, 2), (5, 24, 3)])
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_shared_records_on_slabs_with_a_priority_group(p, n, world, nt):
    """z-slabs behind mfgpu_dist (in-process transport): slab-local numbering shares the same way; the interface batches
    run as ranged launches / one launch with a hole, pass 2 has a priority group.  Shared == expanded bit for bit."""
    from pymfgpu.parallel import slab_ranges

    full = mf.Mesh.uniform(3, p, n)
    od = oracle_desc_from_mesh(full, dtype=np.float64)
    key = {tuple(np.round(c, 9)): i for i, c in enumerate(full.dof_coords())}
    fx = full.dof_coords()
    x = (np.sin(3 * fx[:, 0]) + fx[:, 1] ** 2 - np.cos(2 * fx[:, 2]) * fx[:, 0]).astype(mf.np_dtype(nt)).astype(np.float64)
    results = []
    for force_expanded in (False, True):
        slabs = []
        for r, (zb, ze) in enumerate(slab_ranges(n, world)):
            mesh = mf.Mesh.uniform(3, p, n, slab=(zb, ze), number_type=nt)
            gi = np.array([key[tuple(np.round(c, 9))] for c in mesh.dof_coords()])
            if force_expanded:
                mesh.desc.flags |= mf.NO_SHARED_RECORDS
            op = mf.Operator(mesh.desc, mesh)
            if p == 4:
                assert op.plan_stats()["index_records"] == ("expanded" if force_expanded else "shared")
            dist = mf.Dist(mesh, r, world)
            dist.attach(op)
            a, b = mf.DeviceVector(mesh.n_dofs, nt), mf.DeviceVector(mesh.n_dofs, nt)
            a.from_host(x[gi])
            slabs.append(dict(mesh=mesh, op=op, dist=dist, gi=gi, a=a, b=b))
        for lo, up in zip(slabs, slabs[1:]):
            lo["dist"].connect_local(up["dist"])
        for s in slabs:
            s["dist"].vmult_begin(s["op"], s["b"], s["a"])
        for s in slabs:
            s["dist"].vmult_end(s["op"], s["b"])
        mf.synchronize()
        results.append([s["b"].to_host() for s in slabs])
        ref = o.vmult(od, x)
        for s, y in zip(slabs, results[-1]):
            assert rel(y, ref[s["gi"]]) <= TOL[nt]
    for y, y_x in zip(*results):
        np.testing.assert_array_equal(y, y_x)


def test_meshes_that_do_not_share_keep_the_expanded_form():
    """the adaptive mesh (dofs numbered cell by cell in Morton order, hanging-node records) and a mesh of ragged batches:
    today's records, today's kernel"""
    for mesh in (mf.Mesh.adaptive(3, 4, 4), mf.Mesh.uniform(3, 4, [7, 8, 10])):
        od = oracle_desc_from_mesh(mesh)
        op = mf.Operator(mesh.desc, mesh)
        st = op.plan_stats()
        assert st["index_records"] == "expanded" and op.kernel_name() == "apply_planes3", st
        x = np.random.default_rng(11).standard_normal(mesh.n_dofs)
        assert rel(gpu_vmult(op, x), o.vmult(od, x)) <= 1e-12
