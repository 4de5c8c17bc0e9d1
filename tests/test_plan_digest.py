"""CPU: the host planner's output, word for word.  For every case below, a SHA-256 of each array pymfgpu.Plan exposes
(mfgpu_plan_array_u32 ids 0..21, lmap, bflags), the mfgpu_plan_shares_records flags and mfgpu_suggest_renumbering, compared
with tests/golden/plan_digests.json.  The fixture is recorded from the library of the commit BEFORE a change to the
planner (never from the code under test):

    MFGPU_RECORD_PLAN_DIGESTS=1 python -m pytest tests/test_plan_digest.py

rewrites it from the library that is loaded (MFGPU_LIB selects one).  A case without a recorded digest fails."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import pymfgpu as mf
from oracle import mf_oracle as o
from test_hanging_host import leaves_refine
from util import desc_from_oracle

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digests.json")
RECORD = os.environ.get("MFGPU_RECORD_PLAN_DIGESTS") == "1"
N_ARRAYS = 22  # ids of mfgpu_plan_array_u32


def _mesh(mesh, kernel=mf.KERNEL_AUTO, flags=0, **knobs):
    mesh.desc.kernel = kernel
    mesh.desc.flags |= flags
    for k, v in knobs.items():
        setattr(mesh.desc, k, v)
    return mesh.desc, mesh


def _uniform(dim, p, n, number_type=mf.F64, **kw):
    return lambda: _mesh(mf.Mesh.uniform(dim, p, n, number_type=number_type), **kw)


def _adaptive(p, n_ref, **kw):
    return lambda: _mesh(mf.Mesh.adaptive(3, p, n_ref), **kw)


def _ragged(colored):
    # the description of test_host.test_plan_orphans_and_ragged_mesh
    od = o.uniform_mesh_desc(2, 2, 4)
    keep_cells = np.array([0, 1, 2, 5, 10, 15])
    od2 = o.Desc(2, 2, od.n_dofs, od.loc2glob[keep_cells], od.JxW[keep_cells], od.inv_jac[keep_cells],
                 od.coefficient[keep_cells], od.constrained)
    return desc_from_oracle(od2, max_cells_per_batch=3, colored=colored)


def _graded(p, levels):
    """a 4x4x4 grid whose corner cell is refined `levels` times, every time the corner child: strongly graded towards
    the corner, 2:1 balanced over faces, edges and vertices"""
    leaves = leaves_refine(3, 2, [(0, 0, 0)])
    for lv in range(3, 2 + levels):
        leaves = [c for c in leaves if c != [lv, 0, 0, 0]] + [[lv + 1, k & 1, (k >> 1) & 1, k >> 2] for k in range(8)]
    return lambda: _mesh(mf.Mesh.from_leaves(3, p, leaves))


CASES = {
    # 2D
    "2d_p2_n32": _uniform(2, 2, 32),
    "2d_p4_n4": _uniform(2, 4, 4),
    "2d_p2_n8_colored": _uniform(2, 2, 8, flags=mf.COLORED_SCATTER),
    # 3D pencil plans, ragged counts
    "3d_p1_n3": _uniform(3, 1, 3),
    "3d_p2_n6": _uniform(3, 2, 6),
    "3d_p6_n2": _uniform(3, 6, 2),
    "3d_p3_n234": _uniform(3, 3, [2, 3, 4]),
    # forced pencils: max_chunks of 4 at p = 3 under apply_batches_x
    "3d_p3_n5_pencils_x": _uniform(3, 3, 5, kernel=mf.KERNEL_PENCILS_X),
    "3d_p3_n5_pencils": _uniform(3, 3, 5, kernel=mf.KERNEL_PENCILS),
    # 3D plane plans; n = 22: extent no multiple of the box (box start, wrap, growth)
    "3d_p4_n3": _uniform(3, 4, 3),
    "3d_p4_n5": _uniform(3, 4, 5),
    "3d_p3_n5": _uniform(3, 3, 5),
    "3d_p4_n4_cells5": _uniform(3, 4, 4, max_cells_per_batch=5),
    "3d_p4_n22": _uniform(3, 4, 22),
    # forced planes, planes4 wide limits
    "3d_p2_n5_planes": _uniform(3, 2, 5, kernel=mf.KERNEL_PLANES),
    "3d_p3_n4_planes_2w": _uniform(3, 3, 4, kernel=mf.KERNEL_PLANES_2W),
    "3d_p5_n4": _uniform(3, 5, 4),
    # (n_ref = 2, the degenerate end of the recipe: ONE cell, no hanging nodes, whatever the cell limit)
    "adaptive_p2_nref2": _adaptive(2, 2),
    "adaptive_p3_nref2": _adaptive(3, 2),
    "adaptive_p4_nref2": _adaptive(4, 2),
    "adaptive_p5_nref2": _adaptive(5, 2),
    "adaptive_p4_nref2_cells3": _adaptive(4, 2, max_cells_per_batch=3),
    # hanging nodes, n_ref = 4 (736 cells, 552 of them with a mask).  p = 3, 4 and p = 2 on request: masked plane batches
    # interleaved with the plain ones, private-entry budget; p = 5: masked cells segregated to the pencil kernel, the
    # stable "plane batches first" sort (cells4: pencil batches of several cells); p = 2 by default, PENCILS_X and
    # PENCILS with a cell limit: masked and unmasked cells SHARE batches, "masked cells first" reorders them
    "adaptive_p2_cells8": _adaptive(2, 4, max_cells_per_batch=8),
    "adaptive_p2_planes": _adaptive(2, 4, kernel=mf.KERNEL_PLANES),
    "adaptive_p3": _adaptive(3, 4),
    "adaptive_p3_pencils_x_cells8": _adaptive(3, 4, kernel=mf.KERNEL_PENCILS_X, max_cells_per_batch=8),
    "adaptive_p4": _adaptive(4, 4),
    "adaptive_p4_cells3": _adaptive(4, 4, max_cells_per_batch=3),
    "adaptive_p4_pencils_cells6": _adaptive(4, 4, kernel=mf.KERNEL_PENCILS, max_cells_per_batch=6),
    "adaptive_p5": _adaptive(5, 4),
    "adaptive_p5_cells4": _adaptive(5, 4, max_cells_per_batch=4),
    # a 4x4x4 grid graded towards one corner (from_leaves): few masked cells among many plain ones.  They pin the class
    # filter of the grower, both limit pairs, the private-entry budget, the n_plain_plane_batches reset and the sort on
    # small batches with leftovers -- and are the attempts to reach the split-and-classify-again loop (none does)
    "graded_p4_l3": _graded(4, 3),
    "graded_p3_l4": _graded(3, 4),
    "graded_p5_l3": _graded(5, 3),
    # general geometry: no MFGPU_UNIFORM_J0, irregular connectivity
    "ball_3d_p2": lambda: _mesh(mf.Mesh.ball(3, 2, 1)),
    "ball_2d_p3": lambda: _mesh(mf.Mesh.ball(2, 3, 2)),
    # orphans
    "ragged_2d": lambda: _ragged(False),
    "ragged_2d_colored": lambda: _ragged(True),
    # float: p = 3 conforming runs in the pencil kernel, in double in apply_planes4
    "3d_p3_n5_f32": _uniform(3, 3, 5, number_type=mf.F32),
}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def plan_digests(desc, keep):
    plan = mf.Plan(desc, keep)
    out = {str(i): _sha(plan._u32(i)) for i in range(N_ARRAYS)}
    out["lmap"] = _sha(plan.lmap)
    out["bflags"] = _sha(plan.bflags)
    out["shares_records"] = int(mf.lib().mfgpu_plan_shares_records(plan._h))
    new_index = np.zeros(int(desc.n_dofs), dtype=np.uint32)
    assert mf.lib().mfgpu_suggest_renumbering(C.byref(desc), new_index.ctypes.data) == 0
    out["renumbering"] = _sha(new_index)
    return out


@pytest.fixture(scope="module")
def recorded():
    if RECORD:
        digests = {name: plan_digests(*make()) for name, make in CASES.items()}
        with open(FIXTURE, "w") as f:
            json.dump(digests, f, indent=0, sort_keys=True)
            f.write("\n")
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_is_bit_identical_to_the_recorded_one(name, recorded):
    assert name in recorded, "no recorded digest for this case"
    got = plan_digests(*CASES[name]())
    assert set(got) == set(recorded[name])
    differ = sorted(k for k in got if got[k] != recorded[name][k])
    assert not differ, differ
