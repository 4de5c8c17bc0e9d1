"""Shared form of the plane kernels' index records (mfgpu_plan.cpp share_plane_records; no GPU needed).

A plane plan's dof lists (mfgpu_plan_array_u32 13) and index runs (14) are fixed-size records per batch.  Where the
dof numbering repeats from batch to batch they are a handful of distinct records repeated; the shared form stores
every distinct record once (17: dof lists minus the batch's smallest dof id, bit 31 kept; 18: index runs) and per
batch {that dof id, record numbers} (19).  It is lossless: expanding it gives 13 and 14 word for word, whichever form
the plan chooses.

Pass 2 likewise (share_pass2_records): the pass-2 dofs grouped by the batch of their FIRST partial sum, one record per
owner batch (20), distinct ones once, per batch {smallest dof id, record offset} (21).  Expanding them gives the plan's
(sdofs, s_off, s_idx) as the same set of dofs, each with its slots in the same order."""
import numpy as np
import pytest

import pymfgpu as mf

KGU = {3: 5, 4: 11, 5: 18, 6: 28, 7: 41}  # p_kgu of mfgpu_internal.h
HS = {3: 3, 4: 6, 5: 9, 6: 14, 7: 18}      # p_hs
P2_HEADER, P2_SLOT_BITS = 16, 12            # kP2Header, kP2SlotBits


def record_sizes(p):
    n = p + 1
    return KGU[n] * 64, ((n * n + 1) // 2) * ((64 // n) * n)


def expand(plan, p):
    nb, nx = record_sizes(p)
    tab = plan.sh_batch
    dofs = plan.sh_dofs.reshape(-1, nb)
    idx = plan.sh_idx.reshape(-1, nx)
    assert np.all(tab[:, 3] == 0)
    if len(tab):
        assert tab[:, 1].max() < len(dofs) and tab[:, 2].max() < len(idx)
        # every record is used, and none is stored twice
        assert len(np.unique(tab[:, 1])) == len(dofs) == len(np.unique(dofs, axis=0))
        assert len(np.unique(tab[:, 2])) == len(idx) == len(np.unique(idx, axis=0))
    rel = dofs[tab[:, 1]]
    # relative entries: non-negative in their low 31 bits, and the smallest of a batch is 0 (base = its smallest dof id)
    low = rel & np.uint32(0x7fffffff)
    if len(tab):
        assert np.all(low.min(axis=1) == 0)
    full = (low.astype(np.uint64) + tab[:, 0:1]).astype(np.uint32) | (rel & np.uint32(0x80000000))
    return full.reshape(-1), idx[tab[:, 2]].reshape(-1), len(dofs), len(idx)


def expand_pass2(plan, p):
    """{dof entry (bit 31 kept): [halo slots]} from the owner-batch records, and the number of distinct records"""
    hs = HS[p + 1] * 64
    rec, tab = plan.sh_p2rec, plan.sh_p2tab
    out = {}
    for b, (base, off) in enumerate(tab):
        r = rec[off:]
        ne, e0, kmax = int(r[0]), int(r[1]), int(r[2])
        assert e0 % 64 == 0 and e0 - 64 < ne <= e0 and kmax <= 12
        d = r[P2_HEADER:P2_HEADER + e0]
        k = r[P2_HEADER + e0:P2_HEADER + 2 * e0]
        assert np.all(d[ne:] == 0xffffffff) and np.all(k[ne:] == 0)
        assert np.all(np.diff(k[:ne].astype(np.int64)) <= 0) and (ne == 0 or k[0] == kmax) and np.all(k[:ne] >= 1)
        for e in range(ne):
            w = [int(r[int(r[3 + t]) + e]) for t in range(int(k[e]))]
            assert (w[0] >> P2_SLOT_BITS) == 0  # the owner is the first toucher
            slots = [(b + (x >> P2_SLOT_BITS)) * hs + (x & ((1 << P2_SLOT_BITS) - 1)) for x in w]
            entry = ((int(d[e]) & 0x7fffffff) + int(base)) | (int(d[e]) & 0x80000000)
            assert entry not in out
            out[entry] = slots
    return out, len(np.unique(tab[:, 1])) if len(tab) else 0


def pass2_reference(plan):
    sd, so, si = plan.sdofs, plan.s_off, plan.s_idx
    return {int(sd[i]): [int(x) for x in si[so[i]:so[i + 1]]] for i in range(len(sd)) if so[i + 1] > so[i]}


MESHES = {
    "p3_n48": (3, lambda: mf.Mesh.uniform(3, 3, 48)),
    "p4_n18": (4, lambda: mf.Mesh.uniform(3, 4, 18)),
    "p4_n54": (4, lambda: mf.Mesh.uniform(3, 4, 54)),
    "p5_n40": (5, lambda: mf.Mesh.uniform(3, 5, 40)),
    "p6_n36": (6, lambda: mf.Mesh.uniform(3, 6, 36)),
    "p4_n30_slab_6_18": (4, lambda: mf.Mesh.uniform(3, 4, 30, slab=(6, 18))),
    "p4_7x8x10_slab_2_9": (4, lambda: mf.Mesh.uniform(3, 4, [7, 8, 10], slab=(2, 9))),
    "p4_7x8x10": (4, lambda: mf.Mesh.uniform(3, 4, [7, 8, 10])),
    "p3_n7": (3, lambda: mf.Mesh.uniform(3, 3, 7)),
    "p5_n7": (5, lambda: mf.Mesh.uniform(3, 5, 7)),
    "p6_n5": (6, lambda: mf.Mesh.uniform(3, 6, 5)),
    "p4_adaptive4": (4, lambda: mf.Mesh.adaptive(3, 4, 4)),
    "p3_adaptive4": (3, lambda: mf.Mesh.adaptive(3, 3, 4)),
    "p4_ball2": (4, lambda: mf.Mesh.ball(3, 4, 2)),
}
# distinct (index-run, dof-list) records on cubes the box batches tile: a box is first, inner or last per direction
TILED = {"p3_n48": (26, 27), "p4_n18": (26, 27), "p4_n54": (26, 27), "p5_n40": (26, 27), "p6_n36": (26, 27),
         "p4_n30_slab_6_18": (27, 27)}
EXPANDED = ["p4_7x8x10_slab_2_9", "p4_7x8x10", "p4_adaptive4", "p3_adaptive4"]


@pytest.mark.parametrize("name", list(MESHES))
def test_shared_form_expands_to_the_plane_records(name):
    p, make = MESHES[name]
    mesh = make()
    plan = mf.Plan(mesh.desc, mesh)
    dofs, idx, n_dof_rec, n_idx_rec = expand(plan, p)
    np.testing.assert_array_equal(dofs, plan.pr_dofs)
    np.testing.assert_array_equal(idx, plan.pr_idx)
    nb, _ = record_sizes(p)
    n_batches = len(plan.pr_dofs) // nb
    print(f"{name}: {n_batches} plane batches, {n_idx_rec} index-run / {n_dof_rec} dof-list records, "
          f"{'shared' if plan.shares_records else 'expanded'}")
    assert len(plan.sh_batch) == n_batches
    if name in TILED:
        assert (n_idx_rec, n_dof_rec) == TILED[name]
        assert n_idx_rec <= 27 and n_dof_rec <= 27
        assert plan.shares_records
    if name in EXPANDED:
        assert not plan.shares_records and not plan.shares_pass2_records
    if n_batches and len(plan.sh_p2tab):
        got, n_p2_rec = expand_pass2(plan, p)
        print(f"{name}: {n_p2_rec} pass-2 records, {'shared' if plan.shares_pass2_records else 'expanded'}")
        assert got == pass2_reference(plan)
        if name in TILED:
            assert n_p2_rec == 27 and plan.shares_pass2_records
    else:  # (batches outside the plane kernels: pass 2 keeps its class arrays)
        assert not plan.shares_pass2_records
    if n_batches == 0:  # (the ball: general geometry, no plane batches)
        assert not plan.shares_records and n_dof_rec == 0 and n_idx_rec == 0


def test_n64_shares_and_the_choice_is_by_bytes():
    """64 is no multiple of the box edges: ragged batches, ~3000 distinct records among 22 238 -- still clearly
    smaller than the expanded arrays, so the plan shares.  The choice compares bytes and nothing else."""
    mesh = mf.Mesh.uniform(3, 4, 64)
    plan = mf.Plan(mesh.desc, mesh)
    dofs, idx, nd, ni = expand(plan, 4)
    np.testing.assert_array_equal(dofs, plan.pr_dofs)
    np.testing.assert_array_equal(idx, plan.pr_idx)
    shared = len(plan.sh_dofs) + len(plan.sh_idx) + plan.sh_batch.size
    assert shared * 2 <= len(plan.pr_dofs) + len(plan.pr_idx) and plan.shares_records
    assert nd < 4000 and ni < 4000


def test_renumbered_mesh_keeps_the_expanded_form_losslessly():
    """a numbering that does not repeat (the optional batch-major renumbering numbers the shared dofs in pass-2 order):
    whatever the plan chooses, the shared form still expands to the records word for word"""
    mesh = mf.Mesh.uniform(3, 4, 12)
    mesh.renumber(mesh.suggest_renumbering())
    plan = mf.Plan(mesh.desc, mesh)
    dofs, idx, _, _ = expand(plan, 4)
    np.testing.assert_array_equal(dofs, plan.pr_dofs)
    np.testing.assert_array_equal(idx, plan.pr_idx)
