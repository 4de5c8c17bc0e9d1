#!/usr/bin/env python3
"""The p-transfer on a mesh with hanging nodes, in one process, alternating.
  1. the three calls of the transfer on the adaptively refined cube (Mesh.adaptive(3, ., n_ref), default n_ref 6) at
     (2 -> 4) and (1 -> 2), each next to the conforming kernel at the same degrees on the 64^3 cube: microseconds, cells/s
     and the achieved bytes/s of the model of tools/bench_pmg.py plus 4 bytes of mask per cell
       per cell 4 (NC + NF) index bytes + T (NC + NF) vector bytes (+ T NF for the read of prolongate_add's update) (+ 4)
     (every cell is charged its full NF fine values, although a cell moves only the ones it owns).
  2. the problem of host/poisson_pmg.cc -DADAPTIVE_GRID (3D p = 4, that mesh at degrees 1 -> 2 -> 4, Chebyshev(5, 15),
     estimated lambda_max, AUTO coarse solve: above MFGPU_VCYCLE_DENSE_MAX dofs on level 0 the unpreconditioned device CG)
     for a few caps on the coarse iterations: the time of one V-cycle application and of the CG solve (device CG, relative
     1e-12, the drivers' right-hand side), next to the local-smoothing h-multigrid V-cycle of poisson-mg-3d-p4-adaptive
     (VCycle.from_hierarchy on Mesh.adaptive_mg, which balances over vertices too: not quite the same cells).
The protocol is that of tools/bench_pmg.py: a host clock around `reps` enqueues that end in a device synchronise, one
untimed ramp round, then `rounds` rounds in which the contenders alternate; median with the spread.
usage: tools/bench_pmg_hn.py [--rounds R] [--n-ref 6] [--cube 64] [--caps 10,30,100] [--skip-solve]  -> one JSON line per row"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the library: libmfgpu.so binds to the HIP runtime torch brings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-cuda_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pymfgpu as mf  # noqa: E402
from bench_pmg import HBM_PEAK, alternate, model_bytes, stats  # noqa: E402


def bench_transfers(n_ref, cube, rounds):
    for pc, pf in ((2, 4), (1, 2)):
        pairs = {"hn": (mf.Mesh.adaptive(3, pc, n_ref), mf.Mesh.adaptive(3, pf, n_ref)),
                 "conforming": (mf.Mesh.uniform(3, pc, cube), mf.Mesh.uniform(3, pf, cube))}
        t = {"hn": mf.Transfer.p_hn_from_meshes(*pairs["hn"]), "conforming": mf.Transfer.p_from_meshes(*pairs["conforming"])}
        rng = np.random.default_rng(0)
        vc, vf = {}, {}
        for key, (c, f) in pairs.items():
            vc[key], vf[key] = mf.DeviceVector(c.n_dofs), mf.DeviceVector(f.n_dofs)
            vc[key].from_host(rng.standard_normal(c.n_dofs))
            vf[key].from_host(rng.standard_normal(f.n_dofs))
        masked = int((pairs["hn"][0].arrays()["constraint_mask"] != 0).sum())
        for what in ("prolongate", "prolongate_add", "restrict_and_add"):
            if what == "restrict_and_add":
                variants = {k: (lambda k=k: t[k].restrict_and_add(vc[k], vf[k])) for k in t}
            else:
                variants = {k: (lambda k=k: getattr(t[k], what)(vf[k], vc[k])) for k in t}
            times = alternate(variants, rounds, 20)
            out = {"config": f"{what} ({pc} -> {pf}) 3D: adaptive n_ref {n_ref} with hanging nodes / conforming {cube}^3 cube",
                   "rounds": rounds, "calls_per_round": 20, "hn_masked_cells": masked}
            for key, (c, f) in pairs.items():
                us, mm = stats(times[key], 2)
                nbytes = model_bytes(c.n_cells, (pc + 1) ** 3, (pf + 1) ** 3, what) + (4 * c.n_cells if key == "hn" else 0)
                out[f"{key}_us"], out[f"{key}_min_max_us"] = us, mm
                out[f"{key}_cells"], out[f"{key}_fine_dofs"] = c.n_cells, f.n_dofs
                out[f"{key}_Mcells_per_s"] = round(c.n_cells / us, 1)
                out[f"{key}_model_bytes"], out[f"{key}_model_GB_per_s"] = nbytes, round(nbytes / us * 1e-3, 1)
                out[f"{key}_share_of_hbm_peak"] = round(nbytes / (us * 1e-6) / HBM_PEAK, 4)
            out["hn_over_conforming_per_cell"] = round((out["hn_us"] / out["hn_cells"]) / (out["conforming_us"] / out["conforming_cells"]), 3)
            print(json.dumps(out), flush=True)


def bench_solve(n_ref, caps, rounds):
    meshes = [mf.Mesh.adaptive(3, p, n_ref) for p in (1, 2, 4)]
    hmesh = mf.Mesh.adaptive_mg(3, 4, n_ref)
    V = {f"p_cap_{cap}": (mf.VCycle.from_level_meshes(meshes, coarse_max_iterations=cap), meshes[-1]) for cap in caps}
    V["h"] = (mf.VCycle.from_hierarchy(hmesh), hmesh)
    out = {"config": f"3D p=4 adaptive n_ref {n_ref}: p-V-cycle over degrees 1, 2, 4 per coarse cap / local-smoothing h-V-cycle",
           "rounds": rounds, "p_n_dofs": meshes[-1].n_dofs, "p_level_dofs": [M.n_dofs for M in meshes], "h_n_dofs": hmesh.n_dofs}
    state = {}
    for key, (v, fine) in V.items():
        N = fine.n_dofs
        if ("op", N, id(fine)) not in state:
            op = mf.Operator(fine.desc, fine)
            i = np.arange(N, dtype=np.float64)
            xs = mf.DeviceVector(N)
            xs.from_host(np.sin(0.37 * i) + 0.5 * np.cos(0.011 * i))
            op.set_constrained_values(xs, 0.0)
            b, x, z = mf.DeviceVector(N), mf.DeviceVector(N), mf.DeviceVector(N)
            op.vmult(b, xs)
            state[("op", N, id(fine))] = (op, xs, b, x, z, 1e-12 * b.l2_norm())
        op, xs, b, x, z, tol = state[("op", N, id(fine))]
        cg = mf.CG(op, mf.CG_CALLBACK)
        cg.set_vcycle(v)
        info = cg.solve(x, b, tol, 1000)
        x.add(-1.0, xs)
        out[f"{key}_levels"], out[f"{key}_cg_status"] = v.n_levels, int(info.status)
        out[f"{key}_cg_iterations"], out[f"{key}_rel_error"] = int(info.iterations), float(f"{x.l2_norm() / xs.l2_norm():.3e}")
        V[key] = (v, cg, b, x, z, tol)
    apply_t = alternate({k: (lambda a=a: a[0].apply(a[4], a[2])) for k, a in V.items()}, rounds, 4)
    solve_t = alternate({k: (lambda a=a: a[1].solve(a[3], a[2], a[5], 1000)) for k, a in V.items()}, rounds, 1)
    for key in V:
        out[f"{key}_vcycle_us"], out[f"{key}_vcycle_min_max_us"] = stats(apply_t[key])
        out[f"{key}_solve_us"], out[f"{key}_solve_min_max_us"] = stats(solve_t[key])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-ref", type=int, default=6)
    ap.add_argument("--cube", type=int, default=64)
    ap.add_argument("--caps", default="10,30,100")
    ap.add_argument("--skip-solve", action="store_true")
    args = ap.parse_args()
    bench_transfers(args.n_ref, args.cube, args.rounds)
    if not args.skip_solve:
        bench_solve(args.n_ref, [int(c) for c in args.caps.split(",") if c], args.rounds)


if __name__ == "__main__":
    main()
