#!/usr/bin/env python3
"""Global-coarsening multigrid against local smoothing and the p-V-cycle, in one process, alternating.
  1. the problem of host/poisson_gc.cc (3D p = 4, Chebyshev(5, 15), estimated lambda_max, AUTO coarse solve, device CG to
     1e-12 |b|, the drivers' right-hand side) on Mesh.adaptive_mg(3, 4, n_ref), the mesh both hierarchies accept:
       h        VCycle.from_hierarchy (local smoothing on the level hierarchy)
       gc       VCycle.from_global_coarsening at p = 4 throughout
       gc_124   VCycle.from_global_coarsening with degrees (1, 2, 4)
     and on Mesh.adaptive(3, 4, n_ref) the two gc rows next to section 19's p-V-cycle (that mesh at degrees 1, 2, 4, coarse
     CG capped at 30): microseconds per V-cycle, CG iterations, solve time.
  2. the three transfer calls at p = 4 on the finest pair (coarsened mesh -> Mesh.adaptive(3, 4, n_ref)) next to section
     19's p-transfer (2 -> 4) on the same cells: microseconds, per fine cell, and the achieved bytes/s of the model
       h_hn  4 N n_fine fine indices + 8 n_fine (parent, word) + 4 N n_coarse coarse indices (read once: siblings share
             them in L2) + 8 N (n_coarse + n_fine) vector bytes (+ 8 N n_fine for the read of prolongate_add's update)
       p_hn  tools/bench_pmg.py's model plus 4 bytes of mask per cell
The protocol is that of tools/bench_pmg.py: a host clock around `reps` enqueues that end in a device synchronise, one
untimed ramp round, then `rounds` rounds in which the contenders alternate; median with min and max.
usage: tools/bench_gc.py [--rounds R] [--n-ref 6] [--skip-solve] [--skip-transfers] [--kinds adaptive_mg,adaptive]
       [--only h,gc_124]  -> one JSON line per row"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: libmfgpu.so binds to the HIP runtime torch brings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-cuda_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pymfgpu as mf  # noqa: E402
from bench_pmg import HBM_PEAK, alternate, model_bytes, stats  # noqa: E402


def bench_solve(kind, n_ref, rounds, only=None):
    t0 = time.perf_counter()
    fine = (mf.Mesh.adaptive_mg if kind == "adaptive_mg" else mf.Mesh.adaptive)(3, 4, n_ref)
    make = {"gc": lambda: mf.VCycle.from_global_coarsening(fine),
            "gc_124": lambda: mf.VCycle.from_global_coarsening(fine, (1, 2, 4))}
    if kind == "adaptive_mg":
        make = {"h": lambda: mf.VCycle.from_hierarchy(fine), **make}
    else:
        make = {"pmg_124_cap_30": lambda: mf.VCycle.from_level_meshes(
            [mf.Mesh.from_leaves(3, p, fine.cell_levels()) for p in (1, 2)] + [fine], coarse_max_iterations=30), **make}
    V = {key: fn() for key, fn in make.items() if only is None or key in only}  # (--only: fewer hierarchies in the process)
    print(f"# {kind}: {len(V)} hierarchies built in {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
    out = {"config": f"3D p=4 Mesh.{kind}(3, 4, {n_ref}): V-cycle and CG solve to 1e-12 |b| per hierarchy", "rounds": rounds,
           "n_dofs": fine.n_dofs, "n_cells": fine.n_cells, "gc_cells_per_level": [M.n_cells for M in mf.Mesh.coarsening_sequence(fine, 1)],
           "host_setup_s": round(time.perf_counter() - t0, 1)}
    N = fine.n_dofs
    op = mf.Operator(fine.desc, fine)
    i = np.arange(N, dtype=np.float64)
    xs = mf.DeviceVector(N)
    xs.from_host(np.sin(0.37 * i) + 0.5 * np.cos(0.011 * i))
    op.set_constrained_values(xs, 0.0)
    b, x, z = mf.DeviceVector(N), mf.DeviceVector(N), mf.DeviceVector(N)
    op.vmult(b, xs)
    tol = 1e-12 * b.l2_norm()
    cgs = {}
    for key, v in V.items():
        cgs[key] = mf.CG(op, mf.CG_CALLBACK)
        cgs[key].set_vcycle(v)
        info = cgs[key].solve(x, b, tol, 1000)
        x.add(-1.0, xs)
        out[f"{key}_levels"], out[f"{key}_cg_status"] = v.n_levels, int(info.status)
        out[f"{key}_cg_iterations"], out[f"{key}_rel_error"] = int(info.iterations), float(f"{x.l2_norm() / xs.l2_norm():.3e}")
    apply_t = alternate({k: (lambda v=v: v.apply(z, b)) for k, v in V.items()}, rounds, 4)
    solve_t = alternate({k: (lambda c=c: c.solve(x, b, tol, 1000)) for k, c in cgs.items()}, rounds, 1)
    for key in V:
        out[f"{key}_vcycle_us"], out[f"{key}_vcycle_min_max_us"] = stats(apply_t[key])
        out[f"{key}_solve_us"], out[f"{key}_solve_min_max_us"] = stats(solve_t[key])
    print(json.dumps(out), flush=True)


def bench_transfers(n_ref, rounds):
    p, N = 4, 125
    fine = mf.Mesh.adaptive(3, p, n_ref)
    coarse = mf.Mesh.from_leaves(3, p, mf.Mesh.coarsen_leaves(3, fine.cell_levels()))
    low = mf.Mesh.from_leaves(3, 2, fine.cell_levels())
    pairs = {"h_hn": (coarse, fine), "p_hn": (low, fine)}
    t = {"h_hn": mf.Transfer.h_hn_from_meshes(coarse, fine), "p_hn": mf.Transfer.p_hn_from_meshes(low, fine)}
    rng = np.random.default_rng(0)
    vf = mf.DeviceVector(fine.n_dofs)
    vf.from_host(rng.standard_normal(fine.n_dofs))
    vc = {}
    for key, (c, _) in pairs.items():
        vc[key] = mf.DeviceVector(c.n_dofs)
        vc[key].from_host(rng.standard_normal(c.n_dofs))
    _, child = mf.coarsening_map(coarse, fine)
    for what in ("prolongate", "prolongate_add", "restrict_and_add"):
        if what == "restrict_and_add":
            variants = {k: (lambda k=k: t[k].restrict_and_add(vc[k], vf)) for k in t}
        else:
            variants = {k: (lambda k=k: getattr(t[k], what)(vf, vc[k])) for k in t}
        times = alternate(variants, rounds, 20)
        out = {"config": f"{what} 3D p = 4 on Mesh.adaptive(3, 4, {n_ref}): h_hn from its coarsening / p_hn (2 -> 4) on the same cells",
               "rounds": rounds, "calls_per_round": 20, "fine_cells": fine.n_cells, "coarse_cells": coarse.n_cells,
               "unchanged_cells": int((child == 0).sum()), "fine_dofs": fine.n_dofs}
        extra = 8 * N * fine.n_cells if what == "prolongate_add" else 0
        nbytes = {"h_hn": fine.n_cells * (4 * N + 8) + coarse.n_cells * 4 * N + 8 * N * (coarse.n_cells + fine.n_cells) + extra,
                  "p_hn": model_bytes(fine.n_cells, 27, N, what) + 4 * fine.n_cells}
        for key in t:
            us, mm = stats(times[key], 2)
            out[f"{key}_us"], out[f"{key}_min_max_us"] = us, mm
            out[f"{key}_ns_per_fine_cell"] = round(1e3 * us / fine.n_cells, 3)
            out[f"{key}_model_bytes"], out[f"{key}_model_GB_per_s"] = nbytes[key], round(nbytes[key] / us * 1e-3, 1)
            out[f"{key}_share_of_hbm_peak"] = round(nbytes[key] / (us * 1e-6) / HBM_PEAK, 4)
        out["h_hn_over_p_hn"] = round(out["h_hn_us"] / out["p_hn_us"], 3)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n-ref", type=int, default=6)
    ap.add_argument("--skip-solve", action="store_true")
    ap.add_argument("--skip-transfers", action="store_true")
    ap.add_argument("--kinds", default="adaptive_mg,adaptive", help="the meshes of the solve rows")
    ap.add_argument("--only", default=None, help="comma list of h, pmg_124_cap_30, gc, gc_124: build only these hierarchies")
    args = ap.parse_args()
    if not args.skip_transfers:
        bench_transfers(args.n_ref, args.rounds)
    if not args.skip_solve:
        for kind in args.kinds.split(","):
            bench_solve(kind, args.n_ref, args.rounds, None if args.only is None else args.only.split(","))


if __name__ == "__main__":
    main()
