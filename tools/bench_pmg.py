#!/usr/bin/env python3
"""p-multigrid against h-multigrid on the same finest level, in one process, alternating.
  1. 3D p = 4 on 8^3, 32^3 and 64^3 cubes and on the ball (n_ref 3): the time of one V-cycle application and of the CG
     solve (device CG, relative 1e-12, the drivers' right-hand side b = A x*) for
       h       the h-hierarchy at p = 4 (VCycle.from_meshes: 1, 2, 4 ... cells per direction / ball n_ref 0 ...)
       hybrid  the hierarchy of host/poisson_pmg.cc (VCycle.from_level_meshes: h-levels at p = 1 from 2 cells per
               direction / ball n_ref 0, then p = 1 -> 2 -> 4 on the finest mesh)
     both with the library's defaults (Chebyshev(5, 15), estimated lambda_max, AUTO coarse solve).
  2. the p-transfer kernels alone, each next to the h-transfer onto the same fine level: prolongate_add at (2 -> 4) and
     (1 -> 2), restrict_and_add at (4 -> 2) and (2 -> 1); with the bytes of the model
       per cell 4 (NC + NF) index bytes + T (NC + NF) vector bytes (+ T NF for the read of prolongate_add's update)
     the achieved bytes/s, and their share of the 8 TB/s HBM peak (6.3 TB/s is what a plain copy reaches).
The protocol is that of tools/bench_vcycle.py: a host clock around `reps` enqueues that end in a device synchronise, one
untimed ramp round, then `rounds` rounds in which the contenders alternate; median with the spread.
usage: tools/bench_pmg.py [--rounds R] [--cases 8,32,64,ball] [--transfers 32,64,ball]   -> one JSON line per row"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: libmfgpu.so binds to the HIP runtime torch brings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-cuda_amd"))
import pymfgpu as mf  # noqa: E402

F64 = mf.F64
BALL_N_REF = 3
HBM_PEAK = 8.0e12


def mesh(case, level, degree):
    """level: cells per direction of a cube, n_ref of the ball"""
    return mf.Mesh.ball(3, degree, level) if case == "ball" else mf.Mesh.uniform(3, degree, level)


def h_levels(case, first):
    if case == "ball":
        return list(range(first, BALL_N_REF + 1))
    n = int(case)
    return [c for c in (1 << k for k in range(n.bit_length())) if c >= first]


def timed(fn, reps):
    mf.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    mf.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def stats(ts, digits=1):
    return round(float(np.median(ts)), digits), [round(min(ts), digits), round(max(ts), digits)]


def alternate(variants, rounds, reps):
    times = {k: [] for k in variants}
    for rnd in range(rounds + 1):  # round 0 is the untimed ramp
        for key, fn in variants.items():
            t = timed(fn, reps)
            if rnd:
                times[key].append(t)
    return times


def bench_case(case, rounds):
    top = h_levels(case, 0)[-1]
    h_meshes = [mesh(case, l, 4) for l in h_levels(case, 0 if case == "ball" else 1)]
    hy_meshes = [mesh(case, l, 1) for l in h_levels(case, 0 if case == "ball" else 2)] + [mesh(case, top, 2), mesh(case, top, 4)]
    V = {"h": mf.VCycle.from_meshes(h_meshes), "hybrid": mf.VCycle.from_level_meshes(hy_meshes)}
    fine = h_meshes[-1]
    N = fine.n_dofs
    op = mf.Operator(fine.desc, fine)
    i = np.arange(N, dtype=np.float64)
    xs = mf.DeviceVector(N)
    xs.from_host(np.sin(0.37 * i) + 0.5 * np.cos(0.011 * i))
    op.set_constrained_values(xs, 0.0)
    b, x, z = mf.DeviceVector(N), mf.DeviceVector(N), mf.DeviceVector(N)
    op.vmult(b, xs)
    tol = 1e-12 * b.l2_norm()
    cg = {}
    for key, v in V.items():
        cg[key] = mf.CG(op, mf.CG_CALLBACK)
        cg[key].set_vcycle(v)
    info, err = {}, {}
    for key in V:
        info[key] = cg[key].solve(x, b, tol, 1000)
        x.add(-1.0, xs)
        err[key] = x.l2_norm() / xs.l2_norm()
    reps = 10 if N < 5_000_000 else 4
    apply_t = alternate({k: (lambda v=v: v.apply(z, b)) for k, v in V.items()}, rounds, reps)
    solve_t = alternate({k: (lambda s=s: s.solve(x, b, tol, 1000)) for k, s in cg.items()}, rounds, 1)
    out = {"config": f"3D p=4 ball n_ref {BALL_N_REF}" if case == "ball" else f"3D p=4 {case}^3 cells", "n_dofs": N,
           "rounds": rounds, "applies_per_round": reps}
    for key, v in V.items():
        out[f"{key}_levels"] = v.n_levels
        out[f"{key}_level_0_dofs"] = (h_meshes if key == "h" else hy_meshes)[0].n_dofs
        out[f"{key}_vcycle_us"], out[f"{key}_vcycle_min_max_us"] = stats(apply_t[key])
        out[f"{key}_cg_iterations"], out[f"{key}_rel_error"] = int(info[key].iterations), float(f"{err[key]:.3e}")
        out[f"{key}_solve_us"], out[f"{key}_solve_min_max_us"] = stats(solve_t[key])
        out[f"{key}_vcycle_bytes"] = v.memory_consumption()
    out["hybrid_over_h_vcycle"] = round(out["hybrid_vcycle_us"] / out["h_vcycle_us"], 3)
    out["hybrid_over_h_solve"] = round(out["hybrid_solve_us"] / out["h_solve_us"], 3)
    print(json.dumps(out), flush=True)


def model_bytes(n_cells, NC, NF, what):
    """index bytes + vector bytes of the per-cell model, double"""
    vec = NC + NF + (NF if what == "prolongate_add" else 0)
    return n_cells * (4 * (NC + NF) + 8 * vec)


def bench_transfers(case, rounds):
    top = h_levels(case, 0)[-1]
    below = BALL_N_REF - 1 if case == "ball" else top // 2
    for what, pc, pf in (("prolongate_add", 2, 4), ("prolongate_add", 1, 2), ("restrict_and_add", 2, 4),
                         ("restrict_and_add", 1, 2)):
        fine = mesh(case, top, pf)
        pm, hm = mesh(case, top, pc), mesh(case, below, pf)
        tp, th = mf.Transfer.p_from_meshes(pm, fine), mf.Transfer.from_meshes(hm, fine)
        rng = np.random.default_rng(0)
        vf = mf.DeviceVector(fine.n_dofs)
        vf.from_host(rng.standard_normal(fine.n_dofs))
        vc = {}
        for key, m in (("p", pm), ("h", hm)):
            vc[key] = mf.DeviceVector(m.n_dofs)
            vc[key].from_host(rng.standard_normal(m.n_dofs))
        if what == "prolongate_add":
            variants = {"p": lambda: tp.prolongate_add(vf, vc["p"]), "h": lambda: th.prolongate_add(vf, vc["h"])}
        else:
            variants = {"p": lambda: tp.restrict_and_add(vc["p"], vf), "h": lambda: th.restrict_and_add(vc["h"], vf)}
        times = alternate(variants, rounds, 20)
        cells = {"p": (pm.n_cells, (pc + 1) ** 3, (pf + 1) ** 3), "h": (hm.n_cells, (pf + 1) ** 3, (2 * pf + 1) ** 3)}
        name = f"ball n_ref {BALL_N_REF}" if case == "ball" else f"{case}^3 cells"
        out = {"config": f"{what} onto 3D p={pf} {name} ({fine.n_dofs} dofs): p-transfer ({pc} -> {pf}) / h-transfer",
               "rounds": rounds, "calls_per_round": 20}
        for key in ("p", "h"):
            us, mm = stats(times[key], 2)
            nbytes = model_bytes(*cells[key], what)
            out[f"{key}_us"], out[f"{key}_min_max_us"] = us, mm
            out[f"{key}_cells"], out[f"{key}_model_bytes"] = cells[key][0], nbytes
            out[f"{key}_model_GB_per_s"] = round(nbytes / us * 1e-3, 1)
            out[f"{key}_share_of_hbm_peak"] = round(nbytes / (us * 1e-6) / HBM_PEAK, 4)
        out["p_over_h"] = round(out["p_us"] / out["h_us"], 3)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="8,32,64,ball")
    ap.add_argument("--transfers", default="32,64,ball")
    args = ap.parse_args()
    for case in [c for c in args.cases.split(",") if c]:
        bench_case(case, args.rounds)
    for case in [c for c in args.transfers.split(",") if c]:
        bench_transfers(case, args.rounds)


if __name__ == "__main__":
    main()
