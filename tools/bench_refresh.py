#!/usr/bin/env python3
"""Time of bringing a V-cycle up to date after a coefficient update: mfgpu_vcycle_refresh on the existing object against
the only route there was before it, destroy + mfgpu_vcycle_create on the same updated levels; in the same process,
alternating.
  refresh   VCycle.refresh(eig_steps=0) and a synchronisation: per level above 0 the inverse diagonal and as many
            power-iteration steps as the estimate took at creation, the Chebyshev scalars, the dense coarse inverse
  recreate  VCycle.destroy() + VCycle(...) with estimated lambda_max (blocks by itself) and a synchronisation
and the split of both into their three parts, each timed alone on the same levels:
  diagonals  compute_inverse_diagonal on the levels above 0 (the same calls on both sides; recreate adds level 0's)
  estimates  estimate_lambda_max_enqueue with the refresh's step counts / estimate_lambda_max (host loop, level 0 too)
  coarse     refresh / create of a one-level dense VCycle on the level-0 operator with lambda_max given: the coarse inverse
The hierarchies of tools/bench_vcycle.py: uniform 3D p = 4 at 8^3, 32^3 and 64^3 cells and the adaptive p = 4 mesh of
poisson-mg-3d-p4-adaptive 6; double and float levels; MFGPU_UPDATABLE_COEFFICIENTS on every level, the coefficient
replaced once by 1 + x^2 + 2 y^2 + 3 z^2 before anything is timed.  Wall time of the host, since the re-create is host
work; median of the rounds with min and max, after one untimed round.
usage: tools/bench_refresh.py [--rounds R] [--cases 8,32,64,adaptive]   -> one JSON line per row"""
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

F64, F32 = mf.F64, mf.F32
UPD = mf.UPDATABLE_COEFFICIENTS


def wall_us(fn):
    mf.synchronize()
    t0 = time.perf_counter()
    fn()
    mf.synchronize()
    return 1e6 * (time.perf_counter() - t0)


def stats(ts):
    return round(float(np.median(ts)), 1), [round(min(ts), 1), round(max(ts), 1)]


def build(case, nt):
    if case == "adaptive":
        mesh = mf.Mesh.adaptive_mg(3, 4, 6, number_type=nt)
        levels, keep = mf.VCycle.hierarchy_levels(mesh, flags=UPD)
        return levels, keep, keep[2], mesh.n_dofs, "adaptive 3D p=4 n_ref 6"
    n = int(case)
    meshes = [mf.Mesh.uniform(3, 4, c, number_type=nt) for c in (1 << k for k in range(n.bit_length()))]
    levels = [{"op": mf.Operator(mf.VCycle._flagged(M.desc, UPD), M), "n_dofs": M.n_dofs,
               "transfer": mf.Transfer.from_meshes(meshes[l - 1], M) if l else None} for l, M in enumerate(meshes)]
    return levels, meshes, meshes, meshes[-1].n_dofs, f"3D p=4 {n}^3 cells"


def bench_case(case, nt, rounds):
    levels, keep, meshes, n_active, name = build(case, nt)
    for lev, M in zip(levels, meshes):  # the coefficient update the refresh follows
        x = M.arrays()["quadrature_points"].astype(np.float64)
        c = mf.DeviceVector(x.shape[0] * x.shape[1], nt)
        c.from_host((1.0 + x[..., 0] ** 2 + 2.0 * x[..., 1] ** 2 + 3.0 * x[..., 2] ** 2).reshape(-1))
        lev["op"].update_coefficients(c)
        mf.synchronize()
    n = [lev["n_dofs"] for lev in levels]
    state = {"V": mf.VCycle(levels, F64, n_active, keep=keep)}
    lam = state["V"].lambda_max()  # the estimates of creation, on the updated levels
    state["V"].refresh()  # the first refresh allocates
    V0 = mf.VCycle(levels[:1], nt, n[0], lambda_max=[1.0], coarse=mf.VCYCLE_COARSE_DENSE)
    V0.refresh()
    info = state["V"].refresh_status()
    state["V_refreshed_lambda"] = state["V"].lambda_max()  # those of the refresh: the same iteration on the device
    dinv = [mf.DeviceVector(k, nt) for k in n]
    ws = [mf.DeviceVector(mf.eig_workspace_bytes(k, nt) // 8) for k in n]
    steps = []
    for l, lev in enumerate(levels):  # the step counts the refresh enqueues
        lev["op"].compute_inverse_diagonal(dinv[l])
        steps.append(mf.estimate_lambda_max(lev["op"], dinv[l], 15, with_steps=True)[1])

    def recreate():
        state["V"].destroy()
        state["V"] = mf.VCycle(levels, F64, n_active, keep=keep)

    def recreate_coarse():
        state.pop("V0", None)
        state["V0"] = mf.VCycle(levels[:1], nt, n[0], lambda_max=[1.0], coarse=mf.VCYCLE_COARSE_DENSE)

    variants = {
        "refresh": lambda: state["V"].refresh(),
        "recreate": recreate,
        "refresh_diagonals": lambda: [levels[l]["op"].compute_inverse_diagonal(dinv[l]) for l in range(1, len(n))],
        "recreate_diagonals": lambda: [levels[l]["op"].compute_inverse_diagonal(dinv[l]) for l in range(len(n))],
        "refresh_estimates": lambda: [mf.estimate_lambda_max_enqueue(levels[l]["op"], dinv[l], 15, steps[l], ws[l])
                                      for l in range(1, len(n))],
        "recreate_estimates": lambda: [mf.estimate_lambda_max(levels[l]["op"], dinv[l], 15) for l in range(len(n))],
        "refresh_coarse": lambda: V0.refresh(),
        "recreate_coarse": recreate_coarse,
    }
    times = {k: [] for k in variants}
    for rnd in range(rounds + 1):  # round 0 is the untimed ramp
        for key, fn in variants.items():
            t = wall_us(fn)
            if rnd:
                times[key].append(t)
        state["V"].refresh()  # the object of the next round has had its first refresh
    fresh = state["V_refreshed_lambda"]
    out = {"config": name, "levels_type": "double" if nt == F64 else "float", "n_levels": len(n), "n_active": n_active,
           "n_dofs_level_0": n[0], "rounds": rounds, "eig_steps_per_level": steps[1:], "eig_status_max": info.eig_status_max,
           "lambda_max_rel_difference": float(np.max(np.abs(lam[1:] - fresh[1:]) / fresh[1:])) if len(n) > 1 else 0.0}
    for key, ts in times.items():
        out[f"{key}_us"], out[f"{key}_min_max_us"] = stats(ts)
    out["recreate_over_refresh"] = round(out["recreate_us"] / out["refresh_us"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="8,32,64,adaptive")
    args = ap.parse_args()
    for case in [c for c in args.cases.split(",") if c]:
        for nt in (F64, F32):
            bench_case(case, nt, args.rounds)


if __name__ == "__main__":
    main()
