#!/usr/bin/env python3
"""Time of one V-cycle application: the shim's schedule through the separate C-ABI calls against the one-object
mfgpu_vcycle, on the same level operators, transfers and copy pairs, in the same process, alternating.
  shim    MultigridPreconditioner::level_v_step of host/mfgpu_shim_mg.h call for call -- zero fills, fused Chebyshev
          smoother, vmult + interface_down + add + sadd, restrict_and_add, prolongate + add, interface_up + equ + add --
          with MGCoarseIterative of host/poisson_mg.cc on level 0: a host-looped CG with two blocking reductions per
          iteration, to a relative max(1e-10, 100 eps)
  vcycle  VCycle.apply (dense coarse solve)
  vcycle_cg  the same with MFGPU_VCYCLE_COARSE_CG forced and its default of n_dofs(0) enqueued iterations per apply (the
          mode AUTO takes above 2048 level-0 dofs), and vcycle_cg_capped with coarse_max_iterations = the host CG's count
Uniform 3D p = 4 at 8^3, 32^3 and 64^3 cells (levels 1, 2, 4 ... cells per direction) and the adaptive p = 4 mesh of
poisson-mg-3d-p4-adaptive 6; double levels and float levels under double active vectors; lambda_max estimated once and
handed to both.  Median of the rounds with the spread.  Reported separately: the coarse solve alone in both forms (host
CG: time and iteration count; device: a one-level VCycle on the level-0 operator, i.e. copy in, dense solve, copy out), and
with --drivers the wall time of poisson-mg-3d-p4-devcg against poisson-mg-3d-p4-devmg.
usage: tools/bench_vcycle.py [--rounds R] [--cases 8,32,64,adaptive] [--drivers N_REF]   -> one JSON line per row"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the library: libmfgpu.so binds to the HIP runtime torch brings)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-cuda_amd"))
import pymfgpu as mf  # noqa: E402

DEGREE, RANGE = 5, 15.0
F64, F32 = mf.F64, mf.F32


class LevelOp:
    """the level matrix of a levels entry (an Operator, or a Level's operator) with what mf.CG needs"""

    def __init__(self, lev, nt):
        self.op, self._n, self.number_type = lev["op"], lev["n_dofs"], nt
        self._h = mf._op_handle(lev["op"])

    def n(self):
        return self._n

    def vmult(self, dst, src):
        mf._check(mf.lib().mfgpu_vmult(self._h, dst.ptr, src.ptr, None))


class ShimVcycle:
    def __init__(self, levels, nt, n_active, lmax):
        self.levels, self.nt, self.nl, self.n_active = levels, nt, len(levels), n_active
        self.ops = [LevelOp(lev, nt) for lev in levels]
        self.n = [lev["n_dofs"] for lev in levels]
        vec = lambda: [mf.DeviceVector(n, nt) for n in self.n]
        self.defect, self.sol, self.tmp, self.edge, self.dinv, self.r, self.t, self.upd = (vec() for _ in range(8))
        for op, dinv in zip(self.ops, self.dinv):
            mf._check(mf.lib().mfgpu_compute_inverse_diagonal(op._h, dinv.ptr, None))
        self.cheb = [mf.cg_chebyshev_scalars(DEGREE, lm, RANGE) for lm in lmax]
        self.pairs = levels[0].get("to_mg") is not None
        n0 = self.n[0]
        self.cr, self.cp, self.cq = (mf.DeviceVector(n0, nt) for _ in range(3))
        self.coarse_tol = max(1e-10, 100.0 * np.finfo(mf.np_dtype(nt)).eps)
        self.coarse_iterations = 0

    def coarse(self):  # MGCoarseIterative::operator()
        x, b, r, p, q, A = self.sol[0], self.defect[0], self.cr, self.cp, self.cq, self.ops[0]
        x.fill(0.0)
        r.equ(1.0, b)
        p.equ(1.0, r)
        rr = r.dot(r)
        tol = self.coarse_tol * np.sqrt(rr)
        it = 0
        while it < self.n[0] and np.sqrt(rr) > tol:
            A.vmult(q, p)
            alpha = rr / p.dot(q)
            x.add(alpha, p)
            r.add(-alpha, q)
            rr_new = r.dot(r)
            p.sadd(rr_new / rr, 1.0, r)
            rr = rr_new
            it += 1
        self.coarse_iterations = it

    def smooth(self, l, b, zero_start):  # PreconditionChebyshev::run_fused
        A, x, f, n, nt = self.ops[l], self.sol[l], self.cheb[l], self.n[l], self.nt
        if not zero_start:
            A.vmult(self.t[l], x)
        mf.chebyshev_start(x, self.upd[l], self.r[l], b, None if zero_start else self.t[l], self.dinv[l], f[0], zero_start, n, nt)
        for k in range(1, DEGREE):
            A.vmult(self.t[l], self.upd[l])
            mf.chebyshev_update(x, self.upd[l], self.r[l], self.t[l], self.dinv[l], f[2 * k - 1], f[2 * k], n, nt)

    def v_step(self, l):
        if l == 0:
            self.coarse()
            return
        lev, A = self.levels[l], self.ops[l]
        defect, sol, tmp, edge = self.defect, self.sol, self.tmp, self.edge
        has_edges = lev.get("has_edges", False)
        self.smooth(l, defect[l], True)
        A.vmult(tmp[l], sol[l])
        if has_edges:
            lev["op"].vmult_interface_down(edge[l], sol[l])
            tmp[l].add(1.0, edge[l])
        tmp[l].sadd(-1.0, 1.0, defect[l])
        lev["transfer"].restrict_and_add(defect[l - 1], tmp[l])
        sol[l - 1].fill(0.0)
        self.v_step(l - 1)
        lev["transfer"].prolongate(tmp[l], sol[l - 1])
        sol[l].add(1.0, tmp[l])
        if has_edges:
            lev["op"].vmult_interface_up(edge[l], sol[l])
            tmp[l].equ(1.0, defect[l])
            tmp[l].add(-1.0, edge[l])
            self.smooth(l, tmp[l], False)
        else:
            self.smooth(l, defect[l], False)

    def apply(self, z, r):  # PreconditionMG::vmult, double active vectors
        top = self.nl - 1
        for l in range(self.nl):
            self.defect[l].fill(0.0)
            if self.pairs:
                mf.copy_pairs_convert(self.levels[l]["to_mg"], self.defect[l], self.nt, r, F64)
        if not self.pairs:
            mf.vec_convert(self.defect[top], self.nt, r, F64, self.n[top])
        self.v_step(top)
        if not self.pairs:
            mf.vec_convert(z, F64, self.sol[top], self.nt, self.n[top])
            return
        z.fill(0.0)
        for l in range(self.nl):
            mf.copy_pairs_convert(self.levels[l]["from_mg"], z, F64, self.sol[l], self.nt)


def timed(fn, reps):
    mf.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    mf.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def stats(ts):
    return round(float(np.median(ts)), 1), [round(min(ts), 1), round(max(ts), 1)]


def bench_case(case, nt, rounds):
    if case == "adaptive":
        mesh = mf.Mesh.adaptive_mg(3, 4, 6, number_type=nt)
        levels, keep = mf.VCycle.hierarchy_levels(mesh)
        n_active, name = mesh.n_dofs, "adaptive 3D p=4 n_ref 6"
    else:
        n = int(case)
        meshes = [mf.Mesh.uniform(3, 4, c, number_type=nt) for c in (1 << k for k in range(n.bit_length()))]
        levels = [{"op": mf.Operator(M.desc, M), "n_dofs": M.n_dofs,
                   "transfer": mf.Transfer.from_meshes(meshes[l - 1], M) if l else None} for l, M in enumerate(meshes)]
        keep, n_active, name = meshes, meshes[-1].n_dofs, f"3D p=4 {n}^3 cells"
    V = mf.VCycle(levels, F64, n_active, keep=keep)  # estimates lambda_max
    S = ShimVcycle(levels, nt, n_active, V.lambda_max())
    V0 = mf.VCycle(levels[:1], nt, levels[0]["n_dofs"], lambda_max=[1.0])  # the dense coarse solve alone
    rh = np.random.default_rng(0).standard_normal(n_active)
    r, zs, zv = mf.DeviceVector(n_active), mf.DeviceVector(n_active), mf.DeviceVector(n_active)
    r.from_host(rh)
    S.apply(zs, r)
    V.apply(zv, r)
    mf.synchronize()
    a, b = zs.to_host(), zv.to_host()
    Vcg = mf.VCycle(levels, F64, n_active, lambda_max=V.lambda_max(), coarse=mf.VCYCLE_COARSE_CG)
    Vcap = mf.VCycle(levels, F64, n_active, lambda_max=V.lambda_max(), coarse=mf.VCYCLE_COARSE_CG,
                     coarse_max_iterations=max(S.coarse_iterations, 1))
    diff = float(np.linalg.norm(a - b) / np.linalg.norm(a))
    reps = 10 if n_active < 5_000_000 else 4
    z0 = mf.DeviceVector(levels[0]["n_dofs"], nt)
    variants = {"shim": lambda: S.apply(zs, r), "vcycle": lambda: V.apply(zv, r), "vcycle_cg": lambda: Vcg.apply(zv, r),
                "vcycle_cg_capped": lambda: Vcap.apply(zv, r), "coarse_host": S.coarse,
                "coarse_device": lambda: V0.apply(z0, S.defect[0])}
    times = {k: [] for k in variants}
    for rnd in range(rounds + 1):  # round 0 is the untimed ramp
        for key, fn in variants.items():
            t = timed(fn, reps)
            if rnd:
                times[key].append(t)
    out = {"config": name, "levels_type": "double" if nt == F64 else "float", "n_levels": len(levels), "n_active": n_active,
           "n_dofs_level_0": levels[0]["n_dofs"], "rounds": rounds, "applies_per_round": reps,
           "rel_l2_difference_shim_vs_vcycle": diff, "coarse_host_cg_iterations": S.coarse_iterations}
    for key, ts in times.items():
        out[f"{key}_us"], out[f"{key}_min_max_us"] = stats(ts)
    out["shim_over_vcycle"] = round(out["shim_us"] / out["vcycle_us"], 3)
    print(json.dumps(out), flush=True)


def bench_drivers(n_ref, rounds):
    exe = [os.path.join(ROOT, "dealii-cuda_amd", "host", "bin", e) for e in ("poisson-mg-3d-p4-devcg", "poisson-mg-3d-p4-devmg")]
    walls, its = {e: [] for e in exe}, {}
    for rnd in range(rounds + 1):
        for e in exe:
            out = subprocess.run([e, str(n_ref)], capture_output=True, text=True, timeout=600, check=True).stdout.split()
            its[e] = int(out[4])
            if rnd:
                walls[e].append(float(out[5]))
    row = {"config": f"poisson-mg-3d-p4 {n_ref}: solve wall seconds", "rounds": rounds}
    for e in exe:
        key = os.path.basename(e)
        row[f"{key}_s"] = round(float(np.median(walls[e])), 4)
        row[f"{key}_min_max_s"] = [round(min(walls[e]), 4), round(max(walls[e]), 4)]
        row[f"{key}_iterations"] = its[e]
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="8,32,64,adaptive")
    ap.add_argument("--drivers", type=int, default=0, help="n_ref of the driver comparison; 0 = skip")
    args = ap.parse_args()
    for case in [c for c in args.cases.split(",") if c]:
        for nt in (F64, F32):
            bench_case(case, nt, args.rounds)
    if args.drivers:
        bench_drivers(args.drivers, args.rounds)


if __name__ == "__main__":
    main()
