#!/usr/bin/env python3
"""Time per CG iteration: the host-looped solver (three blocking reductions per iteration) against the device-resident
one (mfgpu_cg), eager and replayed from one captured graph.  Uniform 3D p = 4 at 8^3, 32^3 and 64^3 cells, Jacobi and
Chebyshev(5, 15) preconditioners, a fixed iteration count with no convergence exit (tolerance 0) after an untimed ramp;
the three variants alternate within the process and the spread over the rounds is reported.
  host    SolverCG's loop on the DeviceVector calls (dot / l2_norm block; Chebyshev through the fused
          mfgpu_vec_chebyshev_* calls, so that both sides run the same preconditioner launches)
  eager   CG.iterate(K)
  graph   the same iterate(K), captured once and replayed
usage: tools/bench_cg.py [--rounds R] [--sizes 8,32,64]   -> one JSON line per configuration"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-cuda_amd"))
import pymfgpu as mf  # noqa: E402

DEGREE, RANGE = 5, 15.0


def lambda_max(op, dinv, N):
    """1.2 x the power-iteration estimate of the largest eigenvalue of D^-1 A (PreconditionChebyshev::initialize)"""
    v, w = mf.DeviceVector(N), mf.DeviceVector(N)
    v.from_host(np.sin(0.7 * np.arange(N)) + 0.3)
    lam = 1.0
    for _ in range(20):
        op.vmult(w, v)
        w.scale(dinv)
        nw, nv = w.l2_norm(), v.l2_norm()
        lam = nw / nv
        v.equ(1.0 / nw, w)
    return 1.2 * lam


class HostLoop:
    """SolverCG::solve (host/mfgpu_shim_poisson.h) without the convergence exit"""

    def __init__(self, op, N, dinv, cheb):
        self.op, self.N, self.dinv, self.cheb = op, N, dinv, cheb
        self.r, self.z, self.p, self.q = (mf.DeviceVector(N) for _ in range(4))
        self.cr, self.cu, self.ct = (mf.DeviceVector(N) for _ in range(3))

    def prec(self):
        if self.cheb is None:
            self.z.equ(1.0, self.r)
            self.z.scale(self.dinv)
            return
        f = self.cheb
        mf.chebyshev_start(self.z, self.cu, self.cr, self.r, None, self.dinv, f[0], True, self.N, mf.F64)
        for k in range(1, DEGREE):
            self.op.vmult(self.ct, self.cu)
            mf.chebyshev_update(self.z, self.cu, self.cr, self.ct, self.dinv, f[2 * k - 1], f[2 * k], self.N, mf.F64)

    def begin(self, x, b):
        self.x = x
        x.fill(0.0)
        self.r.equ(1.0, b)
        self.prec()
        self.p.equ(1.0, self.z)
        self.rz = self.r.dot(self.z)

    def iterate(self, k):
        for _ in range(k):
            self.op.vmult(self.q, self.p)
            alpha = self.rz / self.p.dot(self.q)
            self.x.add(alpha, self.p)
            self.r.add(-alpha, self.q)
            self.res = self.r.l2_norm()
            self.prec()
            rz_new = self.r.dot(self.z)
            self.p.sadd(rz_new / self.rz, 1.0, self.z)
            self.rz = rz_new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="8,32,64")
    args = ap.parse_args()
    for n in (int(s) for s in args.sizes.split(",")):
        mesh = mf.Mesh.uniform(3, 4, n)
        op = mf.Operator(mesh.desc, mesh)
        N = mesh.n_dofs
        dinv, b, x = mf.DeviceVector(N), mf.DeviceVector(N), mf.DeviceVector(N)
        op.compute_inverse_diagonal(dinv)
        bh = np.random.default_rng(0).standard_normal(N)
        bh[mesh.arrays()["constrained_dofs"]] = 0.0
        b.from_host(bh)
        lam = lambda_max(op, dinv, N)
        for prec in ("jacobi", "chebyshev"):
            K = (60 if prec == "jacobi" else 20) if n < 64 else (30 if prec == "jacobi" else 10)
            cheb = mf.cg_chebyshev_scalars(DEGREE, lam, RANGE) if prec == "chebyshev" else None
            host = HostLoop(op, N, dinv, cheb)
            cg = mf.CG(op, mf.CG_JACOBI if prec == "jacobi" else mf.CG_CHEBYSHEV, dinv, DEGREE, lam, RANGE)
            stream = torch.cuda.Stream()
            st = stream.cuda_stream

            def device_begin():
                cg.begin(x, b, 0.0, 1 << 30, st)

            device_begin()
            cg.iterate(2, st)  # ramp: loads every kernel before the capture
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                cg.iterate(K, torch.cuda.current_stream().cuda_stream)

            def run_host():
                host.begin(x, b)
                mf.synchronize()
                t0 = time.perf_counter()
                host.iterate(K)
                mf.synchronize()
                return (time.perf_counter() - t0) / K

            def run_eager():
                device_begin()
                stream.synchronize()
                t0 = time.perf_counter()
                cg.iterate(K, st)
                stream.synchronize()
                return (time.perf_counter() - t0) / K

            def run_graph():
                device_begin()
                stream.synchronize()
                t0 = time.perf_counter()
                g.replay()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / K

            variants = {"host": run_host, "eager": run_eager, "graph": run_graph}
            times = {k: [] for k in variants}
            for rnd in range(args.rounds + 1):  # round 0 is the untimed ramp
                for name, fn in variants.items():
                    t = fn()
                    if name != "host":  # the timed iterations were real ones: the solve was still running
                        info = cg.status(st)
                        assert (info.iterations, info.status) == (K, 0), info.as_tuple()
                    if rnd:
                        times[name].append(1e6 * t)
            out = {"config": f"3D p=4 {n}^3 cells", "n_dofs": N, "preconditioner": prec, "iterations": K,
                   "rounds": args.rounds}
            for name, ts in times.items():
                out[f"{name}_us_per_iteration"] = round(float(np.median(ts)), 2)
                out[f"{name}_min_max_us"] = [round(min(ts), 2), round(max(ts), 2)]
            out["host_over_eager"] = round(out["host_us_per_iteration"] / out["eager_us_per_iteration"], 3)
            out["host_over_graph"] = round(out["host_us_per_iteration"] / out["graph_us_per_iteration"], 3)
            out["residual_after_K_host"] = host.res
            out["residual_after_K_device"] = cg.status(st).residual
            print(json.dumps(out), flush=True)
            del g, cg, host


if __name__ == "__main__":
    main()
