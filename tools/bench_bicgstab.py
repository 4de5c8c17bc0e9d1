#!/usr/bin/env python3
"""Time per BiCGStab iteration: the host-looped solver (six blocking reductions per iteration) against the
device-resident one (mfgpu_bicgstab), eager and replayed from one captured graph.  Uniform 3D p = 4 at 8^3, 32^3 and 64^3
cells, a QpOperator with scalar diffusion and convection, the Jacobi preconditioner, a fixed iteration count with no
convergence exit (tolerance 0) after an untimed ramp; the three variants alternate within the process and the spread
over the rounds is reported.
  host    SolverBicgstab's order of DeviceVector calls (host/mfgpu_shim_qop.h): dot / l2_norm block
  eager   BiCGStab.iterate(K)
  graph   the same iterate(K), captured once and replayed
usage: tools/bench_bicgstab.py [--rounds R] [--sizes 8,32,64]   -> one JSON line per configuration"""
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

BETA = (1.5, -0.75, 0.5)


def dv(a):
    v = mf.DeviceVector(a.size)
    v.from_host(a)
    return v


class HostLoop:
    """SolverBicgstab::solve (host/mfgpu_shim_qop.h) without the convergence exits"""

    def __init__(self, q, N, dinv):
        self.q, self.dinv = q, dinv
        self.r, self.r0, self.p, self.v, self.y, self.s, self.z, self.t = (mf.DeviceVector(N) for _ in range(8))

    def begin(self, x, b):
        self.x = x
        x.fill(0.0)
        self.p.fill(0.0)
        self.v.fill(0.0)
        self.r.equ(1.0, b)
        self.r0.equ(1.0, b)
        self.res = self.r.l2_norm()
        self.rho = self.alpha = self.omega = 1.0

    def iterate(self, k):
        r, r0, p, v, y, s, z, t, x = self.r, self.r0, self.p, self.v, self.y, self.s, self.z, self.t, self.x
        for _ in range(k):
            rho_new = r0.dot(r)
            beta = (rho_new / self.rho) * (self.alpha / self.omega)
            self.rho = rho_new
            p.add(-self.omega, v)
            p.sadd(beta, 1.0, r)
            y.equ(1.0, p)
            y.scale(self.dinv)
            self.q.vmult(v, y)
            self.alpha = self.rho / r0.dot(v)
            s.equ(1.0, r)
            s.add(-self.alpha, v)
            self.half = s.l2_norm()
            z.equ(1.0, s)
            z.scale(self.dinv)
            self.q.vmult(t, z)
            self.omega = t.dot(s) / t.dot(t)
            x.add(self.alpha, y)
            x.add(self.omega, z)
            r.equ(1.0, s)
            r.add(-self.omega, t)
            self.res = r.l2_norm()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="8,32,64")
    args = ap.parse_args()
    for n in (int(s) for s in args.sizes.split(",")):
        mesh = mf.Mesh.uniform(3, 4, n)
        flags = mesh.desc.flags
        mesh.desc.flags = flags | mf.UPDATABLE_COEFFICIENTS  # inv_jac on the device: the folds of the operator
        it = mf.Integrator(mesh.desc, mesh)
        mesh.desc.flags = flags
        N, npts = mesh.n_dofs, mesh.n_cells * mesh.nd
        q = mf.QpOperator(it, mf.QOP_DIFFUSION_SCALAR | mf.QOP_CONVECTION)
        q.set_coefficients(diffusion=dv(np.ones(npts)), convection=dv(np.tile(np.array(BETA), npts)))
        dinv, b, x = mf.DeviceVector(N), mf.DeviceVector(N), mf.DeviceVector(N)
        q.inverse_diagonal(dinv)
        bh = np.random.default_rng(0).standard_normal(N)
        bh[mesh.arrays()["constrained_dofs"]] = 0.0
        b.from_host(bh)
        mf.synchronize()
        K = 30 if n < 64 else 10
        host = HostLoop(q, N, dinv)
        solver = mf.BiCGStab(q, mf.CG_JACOBI, dinv)
        stream = torch.cuda.Stream()
        st = stream.cuda_stream

        def device_begin():
            solver.begin(x, b, 0.0, 1 << 30, st)

        device_begin()
        solver.iterate(2, st)  # ramp: loads every kernel before the capture
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            solver.iterate(K, torch.cuda.current_stream().cuda_stream)

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
            solver.iterate(K, st)
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
                    info = solver.status(st)
                    assert (info.iterations, info.status) == (K, 0), info.as_tuple()
                if rnd:
                    times[name].append(1e6 * t)
        out = {"config": f"3D p=4 {n}^3 cells", "n_dofs": N, "preconditioner": "jacobi", "iterations": K,
               "rounds": args.rounds}
        for name, ts in times.items():
            out[f"{name}_us_per_iteration"] = round(float(np.median(ts)), 2)
            out[f"{name}_min_max_us"] = [round(min(ts), 2), round(max(ts), 2)]
        out["host_over_eager"] = round(out["host_us_per_iteration"] / out["eager_us_per_iteration"], 3)
        out["host_over_graph"] = round(out["host_us_per_iteration"] / out["graph_us_per_iteration"], 3)
        out["residual_after_K_host"] = host.res
        out["residual_after_K_device"] = solver.status(st).residual
        print(json.dumps(out), flush=True)
        del g, solver, host, q, it


if __name__ == "__main__":
    main()
