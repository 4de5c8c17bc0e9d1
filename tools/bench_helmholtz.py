#!/usr/bin/env python3
"""Cost of the mass term: ms per apply of the Laplace operator and of the Helmholtz operator (mfgpu_desc.mass_coefficient)
of the SAME build on the same mesh, in one process.

Both handles are created once; after the clock ramp bench.py uses (2000 untimed applies) blocks of K timed applies
alternate between the two, R rounds, so that drift of the clocks hits both alike.  Reported per configuration: the median
and the spread of the per-block times, their ratio, and the algorithmic bytes B_alg (bench.py: src read once, dst written
once, one coefficient value and one 32-bit index per point) against B_alg + N_cells n^dim sizeof(Number).

  python3 tools/bench_helmholtz.py [--configs C2,C2f,C3,C5,ball] [--steps 200] [--rounds 7] [--out FILE.json]

C2: 54^3 cells, p = 4, double; C2f: the same in float; C3: bmop ADAPTIVE_GRID n_ref = 6 (hanging nodes), p = 4;
C5: 36^3 cells, p = 6; ball: hyper_ball, 4 global refinements, p = 4 (general geometry); Q2: 96^3 cells, p = 2
(apply_batches_x); D2: 1024^2 cells, p = 2 (2D); ball2: hyper_ball, 5 refinements, p = 2."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dealii-cuda_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import pymfgpu as mf  # noqa: E402

CONFIGS = {
    "C2": dict(p=4, nt=mf.F64, make=lambda nt: mf.Mesh.uniform(3, 4, 54, number_type=nt)),
    "C2f": dict(p=4, nt=mf.F32, make=lambda nt: mf.Mesh.uniform(3, 4, 54, number_type=nt)),
    "C3": dict(p=4, nt=mf.F64, make=lambda nt: mf.Mesh.adaptive(3, 4, 6, number_type=nt)),
    "C5": dict(p=6, nt=mf.F64, make=lambda nt: mf.Mesh.uniform(3, 6, 36, number_type=nt)),
    "ball": dict(p=4, nt=mf.F64, make=lambda nt: mf.Mesh.ball(3, 4, 4, number_type=nt)),
    # the pencil families at low degree, where a chunk holds many cells (the MASS instantiations add them in turn)
    "Q2": dict(p=2, nt=mf.F64, make=lambda nt: mf.Mesh.uniform(3, 2, 96, number_type=nt)),
    "D2": dict(p=2, nt=mf.F64, make=lambda nt: mf.Mesh.uniform(2, 2, 1024, number_type=nt)),
    "ball2": dict(p=2, nt=mf.F64, make=lambda nt: mf.Mesh.ball(3, 2, 5, number_type=nt)),
}


def algorithmic_bytes(n_dofs, n_cells, nd, s, entries=1):
    """bench.py's count; `entries` coefficient values per point (6 on the general-geometry path)"""
    return 2 * s * n_dofs + n_cells * nd * (entries * s + 4)


def run(name, cfg, steps, rounds, ramp):
    nt = cfg["nt"]
    mesh = cfg["make"](nt)
    s = 8 if nt == mf.F64 else 4
    N, nc, nd = mesh.n_dofs, mesh.n_cells, mesh.nd
    general = not (mesh.desc.flags & mf.UNIFORM_J0)
    ops = {"laplace": mf.Operator(mesh.desc, mesh)}
    q = mesh.arrays()["quadrature_points"].astype(np.float64)
    mesh.set_mass_coefficient(1.0 + np.sum(q * q, axis=-1))  # c = 1 + |x|^2
    ops["helmholtz"] = mf.Operator(mesh.desc, mesh)
    a, b = mf.DeviceVector(N, nt), mf.DeviceVector(N, nt)

    def block(op, count):
        """count applies of the bmop protocol (dst = A src, swap), the input rescaled first: no overflow within a block"""
        nonlocal a, b
        a.fill(0.1)
        mf.synchronize()
        t = time.perf_counter()
        for i in range(count):
            op.vmult(b, a)
            a, b = b, a
            if i % 50 == 49:  # (an apply multiplies the values by up to ~2.6 at these sizes: 2.6^50 ~ 6e20)
                a.mul(1e-20)
        mf.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    for _ in range(0, ramp, 250):  # clock ramp: `ramp` untimed applies of EACH operator, alternating blocks of 250
        block(ops["laplace"], 250)
        block(ops["helmholtz"], 250)
    times = {k: [] for k in ops}
    for _ in range(rounds):
        for k, op in ops.items():
            times[k].append(block(op, steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    b_alg = algorithmic_bytes(N, nc, nd, s, 6 if general else 1)
    b_mass = b_alg + nc * nd * s
    out = {
        "config": name, "degree": cfg["p"], "number_type": "double" if nt == mf.F64 else "float", "n_dofs": N, "n_cells": nc,
        "kernel_laplace": ops["laplace"].kernel_name(), "kernel_helmholtz": ops["helmholtz"].kernel_name(),
        "steps_per_block": steps, "rounds": rounds,
        "ms_per_apply_laplace": round(med["laplace"], 5), "ms_per_apply_helmholtz": round(med["helmholtz"], 5),
        "range_laplace": [round(min(times["laplace"]), 5), round(max(times["laplace"]), 5)],
        "range_helmholtz": [round(min(times["helmholtz"]), 5), round(max(times["helmholtz"]), 5)],
        "time_ratio": round(med["helmholtz"] / med["laplace"], 4),
        "algorithmic_bytes_laplace": b_alg, "algorithmic_bytes_helmholtz": b_mass, "byte_ratio": round(b_mass / b_alg, 4),
        "memory_consumption_laplace": ops["laplace"].memory_consumption(),
        "memory_consumption_helmholtz": ops["helmholtz"].memory_consumption(),
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C2f,C3,C5,ball,Q2,D2,ball2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ramp-steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = []
    for name in args.configs.split(","):
        r = run(name, CONFIGS[name], args.steps, args.rounds, args.ramp_steps)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"results": results}, f, indent=1)


if __name__ == "__main__":
    main()
