#!/usr/bin/env python3
"""Cost of a device-side coefficient update (mfgpu_update_coefficients, MFGPU_UPDATABLE_COEFFICIENTS) at the headline mesh
(p = 4, 54^3 cells, double), in one process:

  update    ms per mfgpu_update_coefficients between two hipEvents on the launch stream (torch.cuda.Event, as bench.py
            takes its stream from torch), blocks of K updates alternating between two coefficient arrays
  vmult     ms per mfgpu_vmult of the same handle, measured the same way, blocks alternating with the update blocks
  recreate  what a caller had to do before: mfgpu_destroy + mfgpu_create with the new coefficient as a host array --
            WALL time (the host planner, build_plane_records and all uploads run again), next to the wall time of one
            update followed by a device synchronisation

after the clock ramp bench.py uses (--ramp-steps untimed applies).  By bytes the fold (coefficient and JxW read, folded
value written) and the plane kernels' relayout (read, write) move 40 B per quadrature point.

  python3 tools/bench_update.py [--n 54] [--degree 4] [--steps 50] [--rounds 7] [--recreate 3] [--out FILE.json]"""
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
import torch  # noqa: E402

import pymfgpu as mf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=54)
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ramp-steps", type=int, default=2000)
    ap.add_argument("--recreate", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    mesh = mf.Mesh.uniform(3, args.degree, args.n)
    N, npts = mesh.n_dofs, mesh.n_cells * mesh.nd
    q = mesh.arrays()["quadrature_points"].astype(np.float64)
    coefs = [np.ascontiguousarray(1.0 + s * np.sum(q * q, axis=-1)).reshape(-1) for s in (1.0, 0.5)]
    mesh.desc.coefficient = coefs[0].ctypes.data
    plain_bytes = mf.Operator(mesh.desc, mesh).memory_consumption()
    mesh.desc.flags |= mf.UPDATABLE_COEFFICIENTS
    op = mf.Operator(mesh.desc, mesh)
    dev = [mf.DeviceVector(npts) for _ in coefs]
    for d, c in zip(dev, coefs):
        d.from_host(c)
    a, b = mf.DeviceVector(N), mf.DeviceVector(N)

    def timed(fn, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(count):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / count

    def vmult(i):
        nonlocal a, b
        op.vmult(b, a, stream)
        a, b = b, a
        if i % 50 == 49:
            a.mul(1e-20, stream)

    def update(i):
        op.update_coefficients(dev[i & 1], stream=stream)

    def vmult_block(count):
        a.fill(0.1, stream)
        return timed(vmult, count)

    for _ in range(0, args.ramp_steps, 250):
        vmult_block(250)
    t_upd, t_vm = [], []
    for _ in range(args.rounds):
        t_upd.append(timed(update, args.steps))
        t_vm.append(vmult_block(args.steps))
    # wall time of one update with a synchronisation, and of the path it replaces
    wall_upd = []
    for i in range(args.rounds):
        mf.synchronize()
        t = time.perf_counter()
        update(i)
        mf.synchronize()
        wall_upd.append((time.perf_counter() - t) * 1e3)
    wall_re = []
    for i in range(args.recreate):
        mf.synchronize()
        t = time.perf_counter()
        op.clear()
        mesh.desc.coefficient = coefs[(i + 1) & 1].ctypes.data
        op = mf.Operator(mesh.desc, mesh)
        mf.synchronize()
        wall_re.append((time.perf_counter() - t) * 1e3)
    upd, vm = statistics.median(t_upd), statistics.median(t_vm)
    out = {
        "degree": args.degree, "n_per_dir": args.n, "n_dofs": N, "n_cells": mesh.n_cells, "kernel": op.kernel_name(),
        "steps_per_block": args.steps, "rounds": args.rounds,
        "ms_per_update": round(upd, 5), "range_update": [round(min(t_upd), 5), round(max(t_upd), 5)],
        "ms_per_vmult": round(vm, 5), "range_vmult": [round(min(t_vm), 5), round(max(t_vm), 5)],
        "update_over_vmult": round(upd / vm, 3),
        "bytes_per_update_model": 40 * npts, "update_gb_per_s_model": round(40 * npts / (upd * 1e-3) / 1e9, 1),
        "wall_ms_update_and_sync": round(statistics.median(wall_upd), 4),
        "wall_ms_destroy_and_create": round(statistics.median(wall_re), 2),
        "range_destroy_and_create": [round(min(wall_re), 2), round(max(wall_re), 2)],
        "recreate_over_update": round(statistics.median(wall_re) / statistics.median(wall_upd), 1),
        "memory_consumption_plain": plain_bytes, "memory_consumption_updatable": op.memory_consumption(),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
