#!/usr/bin/env python3
"""Cost of the gradient-recovery indicator (mfgpu_integrator_recovery_indicator) next to one vmult and one evaluate with
gradients of the same mesh, in one process, on Mesh.adaptive(3, 4, 6) and on the 64^3 cube at p = 4 (double):

  indicator  ms per call between two hipEvents on the launch stream (torch.cuda.Event, as bench.py takes its stream from
             torch): the nodal kernel, the gather and the cell kernel
  vmult      ms per mfgpu_vmult of an operator on the same mesh, measured the same way
  evaluate   ms per mfgpu_integrator_evaluate with gradients only

in blocks of --steps calls that alternate between the three, --rounds rounds (median and range), after untimed warm-up
blocks.  By bytes the indicator's scratch moves 2 * dim * 8 B per cell-local node (local buffers written and read by the
gather) on top of what three evaluates read; the figure printed as `indicator_scratch_gb_per_s` is that scratch traffic over
the indicator's time, a lower bound of what it moves.

With --driver the table of host/poisson_amr.cc is run too: adaptive (n_start_ref, n_cycles, fraction) against uniform
refinement (fraction 1) on the same start mesh, both printed as they come, so that errors can be compared at nearby dof
counts.

  python3 tools/bench_amr.py [--steps 20] [--rounds 7] [--meshes adaptive,cube] [--driver] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dealii-cuda_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pymfgpu as mf  # noqa: E402

BIN = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin")


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def bench_mesh(name, mesh, steps, rounds, warmup):
    stream = torch.cuda.current_stream().cuda_stream
    dim, N, npts = int(mesh.desc.dim), mesh.n_dofs, mesh.n_cells * mesh.nd
    op = mf.Operator(mesh.desc, mesh)
    mesh.desc.flags |= mf.UPDATABLE_COEFFICIENTS
    it = mf.Integrator(mesh.desc, mesh)
    u, v = mf.DeviceVector(N), mf.DeviceVector(N)
    u.from_host(np.random.default_rng(0).standard_normal(N))
    eta, grads = mf.DeviceVector(mesh.n_cells), mf.DeviceVector(npts * dim)
    calls = {
        "indicator": lambda: it.recovery_indicator(u, eta, stream=stream),
        "vmult": lambda: op.vmult(v, u, stream),
        "evaluate": lambda: it.evaluate(u, gradients=grads, stream=stream),
    }
    for fn in calls.values():  # first calls load code objects and allocate the indicator's scratch
        timed(fn, warmup)
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t[k].append(timed(fn, steps))
    out = {"mesh": name, "dim": dim, "degree": int(mesh.desc.degree), "n_cells": mesh.n_cells, "n_dofs": N,
           "kernel": op.kernel_name(), "steps_per_block": steps, "rounds": rounds}
    for k in calls:
        out[f"ms_per_{k}"] = round(statistics.median(t[k]), 5)
        out[f"range_{k}"] = [round(min(t[k]), 5), round(max(t[k]), 5)]
    ind = statistics.median(t["indicator"])
    out["indicator_over_vmult"] = round(ind / statistics.median(t["vmult"]), 2)
    out["indicator_over_evaluate"] = round(ind / statistics.median(t["evaluate"]), 2)
    out["indicator_scratch_gb_per_s"] = round(2 * dim * 8 * npts / (ind * 1e-3) / 1e9, 1)
    return out


def driver_table(exe, n_start_ref, n_cycles, fraction):
    run = subprocess.run([os.path.join(BIN, exe), str(n_start_ref), str(n_cycles), str(fraction)], capture_output=True,
                         text=True, timeout=900)
    if run.returncode != 0:
        raise RuntimeError(f"{exe}: {run.stdout}{run.stderr}")
    keys = ["cycle", "cells", "dofs", "cg_iterations", "cg_iterations_from_zero", "l2_error", "eta", "seconds"]
    rows = [dict(zip(keys, (float(x) if "." in x or "e" in x else int(x) for x in ln.split())))
            for ln in run.stdout.splitlines() if ln and not ln.startswith("#")]
    return {"exe": exe, "n_start_ref": n_start_ref, "fraction": fraction, "cycles": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--meshes", default="adaptive,cube")
    ap.add_argument("--driver", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"meshes": [], "driver": []}
    for name in args.meshes.split(","):
        mesh = mf.Mesh.adaptive(3, 4, 6) if name == "adaptive" else mf.Mesh.uniform(3, 4, 64)
        out["meshes"].append(bench_mesh(name, mesh, args.steps, args.rounds, args.warmup))
        print(json.dumps(out["meshes"][-1]), flush=True)
        del mesh
    if args.driver:
        for exe, start, cycles_a, cycles_u in (("poisson-amr-2d-p2", 3, 8, 4), ("poisson-amr-2d-p4", 2, 7, 4),
                                               ("poisson-amr-3d-p2", 2, 6, 3), ("poisson-amr-3d-p4", 1, 5, 3)):
            for fraction, cycles in ((0.3, cycles_a), (1.0, cycles_u)):
                out["driver"].append(driver_table(exe, start, cycles, fraction))
                print(json.dumps(out["driver"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
