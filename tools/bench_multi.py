#!/usr/bin/env python3
"""Time per vector of mfgpu_vmult_multi on the BALL domain (3D hyper_ball, general-geometry path apply_batches_g), in one
process, between two hipEvents on the launch stream (torch.cuda.Event, as bench.py takes its stream from torch), after the
clock ramp bench.py uses (--ramp-steps untimed applies):

  fused2   MFGPU_MULTI_FUSED on 2 vectors (apply_batches_g<.., 2> + reduce_classes<.., 2>)
  fused3   MFGPU_MULTI_FUSED on 3 vectors
  loop     MFGPU_MULTI_LOOP on 3 vectors: three single-vector applies behind one call
  vmult    plain mfgpu_vmult
  auto     the default mode on 3 vectors (what the dispatch table picks)

in --rounds interleaved blocks of --steps calls each; reported: median and min-max of the blocks, per VECTOR.  loop and
vmult run the single-vector kernels unchanged, so they are the baseline.  Byte model per apply:
metric 48 B (float 24 B) per quadrature point, + 8 / 4 B with a mass term, read once per group; per vector 2 x 8 B per
dof (source gather, destination store) plus the partial sums of the shared dofs written and read once.

  python3 tools/bench_multi.py [--configs p:n_ref:f64|f32,...] [--steps 30] [--rounds 7] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dealii-cuda_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import pymfgpu as mf  # noqa: E402


def measure(p, n_ref, nt, args, stream):
    mesh = mf.Mesh.ball(3, p, n_ref, number_type=nt)
    op = mf.Operator(mesh.desc, mesh)
    N, es = mesh.n_dofs, 8 if nt == mf.F64 else 4
    st = op.plan_stats()
    a, b = mf.DeviceVector(3 * N, nt), mf.DeviceVector(3 * N, nt)
    op.vmult_multi(b, a, 3, mode=mf.MULTI_FUSED, stream=stream)  # (allocates the halo buffers of a group)
    mem = op.memory_consumption()

    def block(mode, nv, count):
        """ms per vector of `count` calls; the vectors are swapped and rescaled as bench.py does"""
        nonlocal a, b
        a.fill(0.1, stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(count):
            if mode == "vmult":
                op.vmult(b, a, stream)
            else:
                op.vmult_multi(b, a, nv, mode={"fused": mf.MULTI_FUSED, "loop": mf.MULTI_LOOP, "auto": None}[mode],
                               stream=stream)
            a, b = b, a
            if i % 50 == 49:
                a.mul(1e-20, stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (count * nv)

    for _ in range(0, args.ramp_steps, 250):
        block("vmult", 1, 250)
    legs = {"fused2": ("fused", 2), "fused3": ("fused", 3), "loop": ("loop", 3), "vmult": ("vmult", 1), "auto": ("auto", 3)}
    t = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (mode, nv) in legs.items():
            t[k].append(block(mode, nv, args.steps))
    npts = mesh.n_cells * mesh.nd
    metric = (6 * es) * npts
    per_vec = 2 * es * N + 2 * es * st["rmw_adds_or_halo_slots"]
    out = {"degree": p, "n_ref": n_ref, "number_type": "f64" if nt == mf.F64 else "f32", "n_dofs": N, "n_cells": mesh.n_cells,
           "kernel": op.kernel_name(), "multi_width": op.multi_width(), "n_batches": st["n_batches"],
           "max_batch_dofs": st["max_batch_dofs"], "steps_per_block": args.steps, "rounds": args.rounds,
           "memory_consumption_with_halo_buffers": mem,
           "model_bytes_metric": metric, "model_bytes_per_vector": per_vec}
    for k, (mode, nv) in legs.items():
        med = statistics.median(t[k])
        width = nv if mode == "fused" else 1
        out[k] = {"ms_per_vector": round(med, 5), "range": [round(min(t[k]), 5), round(max(t[k]), 5)],
                  "dofs_per_s": round(N / (med * 1e-3), 0)}
        if mode != "auto":
            out[k]["model_tb_per_s"] = round((metric / width + per_vec) / (med * 1e-3) / 1e12, 3)
    base = out["loop"]["ms_per_vector"]
    for k in ("fused2", "fused3", "auto"):
        out[k]["speedup_over_loop"] = round(base / out[k]["ms_per_vector"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="4:5:f64,2:6:f64,4:5:f32")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ramp-steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for cfg in args.configs.split(","):
        p, n_ref, nt = cfg.split(":")
        r = measure(int(p), int(n_ref), mf.F64 if nt == "f64" else mf.F32, args, stream)
        print(json.dumps(r), flush=True)
        results.append(r)
        if args.out:  # (after every configuration: a later one may not fit the time)
            with open(args.out, "w") as f:
                json.dump({"configs": results}, f, indent=1)


if __name__ == "__main__":
    main()
