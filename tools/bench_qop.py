#!/usr/bin/env python3
"""Cost of the quadrature-point operator (mfgpu_qop_*) and of mfgpu_integrator_integrate, 3D, p = 4 (double), on the
uniform 64^3 cube and on Mesh.adaptive(3, 4, 6), one mesh after the other:

  1  Operator.vmult                                   the hot path, the yardstick
  2  Integrator.evaluate, gradients                   the first half of the unfused route
  3  Integrator.integrate, gradients                  its second half
  4  QpOperator.vmult, scalar diffusion               the term set of row 1
  5  QpOperator.vmult, all five terms (tensor D)
  6  the unfused route for the term set of row 4: evaluate + one device multiply + integrate

Times are us per call between two device events on the launch stream, in blocks of --steps calls that alternate between
all the rows, --rounds rounds ([min, max] and median), after untimed warm-up blocks.  `model_bytes_per_point` is what the
algorithm needs per quadrature point on a uniform-J0 mesh (ND = 125 points and about 64 dofs per cell), a lower bound of
what it moves:
  1  8 coefficient + 16 per dof (src, dst)                                        ~ 16
  2  4 loc2glob + 8 src (gathered) + 24 gradients written                           36
  3  24 gradients + 8 JxW + 8 local written, gather 8 local + 4 index + 12 per dof  58
  4  4 loc2glob + 8 src + 1 mask + 8 folded + 8 local, gather 12 + 12 per dof       47
  5  the same with 128 folded bytes                                                167
  6  rows 2 + 3 + the multiply (24 + 24 read, 24 written)                          166
General geometry adds 72 B (inv_jac) to rows 2 and 3 and makes the scalar diffusion of row 4 72 folded bytes.

  python3 tools/bench_qop.py [--steps 10] [--rounds 7] [--n 64] [--n-ref 6] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dealii-cuda_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pymfgpu as mf  # noqa: E402

DIM, P, ND = 3, 4, 125
MODEL = {"1_operator_vmult": 16, "2_evaluate_gradients": 36, "3_integrate_gradients": 58, "4_qop_scalar_diffusion": 47,
         "5_qop_all_terms": 167, "6_unfused_scalar_diffusion": 166}


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def bench_mesh(name, mesh, args):
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda", 0)
    op = mf.Operator(mesh.desc, mesh)
    flags = mesh.desc.flags
    mesh.desc.flags = flags | mf.UPDATABLE_COEFFICIENTS
    it = mf.Integrator(mesh.desc, mesh)
    mesh.desc.flags = flags
    nc, nd, npts = mesh.n_cells, mesh.n_dofs, mesh.n_cells * ND
    gen = torch.Generator(device=dev).manual_seed(0)

    def rand(*shape):
        return torch.randn(*shape, dtype=torch.float64, device=dev, generator=gen)

    src, dst, dst2 = rand(nd), rand(nd), rand(nd)
    con = torch.from_numpy(mesh.arrays()["constrained_dofs"].astype(np.int64)).to(dev)
    src[con] = 0.0  # the operators read constrained entries as 0, evaluate reads them: the same input for every row
    a = 1.0 + rand(npts) ** 2
    a3 = a[:, None].expand(npts, DIM).contiguous().view(-1)
    grad, flux = rand(npts * DIM), rand(npts * DIM)
    q4 = mf.QpOperator(it, mf.QOP_DIFFUSION_SCALAR)
    q4.set_coefficients(diffusion=a)
    q5 = mf.QpOperator(it, mf.QOP_DIFFUSION_TENSOR | mf.QOP_CONVECTION | mf.QOP_FLUX | mf.QOP_REACTION)
    q5.set_coefficients(diffusion=rand(npts * 9), convection=rand(npts * 3), flux=rand(npts * 3), reaction=rand(npts))
    torch.cuda.synchronize()

    def unfused():
        it.evaluate(src, None, grad, stream)
        torch.mul(grad, a3, out=flux)
        it.integrate(dst2, None, flux, stream)

    calls = {"1_operator_vmult": lambda: op.vmult(dst, src, stream),
             "2_evaluate_gradients": lambda: it.evaluate(src, None, grad, stream),
             "3_integrate_gradients": lambda: it.integrate(dst2, None, flux, stream),
             "4_qop_scalar_diffusion": lambda: q4.vmult(dst, src, stream=stream),
             "5_qop_all_terms": lambda: q5.vmult(dst, src, stream=stream),
             "6_unfused_scalar_diffusion": unfused}
    for fn in calls.values():
        timed(fn, args.warmup)
    # rows 4 and 6 compute the same vector on the free rows (the fused operator adds identity rows)
    q4.vmult(dst, src, stream=stream)
    unfused()
    torch.cuda.synchronize()
    d = dst.clone()
    d[con] = 0.0
    out = {"mesh": name, "cells": nc, "dofs": nd, "points": npts, "general_geometry": not (flags & mf.UNIFORM_J0),
           "steps_per_block": args.steps, "rounds": args.rounds, "kernel": op.kernel_name(),
           "model_bytes_per_point": MODEL,
           "fused_against_unfused_rel_l2": float((d - dst2).norm() / dst2.norm()),
           "qop_bytes": {"4": q4.memory_consumption(), "5": q5.memory_consumption()}}
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            times[k].append(timed(fn, args.steps))
    med = {k: statistics.median(t) for k, t in times.items()}
    for k in calls:
        out[f"us_{k}"] = round(med[k] * 1e3, 1)
        out[f"range_us_{k}"] = [round(min(times[k]) * 1e3, 1), round(max(times[k]) * 1e3, 1)]
        out[f"model_gb_per_s_{k}"] = round(MODEL[k] * npts / (med[k] * 1e-3) / 1e9, 1)
        out[f"over_row1_{k}"] = round(med[k] / med["1_operator_vmult"], 2)
        out[f"over_row6_{k}"] = round(med[k] / med["6_unfused_scalar_diffusion"], 2)
    out["row4_verdict_against_row1"] = "SLOWER" if med["4_qop_scalar_diffusion"] > med["1_operator_vmult"] else "FASTER"
    out["row4_verdict_against_row6"] = "SLOWER" if med["4_qop_scalar_diffusion"] > med["6_unfused_scalar_diffusion"] else "FASTER"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--n-ref", type=int, default=6)
    ap.add_argument("--meshes", default="uniform,adaptive")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = []
    for name in args.meshes.split(","):
        mesh = mf.Mesh.uniform(DIM, P, args.n) if name == "uniform" else mf.Mesh.adaptive(DIM, P, args.n_ref)
        out.append(bench_mesh(name, mesh, args))
        print(json.dumps(out[-1]), flush=True)
        del mesh
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
