#!/usr/bin/env python3
"""Cost of the vector-valued quadrature-point operator (mfgpu_vqop_*), 3D, p = 4 (double), on the uniform 64^3 cube and
on Mesh.adaptive(3, 4, 6), one mesh after the other:

  1  Operator.vmult                                   the hot path, the yardstick (one scalar field)
  2  QpOperator.vmult, scalar diffusion               one scalar field; three of these move a 3-component field
  3  VectorQpOperator.vmult, isotropic                lambda, mu
  4  VectorQpOperator.vmult, tensor4                  81 folded values per point
  5  VectorQpOperator.vmult, isotropic + mass

Times are us per call between two device events on the launch stream, in blocks of --steps calls that alternate between
all the rows, --rounds rounds ([min, max] and median), after untimed warm-up blocks.  Rows 3-5 are labelled FASTER or
SLOWER against three calls of row 2 (the same number of components; not the same operator: the scalar applies do not
couple the components).  `model_bytes_per_point` is what the algorithm needs per quadrature point on a uniform-J0 mesh
(ND = 125 points and about 64 dofs per cell), a lower bound of what it moves:
  1  8 coefficient + 16 per dof (src, dst)                                                          ~ 16
  2  4 loc2glob + 8 src + 1 flag + 8 folded + 8 local, gather 12 + 12 per dof                         47
  3  4 loc2glob + 3 (8 src + 1 flag) + 16 folded + 3 x 8 local, gather 3 x 12 + 3 x 12 per dof       125   (3 x row 2: 141)
  4  the same with 648 folded bytes                                                                   757
  5  row 3 + 8 folded                                                                                 133
General geometry adds the integrator's 72 B of inv_jac to rows 3 and 5 (read, not folded) and makes row 2's folded
coefficient 72 B.

  python3 tools/bench_vqop.py [--steps 10] [--rounds 7] [--n 64] [--n-ref 6] [--out FILE.json]"""
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

DIM, P, ND = 3, 4, 125
MODEL = {"1_operator_vmult": 16, "2_qop_scalar_diffusion": 47, "3_vqop_isotropic": 125, "4_vqop_tensor4": 757,
         "5_vqop_isotropic_mass": 133}


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

    src, dst = rand(nd), rand(nd)
    vsrc, vdst = rand(DIM * nd), rand(DIM * nd)
    a = 1.0 + rand(npts) ** 2
    q2 = mf.QpOperator(it, mf.QOP_DIFFUSION_SCALAR)
    q2.set_coefficients(diffusion=a)
    q3 = mf.VectorQpOperator(it, mf.VQOP_ISOTROPIC)
    q3.set_coefficients(lam=a, mu=a)
    q5 = mf.VectorQpOperator(it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
    q5.set_coefficients(lam=a, mu=a, mass=a)
    q4 = mf.VectorQpOperator(it, mf.VQOP_TENSOR4)
    c4 = rand(npts * DIM ** 4)
    q4.set_coefficients(tensor=c4)
    torch.cuda.synchronize()
    del c4
    calls = {"1_operator_vmult": lambda: op.vmult(dst, src, stream),
             "2_qop_scalar_diffusion": lambda: q2.vmult(dst, src, stream=stream),
             "3_vqop_isotropic": lambda: q3.vmult(vdst, vsrc, stream=stream),
             "4_vqop_tensor4": lambda: q4.vmult(vdst, vsrc, stream=stream),
             "5_vqop_isotropic_mass": lambda: q5.vmult(vdst, vsrc, stream=stream)}
    for fn in calls.values():
        timed(fn, args.warmup)
    out = {"mesh": name, "cells": nc, "dofs": nd, "points": npts, "general_geometry": not (flags & mf.UNIFORM_J0),
           "steps_per_block": args.steps, "rounds": args.rounds, "kernel": op.kernel_name(),
           "model_bytes_per_point": MODEL,
           "vqop_bytes": {"3": q3.memory_consumption(), "4": q4.memory_consumption(), "5": q5.memory_consumption()}}
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
    three = DIM * med["2_qop_scalar_diffusion"]
    for k in ("3_vqop_isotropic", "4_vqop_tensor4", "5_vqop_isotropic_mass"):
        out[f"over_three_row2_{k}"] = round(med[k] / three, 2)
        out[f"verdict_against_three_row2_{k}"] = "SLOWER" if med[k] > three else "FASTER"
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
