#!/usr/bin/env python3
"""Cost of point location on the device (mfgpu_locator_locate), 3D, p = 4 (double), on the uniform 64^3 cube, on
Mesh.adaptive(3, 4, 6) and on the ball at n_ref 4, one mesh after the other in one process:

  caller   --points (1 M) uniformly random points (in the cube; in the ball |x| <= 0.9) in the order they were drawn
  sorted   the same points sorted by the cell that holds them
  percell  one random point per cell, in cell order
each with and without correct hints (the cells of an earlier call).  Next to them, in the same process:
  host     mfgpu_locate_points on the first --host-points (100 000) of the same points, one host thread, wall clock,
           scaled to a million points: the yardstick.  Its cells must equal the device's, and xi is compared.
  located  Points.located on the device's result (wall clock: the one synchronising step, download + host plan) and
           Points.evaluate (values and gradients) on it, what the location is for

Times are us per call between two device events on the launch stream, in blocks of --steps calls that alternate between
all the calls, --rounds rounds (median and range), after untimed warm-up blocks.
`model_bytes_per_point` is what one point reads and writes, with ND = 125, counted without reuse: lanes that work on
the same cell at the same time share its Gauss points in cache, so a model rate above the HBM rate (sorted points) is
reuse, not bandwidth:
  24 (x) + 4 (hint, if any) + 8 (the bin's offsets) + per candidate of the bin 4 (cell index) + 48 (box)
  + per Newton step ND * 24 (the cell's Gauss points; rows of 120 contiguous bytes per lane, lanes on different cells)
  + 4 + 24 (cell, xi)
The lower bound counted here takes one box test and two Newton steps per point (an affine cell: the first step lands, the
second confirms), i.e. the hinted case; the unhinted search reads the boxes of the bin's lower cells as well.

  python3 tools/bench_locate.py [--steps 10] [--rounds 7] [--points 1000000] [--meshes uniform,adaptive,ball] [--out F]"""
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

DIM, P, ND = 3, 4, 125
NEWTON_STEPS_AFFINE = 2


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def model_bytes_per_point(hinted):
    return 24 + (4 if hinted else 0) + 8 + (4 + 48) + NEWTON_STEPS_AFFINE * ND * 24 + 28


def u32(n):
    return mf.DeviceVector(max(n, 1), mf.F32)  # 4-byte device memory holding uint32 (pymfgpu.Locator)


def upload(a):
    v = mf.DeviceVector(a.size)
    v.from_host(a)
    return v


def bench_mesh(name, mesh, args):
    stream = torch.cuda.current_stream().cuda_stream
    flags = mesh.desc.flags
    mesh.desc.flags = flags | mf.UPDATABLE_COEFFICIENTS
    it = mf.Integrator(mesh.desc, mesh)
    mesh.desc.flags = flags
    t0 = time.perf_counter()
    loc = mf.Locator(it, mesh.desc)
    out = {"mesh": name, "cells": mesh.n_cells, "dofs": mesh.n_dofs, "steps_per_block": args.steps, "rounds": args.rounds,
           "locator_create_s": round(time.perf_counter() - t0, 3), "locator_bytes": loc.memory_consumption()}
    rng = np.random.default_rng(0)
    n = args.points
    if name == "ball":
        y = rng.standard_normal((n, DIM))
        x = 0.9 * rng.random((n, 1)) ** (1.0 / DIM) * y / np.linalg.norm(y, axis=1, keepdims=True)
    else:
        x = -1.0 + 2.0 * rng.random((n, DIM))
    w = rng.random((mesh.n_cells, ND))
    x_cell = np.einsum("cq,cqd->cd", w / w.sum(axis=1, keepdims=True), mesh.arrays()["quadrature_points"])

    def locate_once(xs):
        d, cell, xi, cnt = upload(xs), u32(len(xs)), mf.DeviceVector(len(xs) * DIM), u32(1)
        loc.locate(d, cell, xi, n_not_found=cnt, stream=stream)
        torch.cuda.synchronize()
        return d, cell, xi, int(mf.Locator.cells_to_host(cnt)[0])

    # the yardstick: the host function on a part of the same points, and the device's result against it
    m = min(args.host_points, n)
    t0 = time.perf_counter()
    hcell, hxi, hmissing = mf.locate_points(mesh.desc, x[:m])
    host_s = time.perf_counter() - t0
    out["host_points"], out["host_s"] = m, round(host_s, 3)
    out["host_s_per_million_points"] = round(host_s / (m / 1e6), 3)
    d_x, d_cell, d_xi, missing = locate_once(x)
    cells = mf.Locator.cells_to_host(d_cell)[:n].copy()
    out["not_found"] = missing
    out["cells_differing_from_host"] = int(np.sum(cells[:m] != hcell))
    out["max_abs_xi_difference_to_host"] = float(np.max(np.abs(d_xi.to_host()[:m * DIM].reshape(m, DIM) - hxi)))
    order = np.argsort(cells, kind="stable")
    sets = {"caller": (d_x, d_cell, d_xi, n), "sorted": locate_once(x[order])[:3] + (n,),
            "percell": locate_once(x_cell)[:3] + (mesh.n_cells,)}
    calls, npts = {}, {}
    keep = []
    for k, (dx, hint, _, count) in sets.items():
        cell, xi = u32(count), mf.DeviceVector(count * DIM)
        keep.append((cell, xi))
        npts[f"{k}_nohint"] = npts[f"{k}_hint"] = count
        calls[f"{k}_nohint"] = lambda dx=dx, cell=cell, xi=xi: loc.locate(dx, cell, xi, stream=stream)
        calls[f"{k}_hint"] = lambda dx=dx, cell=cell, xi=xi, hint=hint: loc.locate(dx, cell, xi, hint=hint, stream=stream)
    # what the location is for: the points object of the located points and its evaluate
    t0 = time.perf_counter()
    pts = mf.Points.located(it, d_cell, d_xi, n, stream)
    out["points_located_create_s"] = round(time.perf_counter() - t0, 3)
    u = upload(rng.standard_normal(mesh.n_dofs))
    v, g = mf.DeviceVector(n), mf.DeviceVector(n * DIM)
    calls["points_evaluate"] = lambda: pts.evaluate(u, v, g, stream)
    npts["points_evaluate"] = n
    for fn in calls.values():
        timed(fn, args.warmup)
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            times[k].append(timed(fn, args.steps))
    med = {k: statistics.median(t) for k, t in times.items()}
    for k in calls:
        out[f"us_{k}"] = round(med[k] * 1e3, 2)
        out[f"range_us_{k}"] = [round(min(times[k]) * 1e3, 2), round(max(times[k]) * 1e3, 2)]
        out[f"mpoints_per_s_{k}"] = round(npts[k] / (med[k] * 1e-3) / 1e6, 1)
        if k != "points_evaluate":
            mb = model_bytes_per_point(k.endswith("_hint"))
            out[f"model_bytes_per_point_{k}"] = mb
            out[f"model_gb_per_s_{k}"] = round(mb * npts[k] / (med[k] * 1e-3) / 1e9, 1)
    dev_s_per_million = med["caller_nohint"] * 1e-3 / (n / 1e6)
    out["device_s_per_million_points"] = round(dev_s_per_million, 6)
    out["host_over_device"] = round(out["host_s_per_million_points"] / dev_s_per_million, 1)
    for a, b, key in (("caller_hint", "caller_nohint", "hint_over_nohint_caller"),
                      ("sorted_hint", "sorted_nohint", "hint_over_nohint_sorted"),
                      ("sorted_nohint", "caller_nohint", "sorted_over_caller"),
                      ("caller_nohint", "points_evaluate", "locate_over_evaluate")):
        r = med[a] / med[b]
        out[key] = round(r, 2)
        out[key + "_verdict"] = "SLOWER" if r > 1.0 else "not slower"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--host-points", type=int, default=100_000)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--n-ref", type=int, default=6)
    ap.add_argument("--ball-ref", type=int, default=4)
    ap.add_argument("--meshes", default="uniform,adaptive,ball")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = []
    for name in args.meshes.split(","):
        if name == "uniform":
            mesh = mf.Mesh.uniform(DIM, P, args.n)
        elif name == "adaptive":
            mesh = mf.Mesh.adaptive(DIM, P, args.n_ref)
        else:
            mesh = mf.Mesh.ball(DIM, P, args.ball_ref)
        out.append(bench_mesh(name, mesh, args))
        print(json.dumps(out[-1]), flush=True)
        del mesh
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
