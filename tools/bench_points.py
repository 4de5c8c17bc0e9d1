#!/usr/bin/env python3
"""Cost of the points object (mfgpu_points_evaluate / mfgpu_points_integrate), 3D, p = 4 (double), on the uniform 64^3
cube and on Mesh.adaptive(3, 4, 6), in one process per mesh:

  a  Points.evaluate at the Gauss points of every cell (125 points per cell, values and gradients) next to
     Integrator.evaluate, which produces the same numbers: the like-for-like yardstick.  The point kernel has no sum
     factorisation across points (every point contracts the whole cell), so it is expected to be slower.
  b  one random point per cell, located on the host by mfgpu_locate_points: its wall clock is the creation time
  c  a regular sampling grid (256^3 on the uniform mesh, where cell and xi are computed directly; --grid-adaptive^3 on
     the adaptive mesh through the host location)
  d  Points.integrate for a and b (with weights)

Times are ms per call between two device events on the launch stream, in blocks of --steps calls that alternate between
all the calls, --rounds rounds (median and range), after untimed warm-up blocks.  Points per second = points / median.
`model_bytes` is what the algorithm needs, a lower bound of what it moves, with ND = 125, per work item (one cell's
share of at most 512 points, n_k points):
  evaluate   4 ND (loc2glob) + 8 ND (u) [+ 24 ND quadrature points on general geometry, with gradients]
             + n_k (24 xi + 4 permutation + 8 value + 24 gradient)
  integrate  4 ND + n_k (24 xi + 4 permutation + 8 weight) + 8 ND (local vector), and for the gather
             12 B per CSR entry (slot index + local entry) + 12 B per dof (offset + result)

  python3 tools/bench_points.py [--steps 10] [--rounds 7] [--n 64] [--n-ref 6] [--grid 256] [--out FILE.json]"""
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


def timed(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / count


def gauss_grid():
    xq = 0.5 * (np.polynomial.legendre.leggauss(P + 1)[0] + 1.0)
    return np.stack(np.meshgrid(xq, xq, xq, indexing="ij"), axis=-1).reshape(-1, 3)[:, ::-1]  # x fastest


def uniform_grid_in_cells(mesh, n, grid):
    """(cell, xi) of the grid^3 cell-centred sampling grid on the uniform n^3 mesh over [-1, 1]^3, without a search: the
    cell of the integer coordinates (ix, iy, iz) is read off the mesh's own quadrature points"""
    q = mesh.arrays()["quadrature_points"]
    corner = np.floor((q.mean(axis=1) + 1.0) * (n / 2.0)).astype(np.int64)  # [cell, 3]
    index = np.full((n, n, n), -1, np.int64)
    index[corner[:, 0], corner[:, 1], corner[:, 2]] = np.arange(mesh.n_cells)
    assert index.min() >= 0
    t = (np.arange(grid) + 0.5) * (n / grid)  # in cell units
    i, f = np.floor(t).astype(np.int64), t - np.floor(t)
    cell = index[i[:, None, None], i[None, :, None], i[None, None, :]].reshape(-1).astype(np.uint32)
    xi = np.stack(np.broadcast_arrays(f[:, None, None], f[None, :, None], f[None, None, :]), axis=-1).reshape(-1, 3)
    return cell, np.ascontiguousarray(xi)


def model_bytes(pts_per_cell_counts, n_dofs, general, what):
    items = int(np.sum((pts_per_cell_counts + 511) // 512))
    n = int(pts_per_cell_counts.sum())
    if what == "evaluate":
        return items * (12 * ND + (24 * ND if general else 0)) + n * 60
    return items * (4 * ND + 8 * ND + 12 * ND) + n * 36 + 12 * n_dofs


def bench_mesh(name, mesh, args, grid_points):
    stream = torch.cuda.current_stream().cuda_stream
    flags = mesh.desc.flags
    mesh.desc.flags = flags | mf.UPDATABLE_COEFFICIENTS
    it = mf.Integrator(mesh.desc, mesh)
    mesh.desc.flags = flags
    general = not (flags & mf.UNIFORM_J0)
    nc, nd = mesh.n_cells, mesh.n_dofs
    rng = np.random.default_rng(0)
    u = mf.DeviceVector(nd)
    u.from_host(rng.standard_normal(nd))
    out = {"mesh": name, "cells": nc, "dofs": nd, "general_geometry": general, "steps_per_block": args.steps,
           "rounds": args.rounds}
    sets = {}
    # a: the Gauss points of every cell
    t0 = time.perf_counter()
    sets["a_gauss"] = mf.Points.in_cells(it, np.repeat(np.arange(nc, dtype=np.uint32), ND), np.tile(gauss_grid(), (nc, 1)))
    out["a_create_in_cells_s"] = round(time.perf_counter() - t0, 3)
    # b: one random point per cell (a convex combination of the cell's Gauss points), located on the host
    w = rng.random((nc, ND))
    x = np.einsum("cq,cqd->cd", w / w.sum(axis=1, keepdims=True), mesh.arrays()["quadrature_points"])
    t0 = time.perf_counter()
    sets["b_one_per_cell"] = mf.Points(it, mesh.desc, x)
    dt = time.perf_counter() - t0
    out["b_create_s"] = round(dt, 3)
    out["create_s_per_million_points"] = round(dt / (nc / 1e6), 2)
    assert sets["b_one_per_cell"].n_not_found == 0
    # c: the sampling grid
    t0 = time.perf_counter()
    if isinstance(grid_points, tuple):
        sets["c_grid"] = mf.Points.in_cells(it, *grid_points)
    else:
        sets["c_grid"] = mf.Points(it, mesh.desc, grid_points)
    out["c_create_s"] = round(time.perf_counter() - t0, 3)
    out["c_not_found"] = sets["c_grid"].n_not_found
    calls, npts, counts = {}, {}, {}
    bufs = []
    for k, pts in sets.items():
        v, g, r, wts = (mf.DeviceVector(m) for m in (pts.n, 3 * pts.n, nd, pts.n))
        wts.from_host(rng.standard_normal(pts.n))
        bufs.append((v, g, r, wts))
        cells = pts.cells
        counts[k] = np.bincount(cells[cells != mf.POINT_NOT_FOUND], minlength=nc)
        npts[k] = pts.n
        calls[f"{k}_evaluate"] = lambda pts=pts, v=v, g=g: pts.evaluate(u, v, g, stream)
        if k != "c_grid":
            calls[f"{k}_integrate"] = lambda pts=pts, r=r, wts=wts: pts.integrate(r, wts, stream)
        out[f"{k}_points"] = pts.n
        out[f"{k}_object_bytes"] = pts.memory_consumption()
    rv, rg = mf.DeviceVector(nc * ND), mf.DeviceVector(3 * nc * ND)
    calls["a_integrator_evaluate"] = lambda: it.evaluate(u, rv, rg, stream)
    for fn in calls.values():
        timed(fn, args.warmup)
    # like for like: the same numbers
    torch.cuda.synchronize()
    ref_v, ref_g = rv.to_host(), rg.to_host()
    got_v, got_g = bufs[0][0].to_host(), bufs[0][1].to_host()
    out["a_max_abs_difference_to_integrator"] = [float(np.max(np.abs(got_v - ref_v))), float(np.max(np.abs(got_g - ref_g)))]
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            times[k].append(timed(fn, args.steps))
    for k in calls:
        ms = statistics.median(times[k])
        key = k.rsplit("_", 1)[0] if not k.startswith("a_integrator") else "a_gauss"
        out[f"us_{k}"] = round(ms * 1e3, 2)
        out[f"range_us_{k}"] = [round(min(times[k]) * 1e3, 2), round(max(times[k]) * 1e3, 2)]
        out[f"mpoints_per_s_{k}"] = round(npts[key] / (ms * 1e-3) / 1e6, 1)
        if not k.startswith("a_integrator"):
            mb = model_bytes(counts[key], nd, general, k.rsplit("_", 1)[1])
            out[f"model_bytes_{k}"] = mb
            out[f"model_gb_per_s_{k}"] = round(mb / (ms * 1e-3) / 1e9, 1)
    ratio = statistics.median(times["a_gauss_evaluate"]) / statistics.median(times["a_integrator_evaluate"])
    out["a_points_over_integrator"] = round(ratio, 2)
    out["a_verdict"] = "SLOWER" if ratio > 1.0 else "not slower"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--n-ref", type=int, default=6)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--grid-adaptive", type=int, default=128)
    ap.add_argument("--meshes", default="uniform,adaptive")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = []
    for name in args.meshes.split(","):
        if name == "uniform":
            mesh = mf.Mesh.uniform(DIM, P, args.n)
            grid = uniform_grid_in_cells(mesh, args.n, args.grid)
        else:
            mesh = mf.Mesh.adaptive(DIM, P, args.n_ref)
            t = -1.0 + (np.arange(args.grid_adaptive) + 0.5) * (2.0 / args.grid_adaptive)
            grid = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
        out.append(bench_mesh(name, mesh, args, grid))
        print(json.dumps(out[-1]), flush=True)
        del mesh, grid
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
