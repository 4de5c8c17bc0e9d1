#!/usr/bin/env python3
"""Cost of mfgpu_transfer_interpolate next to restrict_and_add and prolongate of the SAME object on the same mesh pair, in
one process: 3D, p = 4 (double), Mesh.adaptive(3, 4, 6) against its coarsening.

  interpolate       ms per call between two hipEvents on the launch stream (torch.cuda.Event, as bench.py takes its
                    stream from torch); the call zeroes the coarse vector first where some coarse dof is stored by nobody
  restrict_and_add  ms per call, measured the same way (the coarse vector keeps accumulating: the values do not matter)
  prolongate        ms per call

in blocks of --steps calls that alternate between the three, --rounds rounds (median and range), after untimed warm-up
blocks.  `interpolate_gb_per_s` is the byte model of the kernel's file header (csrc/mfgpu_transfer_h.hip) over the time:
per coarse cell 4 N coarse indices and 4 * 2^dim fine cell indices, per fine cell 4 N fine indices, 4 B of mask and N T
source entries, and one store per stored coarse dof -- what the algorithm needs, a lower bound of what it moves.

With --driver the table of host/heat_amr.cc is run too: the adaptive run and, where the driver prints it, the run on the
uniform mesh of the finest level reached, so that the errors can be compared per dof.

  python3 tools/bench_adapt.py [--steps 20] [--rounds 7] [--driver] [--out FILE.json]"""
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


def bench_pair(dim, p, n_ref, steps, rounds, warmup):
    stream = torch.cuda.current_stream().cuda_stream
    fine = mf.Mesh.adaptive(dim, p, n_ref)
    coarse = mf.Mesh.coarsening_sequence(fine)[-2]
    t = mf.Transfer.h_hn_interp_from_meshes(coarse, fine)
    plain = mf.Transfer.h_hn_from_meshes(coarse, fine)
    rng = np.random.default_rng(0)
    xf, xc = mf.DeviceVector(fine.n_dofs), mf.DeviceVector(coarse.n_dofs)
    xf.from_host(rng.standard_normal(fine.n_dofs))
    xc.from_host(rng.standard_normal(coarse.n_dofs))
    yf, yc = mf.DeviceVector(fine.n_dofs), mf.DeviceVector(coarse.n_dofs)
    yc.fill(0.0)
    calls = {
        "interpolate": lambda: t.interpolate(yc, xf, stream),
        "restrict_and_add": lambda: t.restrict_and_add(yc, xf, stream),
        "prolongate": lambda: t.prolongate(yf, xc, stream),
    }
    for fn in calls.values():  # first calls load code objects
        timed(fn, warmup)
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(timed(fn, steps))
    nd = (p + 1) ** dim
    out = {"dim": dim, "degree": p, "n_ref": n_ref, "coarse_cells": coarse.n_cells, "fine_cells": fine.n_cells,
           "coarse_dofs": coarse.n_dofs, "fine_dofs": fine.n_dofs, "steps_per_block": steps, "rounds": rounds,
           "image_bytes": t.memory_consumption() - plain.memory_consumption(), "object_bytes": plain.memory_consumption()}
    for k in calls:
        out[f"ms_per_{k}"] = round(statistics.median(times[k]), 5)
        out[f"range_{k}"] = [round(min(times[k]), 5), round(max(times[k]), 5)]
    ms = statistics.median(times["interpolate"])
    out["interpolate_over_restrict_and_add"] = round(ms / statistics.median(times["restrict_and_add"]), 2)
    out["interpolate_over_prolongate"] = round(ms / statistics.median(times["prolongate"]), 2)
    model = coarse.n_cells * (4 * nd + 4 * 2 ** dim) + fine.n_cells * (4 * nd + 4 + 8 * nd) + 8 * coarse.n_dofs
    out["interpolate_model_bytes"] = model
    out["interpolate_gb_per_s"] = round(model / (ms * 1e-3) / 1e9, 1)
    return out


def driver_table(exe, *args):
    run = subprocess.run([os.path.join(BIN, exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        raise RuntimeError(f"{exe}: {run.stdout}{run.stderr}")
    keys = ["step", "time", "cells", "dofs", "families_coarsened", "leaves_refined", "cg_iterations", "l2_error"]
    runs, rows = {}, None
    for ln in run.stdout.splitlines():
        if ln.startswith("# step"):
            rows = runs.setdefault("adaptive" if not runs else "uniform", [])
        elif ln and not ln.startswith("#"):
            rows.append(dict(zip(keys, (float(x) if "." in x or "e" in x else int(x) for x in ln.split()))))
    out = {"exe": exe, "args": list(args), **runs}
    for k, rows in runs.items():  # the error per dof at the last step, and the mean dof count
        out[f"{k}_mean_dofs"] = round(statistics.mean(r["dofs"] for r in rows), 1)
        out[f"{k}_last_l2_error"] = rows[-1]["l2_error"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-ref", type=int, default=6)
    ap.add_argument("--driver", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"pair": bench_pair(3, 4, args.n_ref, args.steps, args.rounds, args.warmup), "driver": []}
    print(json.dumps(out["pair"]), flush=True)
    if args.driver:
        for exe, start, n_steps in (("heat-amr-2d-p2", 4, 20), ("heat-amr-2d-p4", 3, 20), ("heat-amr-3d-p2", 3, 10)):
            out["driver"].append(driver_table(exe, start, n_steps, 0.1, 0.6, 0.05))
            print(json.dumps(out["driver"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
