#!/usr/bin/env python3
"""What the cost-to-go field costs: ``ops.cost_to_go`` per call (host clock around a call that ends in a device synchronise -- the call reads
its status), the field alone and the field with policies, median of the reps, on
  * 4096 mazes of 32x32          (unit cost: cost map = obstacle map; one wavefront per map),
  * 1024 random maps of 64x64    (25 % obstacles, U(0,1) costs; four wavefronts per map),
  * 64 mazes of 128x128          (unit cost; sixteen wavefronts per map, the size limit),
with the sweeps the relaxation took on the device beside the time, and -- on the unit-cost cases -- the host path the package had before:
``synthetic.geodesic_distance`` + ``synthetic.optimal_policies`` (numpy, timed once: it is slow), whose results the kernel's must equal.
One JSON line per workload.

Usage:  python tools/probe_fields.py [--reps 5] [--out profiles/fields/probe_fields.jsonl] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))

from neural_astar import ops  # noqa: E402
from neural_astar.utils import synthetic as syn  # noqa: E402


def mazes(n, size, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = np.stack([syn._carve_maze(rng, size, 0.1) for _ in range(n)])
    goal = (rng.random((n, size * size)) * maps.reshape(n, -1)).argmax(1)
    return maps.astype(np.float32), maps.astype(np.float32), goal


def random_maps(n, size, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = rng.random((n, size, size)) > 0.25
    goal = (rng.random((n, size * size)) * maps.reshape(n, -1)).argmax(1)
    return rng.random((n, size, size)).astype(np.float32), maps.astype(np.float32), goal


def timed(fn, reps):
    out = fn()  # warm-up (and the outputs)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a sixteenth of every batch (a rehearsal)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for name, make, n, size, unit in (("maze32", mazes, 4096, 32, True), ("rand64_u1", random_maps, 1024, 64, False), ("maze128", mazes, 64, 128, True)):
        n = max(4, n // 16) if args.small else n
        cost, passable, gidx = make(n, size, 17)
        goal = np.zeros((n, size * size), np.float32)
        goal[np.arange(n), gidx] = 1
        c, p, g = (torch.from_numpy(a).to(dev).reshape(n, 1, size, size) for a in (cost, passable, goal))
        sweeps = torch.zeros((n,), dtype=torch.int32, device=dev)
        _, t_field = timed(lambda: ops.cost_to_go(c, g, p, policies=False), args.reps)
        out, t_both = timed(lambda: ops.cost_to_go(c, g, p, policies=True, sweeps_out=sweeps), args.reps)
        sw = sweeps.cpu().numpy()
        d = out.dists[:, 0].cpu().numpy()
        row = {"workload": name, "B": n, "H": size, "W": size, "reps": args.reps,
               "field_ms_median": float(np.median(t_field)), "field_ms_min": float(np.min(t_field)), "field_ms_max": float(np.max(t_field)),
               "field_policy_ms_median": float(np.median(t_both)), "field_policy_ms_min": float(np.min(t_both)),
               "field_policy_ms_max": float(np.max(t_both)), "sweeps_median": float(np.median(sw)), "sweeps_max": int(sw.max()),
               "largest_finite_distance": float(d[np.isfinite(d)].max()), "status_nonzero": int((out.status != 0).sum())}
        if unit:
            t0 = time.perf_counter()
            bfs = syn.geodesic_distance(passable > 0, gidx)
            t1 = time.perf_counter()
            pol = syn.optimal_policies(passable > 0, bfs)
            t2 = time.perf_counter()
            row.update(host_geodesic_ms=(t1 - t0) * 1e3, host_policies_ms=(t2 - t1) * 1e3,
                       equal_to_host=bool(np.array_equal(d, np.where(bfs >= 0, bfs.astype(np.float32), np.float32(np.inf)))
                                          and np.array_equal(out.policies.cpu().numpy(), pol[:, :, 0])))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
