#!/usr/bin/env python3
"""What the tiled cost-to-go field costs: ``ops.cost_to_go_tiled`` per call (host clock around the blocking call, median of the reps), with
the rounds and tile visits it took, on
  * 64 mazes of 128x128           -- also through the one-workgroup kernel (``ops.cost_to_go``), the only size both take,
  * 16 mazes of 512x512, 4 of 1024x1024                       (unit cost: cost map = obstacle map),
  * 16 maps of 512x512, 4 of 1024x1024 with U(0,1) costs and 30 % obstacles,
each for 1, 4, 8 and 16 round launches between two reads of the host (``launches_per_batch``; the library's choice is made from this table).
``visits / (rounds * tiles)`` is the share of the workgroups of a round launch that had something to do: what a compacted list of active
tiles would save.  One JSON line per (workload, launches_per_batch).

Usage:  python tools/probe_fields_tiled.py [--reps 5] [--out profiles/fields/probe_fields_tiled.jsonl] [--small] [--cache DIR]
(--cache keeps the generated mazes in DIR/*.npz: carving a 1024x1024 maze in Python takes a while)
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from neural_astar import ops  # noqa: E402
from probe_fields import mazes, timed  # noqa: E402


def random_maps(n, size, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = rng.random((n, size, size)) > 0.3
    goal = (rng.random((n, size * size)) * maps.reshape(n, -1)).argmax(1)
    return rng.random((n, size, size)).astype(np.float32), maps.astype(np.float32), goal


def cached(cache, name, make, n, size):
    path = os.path.join(cache, f"{name}_{n}x{size}.npz") if cache else None
    if path and os.path.exists(path):
        with np.load(path) as z:
            return z["cost"].astype(np.float32), z["passable"].astype(np.float32), z["goal"]
    cost, passable, goal = make(n, size, 17)
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez_compressed(path, cost=cost, passable=passable.astype(np.uint8), goal=goal)
    return cost, passable, goal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a quarter of every batch and of every side (a rehearsal)")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--generate-only", action="store_true", help="fill --cache and stop (needs no GPU)")
    args = ap.parse_args()
    work = (("maze128", mazes, 64, 128), ("maze512", mazes, 16, 512), ("maze1024", mazes, 4, 1024), ("rand512_u1", random_maps, 16, 512),
            ("rand1024_u1", random_maps, 4, 1024))
    if args.small:
        work = tuple((name, make, max(2, n // 4), max(96, size // 4)) for name, make, n, size in work)
    if args.generate_only:
        for name, make, n, size in work:
            cached(args.cache if make is mazes else None, name, make, n, size)
        return
    dev = torch.device("cuda:0")
    th, tw = ops.fields_tile()
    lines = []
    for name, make, n, size in work:
        cost, passable, gidx = cached(args.cache if make is mazes else None, name, make, n, size)   # (random maps are quick to draw)
        goal = np.zeros((n, size * size), np.float32)
        goal[np.arange(n), gidx] = 1
        c, p, g = (torch.from_numpy(a).to(dev).reshape(n, 1, size, size) for a in (cost, passable, goal))
        tiles = -(-size // th) * -(-size // tw)
        base = {"workload": name, "B": n, "H": size, "W": size, "reps": args.reps, "tile": [th, tw], "tiles_per_map": tiles}
        ref = None
        if size * size <= ops.FIELDS_MAX_CELLS:
            ref, t_one = timed(lambda: ops.cost_to_go(c, g, p), args.reps)
            base.update(one_workgroup_ms_median=float(np.median(t_one)), one_workgroup_ms_min=float(np.min(t_one)))
        first = None
        for k in (1, 4, 8, 16):
            visits = torch.zeros((n,), dtype=torch.int32, device=dev)
            (out, rounds), ts = timed(lambda: ops.cost_to_go_tiled(c, g, p, visits_out=visits, launches_per_batch=k), args.reps)
            _, ts_field = timed(lambda: ops.cost_to_go_tiled(c, g, p, policies=False, launches_per_batch=k), args.reps)
            v = visits.cpu().numpy()
            d = out.dists
            row = dict(base, launches_per_batch=k, ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)),
                       field_alone_ms_median=float(np.median(ts_field)), rounds=rounds, visits_total=int(v.sum()), visits_max=int(v.max()),
                       active_share=float(v.sum() / max(1, rounds * tiles * n)), largest_finite_distance=float(d[torch.isfinite(d)].max()),
                       status_nonzero=int((out.status != 0).sum()))
            if ref is not None:
                row["equal_to_one_workgroup"] = bool(torch.equal(out.dists, ref.dists) and torch.equal(out.policies, ref.policies))
            if first is None:
                first = out
            else:
                row["equal_to_first_k"] = bool(torch.equal(out.dists, first.dists) and torch.equal(out.policies, first.policies))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
