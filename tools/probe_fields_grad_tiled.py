#!/usr/bin/env python3
"""What the tiled gradient of the cost-to-go field costs: ``ops.fields_backward_tiled`` per call (host clock around the blocking call,
median of the reps) with the rounds and tile visits it took, beside ``ops.cost_to_go_tiled`` without policy planes on the same inputs, on
  * 64 mazes of 128x128           -- also through the one-workgroup kernel (``ops.fields_backward``), the only size both take: equal bits,
  * 16 mazes of 512x512, 4 of 1024x1024                       (unit cost: cost map = obstacle map),
  * 16 maps of 512x512, 4 of 1024x1024 with U(0,1) costs and 30 % obstacles -- and the same maps with U(0.5,1.5) costs: a U(0,1) cost below
    half an ulp of the distance beside it is absorbed by the forward's addition, that map is a plateau (status 11) and its backward ends
    after the init launch, so the U(0,1) rows say how many maps that hit (``status_plateau``).
The upstream gradient is N(0,1).  One JSON line per workload.

Usage:  python tools/probe_fields_grad_tiled.py [--reps 5] [--out profiles/fields_grad_tiled.json] [--small] [--cache DIR]
(--cache keeps the generated mazes in DIR/*.npz, the files of tools/probe_fields_tiled.py)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from neural_astar import ops  # noqa: E402
from probe_fields import mazes, timed  # noqa: E402
from probe_fields_tiled import cached, random_maps  # noqa: E402


def shifted_maps(n, size, seed):
    cost, passable, goal = random_maps(n, size, seed)
    return cost + np.float32(0.5), passable, goal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a quarter of every batch and of every side (a rehearsal)")
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    work = (("maze128", mazes, 64, 128), ("maze512", mazes, 16, 512), ("maze1024", mazes, 4, 1024), ("rand512_u1", random_maps, 16, 512),
            ("rand1024_u1", random_maps, 4, 1024), ("rand512_u05", shifted_maps, 16, 512), ("rand1024_u05", shifted_maps, 4, 1024))
    if args.small:
        work = tuple((name, make, max(2, n // 4), max(96, size // 4)) for name, make, n, size in work)
    dev = torch.device("cuda:0")
    th, tw = ops.fields_tile()
    lines = []
    for name, make, n, size in work:
        cost, passable, gidx = cached(args.cache if make is mazes else None, name, make, n, size)   # (random maps are quick to draw)
        goal = np.zeros((n, size * size), np.float32)
        goal[np.arange(n), gidx] = 1
        c, p, g = (torch.from_numpy(a).to(dev).reshape(n, 1, size, size) for a in (cost, passable, goal))
        up = torch.randn((n, 1, size, size), generator=torch.Generator(device=dev).manual_seed(5), device=dev)
        tiles = -(-size // th) * -(-size // tw)
        (fo, f_rounds), t_fwd = timed(lambda: ops.cost_to_go_tiled(c, g, p, policies=False), args.reps)
        visits = torch.zeros((n,), dtype=torch.int32, device=dev)
        (grad, status, rounds), ts = timed(lambda: ops.fields_backward_tiled(fo.dists, g, p, up, visits_out=visits), args.reps)
        v = visits.cpu().numpy()
        live = torch.isfinite(fo.dists) & (g == 0)
        row = {"workload": name, "B": n, "H": size, "W": size, "reps": args.reps, "tile": [th, tw], "tiles_per_map": tiles,
               "backward_ms_median": float(np.median(ts)), "backward_ms_min": float(np.min(ts)), "backward_ms_max": float(np.max(ts)),
               "backward_rounds": rounds, "visits_total": int(v.sum()), "visits_max": int(v.max()),
               "active_share": float(v.sum() / max(1, rounds * tiles * n)),
               "forward_field_alone_ms_median": float(np.median(t_fwd)), "forward_rounds": f_rounds,
               "backward_over_forward": float(np.median(ts) / np.median(t_fwd)),
               "live_cells": int(live.sum()), "status_plateau": int((status == ops.FIELD_PLATEAU).sum()),
               "status_other_nonzero": int(((status != 0) & (status != ops.FIELD_PLATEAU)).sum()),
               "grad_finite": bool(torch.isfinite(grad).all()), "grad_nonzero_cells": int((grad != 0).sum())}
        if size * size <= ops.FIELDS_GRAD_MAX_CELLS:
            (ref, ref_st), t_one = timed(lambda: ops.fields_backward(fo.dists, g, p, up), args.reps)
            row.update(one_workgroup_ms_median=float(np.median(t_one)), one_workgroup_ms_min=float(np.min(t_one)),
                       equal_to_one_workgroup=bool(torch.equal(grad, ref) and torch.equal(status, ref_st)))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
