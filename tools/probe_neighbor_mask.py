#!/usr/bin/env python3
"""What the neighbourhood mask costs: one search launch per configuration, timed with HIP events, for
  * the default kernels (Moore-8, no mask: the hand-scheduled streams at 32x32, the large-map kernel at 512x512),
  * the MASKED instantiations with the Moore-8 mask (nastar_forward_ex_masked: same search, compiled step loops),
  * the masked instantiations with the von Neumann mask.
Workloads: maze32 (4096 mazes of 32x32, the bench's) and 256 random maps of 512x512 (15 % obstacles, U(0,1) costs).  One JSON line per
configuration; maps a neighbourhood cannot solve are counted (`unsolved`), not searched again.

Usage:  python tools/probe_neighbor_mask.py [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))

from neural_astar import ops  # noqa: E402
from neural_astar.utils import synthetic as syn  # noqa: E402


def problems(kind, dev):
    if kind == "maze32":
        pr = syn.maze_maps(4096, 32, seed=1234)
        m, s, g = pr.map_designs, pr.start_maps, pr.goal_maps
        cost = m
    else:
        B, H = 256, 512
        rng = np.random.Generator(np.random.PCG64(5))
        m = (rng.random((B, 1, H, H)) > 0.15).astype(np.float32)  # far above the 4-connected percolation threshold: nearly every pair connects
        s = np.zeros_like(m)
        g = np.zeros_like(m)
        for b in range(B):
            cells = np.flatnonzero(m[b])
            si, gi = rng.choice(cells, 2, replace=False)
            s[b].flat[si] = 1
            g[b].flat[gi] = 1
        cost = syn.random_costs(B, H, H, seed=6)
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev)[:, 0].contiguous() for x in (cost, s, g, m)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind in ("maze32", "rand512"):
        cost, s, g, p = problems(kind, dev)
        B, H, W = cost.shape
        ref = None
        for label, mask in (("default", None), ("masked_moore8", ops.NEIGHBORS_MOORE8), ("masked_von_neumann", ops.NEIGHBORS_VON_NEUMANN)):
            run = lambda: ops.search_nograd(cost, s, g, p, 0.5, W * W, neighbor_mask=mask)  # noqa: E731
            out = run()  # warm-up (and the outputs)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            if mask in (None, ops.NEIGHBORS_MOORE8):
                h = out[0].cpu()
                same = None if ref is None else bool(torch.equal(ref, h))
                ref = h if ref is None else ref
            else:
                same = None
            print(json.dumps({"workload": kind, "B": B, "H": H, "W": W, "config": label, "ms_median": float(np.median(ts)),
                              "ms_min": float(np.min(ts)), "maps_per_s": B / (float(np.median(ts)) * 1e-3),
                              "expansions": int(out[0].sum().item()), "unsolved": int((out[3] != 0).sum().item()),
                              "equal_to_default": same}), flush=True)


if __name__ == "__main__":
    main()
