#!/usr/bin/env python3
"""What ordered routes cost: ``plan_routes()`` against ``forward()`` per call (host clock around a call that ends in a device synchronise,
both through the module, under no_grad), on
  * 4096 mazes of 32x32 (cost map = obstacle map: the hand-scheduled stream; routes [4096, 1024] int32 = 16 MiB more output per call),
  * 16 random maps of 512x512 (15 % obstacles, U(0,1) costs: the large-map kernel; the default capacity is H*W = 1 MiB per map, and
    ``max_route_len=4096`` for comparison).
One JSON line per configuration: median, min and max of the reps, and the equality of histories / paths with forward()'s.

Usage:  python tools/probe_routes.py [--reps 7]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neural_astar.planner.differentiable_astar import DifferentiableAstar  # noqa: E402
from probe_neighbor_mask import problems  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = DifferentiableAstar(0.5, 1.0).to(dev).eval()
    for kind, nmaps, caps in (("maze32", 4096, (None,)), ("rand512", 16, (None, 4096))):
        cost, s, g, p = (x[:nmaps].unsqueeze(1).contiguous() for x in problems(kind, dev))
        if kind == "maze32":
            p = cost
        B, _, H, W = cost.shape
        with torch.no_grad():
            fwd, ts = timed(lambda: m(cost, s, g, p), args.reps)
            rows = [("forward", None, ts, None)]
            for cap in caps:
                out, ts = timed(lambda: m.plan_routes(cost, s, g, p, max_route_len=cap), args.reps)
                same = bool(torch.equal(out.histories, fwd.histories) and torch.equal(out.paths, fwd.paths))
                rows.append(("plan_routes", int(out.routes.shape[1]), ts, same))
                longest = int(out.route_lengths.max())
        for label, cap, ts, same in rows:
            print(json.dumps({"workload": kind, "B": B, "H": H, "W": W, "call": label, "route_cap": cap, "ms_median": float(np.median(ts)),
                              "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "longest_route": longest,
                              "equal_to_forward": same}), flush=True)


if __name__ == "__main__":
    main()
