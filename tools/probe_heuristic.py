#!/usr/bin/env python3
"""What a caller-supplied heuristic costs: one search launch per configuration, timed with HIP events, for
  (a) the default kernels (no mask, built-in heuristic: the hand-scheduled streams at 32x32, the large-map kernel at 512x512),
  (b) the MASKED instantiations with the Moore-8 mask (nastar_forward_ex_masked: the compiled step, built-in heuristic) -- the yardstick,
  (c) the HEURISTIC instantiations (nastar_forward_ex_heuristic) fed the built-in heuristic as a tensor: the same search, hh read from LDS
      (13 B per cell: 11 instead of 16 maps of 32x32 resident per CU) / h0 read from HBM beside the cost.
Workloads: maze32 (4096 and 2048 mazes of 32x32: the smaller batch is resident either way, which separates the shorter step from the lost
residency) and 256 random maps of 512x512 (15 % obstacles, U(0,1) costs).  One JSON line per configuration: median, min and max of the reps.

Usage:  python tools/probe_heuristic.py [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neural_astar import ops  # noqa: E402
from probe_neighbor_mask import problems  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind, nmaps in (("maze32", 4096), ("maze32", 2048), ("rand512", 256)):
        cost, s, g, p = (x[:nmaps].contiguous() for x in problems(kind, dev))
        if kind == "maze32":
            p = cost  # (one tensor, as VanillaAstar hands it over)
        B, H, W = cost.shape
        h0 = ops.heuristic(g)
        ref = None
        for label, kw in (("default", {}), ("masked_moore8", {"neighbor_mask": ops.NEIGHBORS_MOORE8}), ("heuristic_builtin", {"heuristic": h0})):
            run = lambda: ops.search_nograd(cost, s, g, p, 0.5, W * W, **kw)  # noqa: E731
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
            h = out[0].cpu()
            same = None if ref is None else bool(torch.equal(ref, h))
            ref = h if ref is None else ref
            print(json.dumps({"workload": kind, "B": B, "H": H, "W": W, "config": label, "ms_median": float(np.median(ts)),
                              "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "maps_per_s": B / (float(np.median(ts)) * 1e-3),
                              "expansions": int(out[0].sum().item()), "unsolved": int((out[3] != 0).sum().item()),
                              "equal_to_default": same}), flush=True)


if __name__ == "__main__":
    main()
