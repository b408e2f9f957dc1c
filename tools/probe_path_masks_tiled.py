#!/usr/bin/env python3
"""What the exact shortest path as a layer costs above 16384 cells (``ops.shortest_paths_tiled``: include/nastar_path_masks_tiled.h, the
tiled relaxation and one more launch; its blackbox backward, the same twice and an elementwise launch) beside the Python composition the
tree offered before, on the same tree:
  forward    ``ops.cost_to_go_tiled`` (no policies) + ``ops.field_routes`` + a torch scatter of the route cells
             -- ``rows=longest``: max_route_len=None (a lengths-only call, a host read, the call that fills the rows);
             -- ``rows=HW``: max_route_len=H*W, no host read in field_routes, rows of H*W entries;
  backward   the torch perturbation ``clamp(lambda * g + cost, min_cost)``, the composed forward again, ``(y_lambda - y) / lambda``.
Workloads: 64 mazes of 128x128 (the one size both layers take: the one-launch ``ops.shortest_paths`` is timed beside them), 16 random
maps of 512x512 and 2 of 1024x1024 (25 % obstacles, the start the reachable cell farthest from the goal), costs U(0.25, 1.25); the
upstream gradient is ``1 - 2 target`` with the optimal path under other seeded costs as the target, lambda = 20, min_cost = 2^-10.  Both
sides run the SAME relaxation, timed alone as ``field_alone_ms``: expect a small difference.  Everything is timed by the wall clock around
the call and a device synchronisation, median / min / max of the reps after two warm-up calls.  Masks and gradients are asserted equal on
both sides before anything is timed.  No pass threshold.  Writes one JSON document.

Usage:  python tools/probe_path_masks_tiled.py [--reps 5] [--out profiles/path_masks_tiled.json] [--small]
"""
import argparse
import datetime
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

LAMBDA, MIN_COST = 20.0, 2.0 ** -10


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def wall_ms(call, reps, warmup=2):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def composed(cost, idx, goal, passable, cap):
    """cost_to_go_tiled + field_routes + scatter -> the [B,1,H,W] mask"""
    B, _, H, W = cost.shape
    field, _ = ops.cost_to_go_tiled(cost, goal, passable, policies=False)
    r = ops.field_routes(field.dists, goal, passable, idx[:, None], max_route_len=cap)
    cell = torch.where(r.routes < 0, H * W, r.routes).long()[:, 0]
    return torch.zeros((B, H * W + 1), device=cost.device).scatter_(1, cell, 1.0)[:, :H * W].reshape(B, 1, H, W)


def random_maps(B, H, W, rng, dev):
    """passable (25 % obstacles), goal (one passable cell), [B] int32 starts: the reachable cell farthest from the goal under unit costs"""
    passable = (rng.random((B, 1, H, W)) > 0.25).astype(np.float32)
    goal = np.zeros_like(passable)
    for b in range(B):
        r, c = int(rng.integers(H)), int(rng.integers(W))
        passable[b, 0, r, c] = goal[b, 0, r, c] = 1
    passable, goal = torch.from_numpy(passable).to(dev), torch.from_numpy(goal).to(dev)
    d = ops.cost_to_go_tiled(passable, goal, passable, policies=False)[0].dists.reshape(B, -1)
    return passable, goal, torch.where(torch.isfinite(d), d, torch.full_like(d, -1.0)).argmax(1).to(torch.int32)


def workload(name, passable, goal, idx, reps, dev, rng):
    B, _, H, W = passable.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    cost = t(0.25 + rng.random((B, 1, H, W)))
    target = ops.shortest_paths_tiled(t(0.25 + rng.random((B, 1, H, W))), idx, goal, passable).paths
    up = 1 - 2 * target

    def layer_both(layer):
        c = cost.clone().requires_grad_(True)
        out = layer(c, idx, goal, passable, lambda_=LAMBDA, min_cost=MIN_COST)
        out.paths.backward(up)
        return out.paths.detach(), c.grad

    def composed_both(cap):
        y = composed(cost, idx, goal, passable, cap)
        y_lam = composed(torch.clamp(LAMBDA * up + cost, min=MIN_COST), idx, goal, passable, cap)
        return y, (y_lam - y) * (1.0 / LAMBDA)

    out = ops.shortest_paths_tiled(cost, idx, goal, passable)
    y, grad = layer_both(ops.shortest_paths_tiled)
    y_ref, grad_ref = composed_both(H * W)
    torch.cuda.synchronize()
    assert torch.equal(out.paths, y) and torch.equal(y, y_ref) and torch.equal(y, composed(cost, idx, goal, passable, None)), f"{name}: the masks differ"
    assert torch.equal(grad, grad_ref), f"{name}: the gradients differ"
    row = {"workload": name, "B": B, "H": H, "W": W, "reps": reps, "maps_solved": int((out.status == 0).sum()),
           "longest_path": int(out.paths.sum((1, 2, 3)).max()), "maps_whose_path_moved": int((grad != 0).flatten(1).any(1).sum()),
           "masks_and_gradients_equal_to_composed": True,
           "field_alone_ms": wall_ms(lambda: ops.cost_to_go_tiled(cost, goal, passable, policies=False), reps),
           "tiled_forward_ms": wall_ms(lambda: ops.shortest_paths_tiled(cost, idx, goal, passable), reps),
           "tiled_forward_backward_ms": wall_ms(lambda: layer_both(ops.shortest_paths_tiled), reps)}
    for tag, cap in (("longest", None), ("HW", H * W)):
        row[f"composed_forward_rows_{tag}_ms"] = wall_ms(lambda: composed(cost, idx, goal, passable, cap), reps)
        row[f"composed_forward_backward_rows_{tag}_ms"] = wall_ms(lambda: composed_both(cap), reps)
    if H * W <= ops.PATH_MASKS_MAX_CELLS:
        one, one_grad = layer_both(ops.shortest_paths)
        assert torch.equal(one, y) and torch.equal(one_grad, grad), f"{name}: the one-launch call differs"
        row["one_launch_forward_ms"] = wall_ms(lambda: ops.shortest_paths(cost, idx, goal, passable), reps)
        row["one_launch_forward_backward_ms"] = wall_ms(lambda: layer_both(ops.shortest_paths), reps)
    best = min(row["composed_forward_rows_longest_ms"]["median"], row["composed_forward_rows_HW_ms"]["median"])
    best_both = min(row["composed_forward_backward_rows_longest_ms"]["median"], row["composed_forward_backward_rows_HW_ms"]["median"])
    row["forward_speedup_median"] = best / row["tiled_forward_ms"]["median"]
    row["forward_backward_speedup_median"] = best_both / row["tiled_forward_backward_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a quarter of every batch and of every large map's side (a rehearsal)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(43))
    n128, n512, side512, side1024 = (16, 4, 256, 512) if args.small else (64, 16, 512, 1024)
    P = syn.maze_maps(n128, 128, seed=13)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    maze_start = t(P.start_maps)
    jobs = [("maze128", (t(P.map_designs), t(P.goal_maps), ops._start_indices(maze_start, n128, 128, 128).reshape(n128).contiguous())),
            (f"rand{side512}", random_maps(n512, side512, side512, rng, dev)), (f"rand{side1024}", random_maps(2, side1024, side1024, rng, dev))]
    rows = []
    for name, (passable, goal, idx) in jobs:
        rows.append(workload(name, passable, goal, idx, args.reps, dev, rng))
        print(json.dumps(rows[-1]), flush=True)
    doc = {"probe": "tools/probe_path_masks_tiled.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(dev),
           "timing": "wall clock around the call and a device synchronisation, after 2 warm-up calls",
           "lambda": LAMBDA, "min_cost": MIN_COST, "small": bool(args.small), "workloads": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
