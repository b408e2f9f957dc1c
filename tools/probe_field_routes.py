#!/usr/bin/env python3
"""What ordered routes for many starts per map cost when they are read off the field (``ops.cost_to_go`` / ``cost_to_go_tiled`` once per map,
then ``ops.field_routes``: include/nastar_field_routes.h) beside the only way the tree offered before: ``plan_routes`` on the S-fold
replicated maps, one search per start.  Workloads:
  * 16 mazes of 32x32, S in {1, 64, 1024} starts per map    (unit cost, Moore-8; the table in LDS),
  * one random map of 512x512 (25 % obstacles), S = 1024     (unit cost, Moore-8; the table in the workspace).
Both sides are timed by the wall clock around the call and a device synchronisation (``plan_routes`` and the tiled field read the host
back, so device events would not see all of it), after warm-up, median / min / max of the reps; the routes' rows hold H*W entries on both
sides.  The two answers are compared before anything is timed: on every query both solve, the field's route is never the longer one (the
search's heuristic carries a tie-breaking term and may return a longer route; the count is recorded).  No pass threshold.

THE STEP of the chase, on each table path: a one-cell serpentine corridor (4-connected, unit cost, the field written by hand), 64 starts
-- one wavefront -- at its far end against 64 starts on the goal, lengths-only calls timed by device events; the difference divided by the
number of steps is the time of one dependent step (one byte read and a few integer instructions).  128x128 (LDS) and
512x512 (workspace).  Writes one JSON document.

Usage:  python tools/probe_field_routes.py [--reps 10] [--out profiles/field_routes.json] [--small]
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

from neural_astar import _native, ops  # noqa: E402
from neural_astar.planner import VanillaAstar  # noqa: E402
from neural_astar.utils import synthetic as syn  # noqa: E402

VON_NEUMANN = 0x0AA


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


def event_ms(launch, reps, warmup=3):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return stats(ts)


def compare(name, planner, maps, goals, S, reps, dev, rng):
    """field + field_routes against plan_routes on the S-fold replicated maps -> a row of the document"""
    B, _, H, W = maps.shape
    free = [np.flatnonzero((maps[b, 0] != 0).reshape(-1).cpu().numpy()) for b in range(B)]
    starts = torch.from_numpy(np.stack([rng.choice(f, S) for f in free]).astype(np.int32)).to(dev)
    tiled = H * W > ops.FIELDS_MAX_CELLS

    def by_field():
        return planner.plan_many(maps, starts, goals, max_route_len=H * W)

    rep_maps = maps.repeat_interleave(S, 0)
    rep_goals = goals.repeat_interleave(S, 0)
    rep_starts = torch.zeros((B * S, 1, H * W), device=dev)
    rep_starts.scatter_(2, starts.reshape(B * S, 1, 1).long(), 1.0)
    rep_starts = rep_starts.reshape(B * S, 1, H, W)

    def by_search():
        return planner.plan_routes(rep_maps, rep_starts, rep_goals, max_route_len=H * W)

    f, s = by_field(), by_search()
    torch.cuda.synchronize()
    both = (f.status.reshape(-1) == 0) & (s.route_lengths > 0)
    fl, sl = f.route_lengths.reshape(-1)[both], s.route_lengths[both]
    assert bool(both.any()) and bool((fl <= sl).all()), f"{name}: a search found a shorter route than the field's"
    t_field = wall_ms(lambda: ops.cost_to_go(maps, goals, maps, policies=False, tiled=tiled), reps)
    t_routes = wall_ms(lambda: ops.field_routes(f.dists, goals, maps, starts, max_route_len=H * W), reps)
    t_both, t_search = wall_ms(by_field, reps), wall_ms(by_search, reps)
    return {"workload": name, "B": B, "S": S, "H": H, "W": W, "reps": reps, "table": "lds" if H * W <= _native.load().nastar_field_routes_lds_cells() else "workspace",
            "queries_solved": int(both.sum()), "longest_route": int(f.route_lengths.max()), "search_routes_longer": int((sl > fl).sum()),
            "field_ms": t_field, "field_routes_ms": t_routes, "plan_many_ms": t_both, "plan_routes_replicated_ms": t_search,
            "speedup_median": t_search["median"] / t_both["median"]}


def corridor(size, dev):
    """a one-cell serpentine of size x size (every other row open, joined at alternating ends), the goal at (0, 0), its field by hand"""
    order = []
    for k, r in enumerate(range(0, size, 2)):
        cols = range(size) if k % 2 == 0 else range(size - 1, -1, -1)
        order += [r * size + c for c in cols]
        if r + 2 < size:
            order.append((r + 1) * size + (size - 1 if k % 2 == 0 else 0))
    order = np.array(order)
    passable = np.zeros(size * size, np.float32)
    passable[order] = 1
    dist = np.full(size * size, np.inf, np.float32)
    dist[order] = np.arange(len(order), dtype=np.float32)
    goal = np.zeros(size * size, np.float32)
    goal[order[0]] = 1
    t = lambda a: torch.from_numpy(a).to(dev).reshape(1, 1, size, size)  # noqa: E731
    return t(dist), t(goal), t(passable), int(order[-1]), len(order) - 1


def step(size, reps, dev):
    dist, goal, passable, far, steps = corridor(size, dev)
    lib = _native.load()
    S = 64
    lengths, status = (torch.empty((1, S), dtype=torch.int32, device=dev) for _ in range(2))
    nbytes = lib.nastar_field_routes_workspace_bytes(1, size, size)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for name, cell in (("far", far), ("goal", 0)):
        starts = torch.full((1, S), cell, dtype=torch.int32, device=dev)

        def launch():
            _native.check(lib.nastar_field_routes(dist.data_ptr(), goal.data_ptr(), passable.data_ptr(), starts.data_ptr(), 1, S, size, size, VON_NEUMANN,
                                                  None, 0, lengths.data_ptr(), None, status.data_ptr(), ws.data_ptr(), nbytes, stream), "nastar_field_routes")

        launch()
        torch.cuda.synchronize()
        assert not status.any() and lengths.unique().tolist() == [steps + 1 if name == "far" else 1]
        out[name] = event_ms(launch, reps)
    return {"corridor": f"{size}x{size}", "table": "workspace" if nbytes else "lds", "steps": steps, "wavefronts": 1, "far_ms": out["far"], "goal_ms": out["goal"],
            "ns_per_step": (out["far"]["median"] - out["goal"]["median"]) * 1e6 / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="S = 64 at most and a 256x256 corridor (a rehearsal)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(31))
    planner = VanillaAstar().to(dev).eval()
    planner.astar.check_solvable = False   # (a walled-in start among the queries is reported in the status, not raised)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    rows = []
    P = syn.maze_maps(16, 32, seed=3)
    for S in (1, 64) if args.small else (1, 64, 1024):
        rows.append(compare("maze32", planner, t(P.map_designs), t(P.goal_maps), S, args.reps, dev, rng))
        print(json.dumps(rows[-1]), flush=True)
    big = (rng.random((1, 1, 512, 512)) > 0.25).astype(np.float32)
    goal = np.zeros((1, 1, 512, 512), np.float32)
    big[0, 0, 256, 256] = goal[0, 0, 256, 256] = 1
    rows.append(compare("rand512", planner, t(big), t(goal), 64 if args.small else 1024, args.reps, dev, rng))
    print(json.dumps(rows[-1]), flush=True)
    steps = [step(128, args.reps, dev), step(256 if args.small else 512, args.reps, dev)]
    for s in steps:
        print(json.dumps(s), flush=True)
    doc = {"probe": "tools/probe_field_routes.py", "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(dev),
           "timing": "workloads: wall clock around the call and a device synchronisation, after 2 warm-up calls; step: device events around one launch",
           "small": bool(args.small), "field_routes_lds_cells": _native.load().nastar_field_routes_lds_cells(), "workloads": rows, "step": steps}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
