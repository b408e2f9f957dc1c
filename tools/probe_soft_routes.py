#!/usr/bin/env python3
"""What sampling routes from the soft field costs (include/nastar_soft_routes.h): time per call and per move of ``nastar_soft_routes`` in
its two kernel shapes -- the tape streamed through LDS, and gathers from the tape -- and in the library's own choice, next to the forward
``nastar_soft_cost_to_go`` that wrote the tape of the SAME maps (the sampler reads the tape once, as the backward does: the forward is its
yardstick).  Random maps (25 % obstacles, costs U(0.1, 1), Moore-8, tau = 0.25, the default horizon 2 (H + W)), S = 4 starts per map on
passable cells, N samples each, rows of horizon + 1 cells, costs, log-probabilities and visit counts all asked for.

The workloads are (B, H x W, S * N) = (64, 32x32, 256), (16, 64x64, 1024), (4, 96x128, 4096), and the same maps with 16 and 64 walkers per
map: where the two shapes cross.  Each figure is the median / min / max of device events around ONE call (the launch that clears the rows and counts, and the walkers'), after
warm-up, the shapes taken in turn inside every repetition.  ``moves``: the moves of the longest route of the call, which is how many planes
a streaming workgroup reads; ``us_per_move`` = median / moves.  Before anything is timed the shapes' outputs are compared bit for bit.  A
probe, not a gate: there is no target.  Writes one JSON line per workload.

Usage:  python tools/probe_soft_routes.py [--reps 10] [--out profiles/soft_routes/probe.jsonl] [--small]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neural_astar import _native  # noqa: E402

MOORE8 = 0x1EF
TAU, S, SEED = 0.25, 4, 2026
SHAPES = {"auto": 0, "lds": 1, "gather": 2}


def event_ms(launches, reps, warmup=2):
    """{name: {"median", "min", "max"}} of the named launches, taken in turn inside every repetition"""
    for _ in range(warmup):
        for launch in launches.values():
            launch()
    torch.cuda.synchronize()
    ts = {name: [] for name in launches}
    for _ in range(reps):
        for name, launch in launches.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))} for name, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_routes", "probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="a quarter of every batch and of every walker count (a rehearsal)")
    args = ap.parse_args()
    import soft_fields_oracle as SO
    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for B, H, W, walkers in ((64, 32, 32, 256), (16, 64, 64, 1024), (4, 96, 128, 4096)):
            if args.small:
                B = max(1, B // 4)
            K = 2 * (H + W)
            cost, passable, goal = SO.random_maps(H * W, B, H, W)
            rng = np.random.default_rng(3)
            starts = np.stack([rng.choice(np.flatnonzero(passable[b].reshape(-1) != 0), S) for b in range(B)]).astype(np.int32)
            c, p, g = (torch.from_numpy(a).to(dev) for a in (cost, passable, goal))
            st = torch.from_numpy(starts).to(dev)
            dist = torch.empty_like(c)
            mst = torch.zeros((B,), dtype=torch.int32, device=dev)
            tape_bytes = int(lib.nastar_soft_fields_tape_bytes(B, H, W, K))
            tape = torch.empty((tape_bytes,), dtype=torch.uint8, device=dev)

            def forward(with_tape=True):
                _native.check(lib.nastar_soft_cost_to_go(c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, TAU, K, dist.data_ptr(), None,
                                                         mst.data_ptr(), tape.data_ptr() if with_tape else None, tape_bytes if with_tape else 0,
                                                         stream), "nastar_soft_cost_to_go")

            forward()
            for SN in (16, 64, walkers // 4 if args.small else walkers):
                N = SN // S
                routes = torch.empty((B, S, N, K + 1), dtype=torch.int32, device=dev)
                lens = torch.empty((B, S, N), dtype=torch.int32, device=dev)
                costs, logp = (torch.empty((B, S, N), dtype=torch.float32, device=dev) for _ in range(2))
                visits = torch.empty((B, S, H, W), dtype=torch.int32, device=dev)
                qst = torch.empty((B, S), dtype=torch.int32, device=dev)

                def sample(shape):
                    _native.check(lib.nastar_soft_routes_with_shape(
                        c.data_ptr(), g.data_ptr(), p.data_ptr(), tape.data_ptr(), tape_bytes, st.data_ptr(), B, S, N, H, W, MOORE8, TAU, K, SEED,
                        None, routes.data_ptr(), K + 1, lens.data_ptr(), costs.data_ptr(), logp.data_ptr(), visits.data_ptr(), qst.data_ptr(),
                        SHAPES[shape], stream), "nastar_soft_routes_with_shape")

                got = {}
                for shape in SHAPES:
                    sample(shape)
                    torch.cuda.synchronize()
                    got[shape] = [x.clone() for x in (routes, lens, costs, logp, visits, qst)]
                for shape in ("lds", "gather"):
                    assert all(torch.equal(x, y) for x, y in zip(got[shape], got["auto"])), (H, W, SN, shape)
                solved = int((qst == 0).sum())
                moves = int(lens.max()) - 1
                row = {"workload": f"rand{H}x{W}", "B": B, "H": H, "W": W, "horizon": K, "tau": TAU, "neighbor_mask": MOORE8, "starts_per_map": S,
                       "samples_per_start": N, "walkers_per_map": SN, "reps": args.reps, "queries_solved": solved, "queries": B * S,
                       "moves": moves, "mean_route_cells": float(lens[lens > 0].float().mean()) if solved else 0.0, "tape_bytes": tape_bytes}
                launches = {shape: (lambda shape=shape: sample(shape)) for shape in SHAPES}
                launches["forward_tape"] = forward
                launches["forward"] = lambda: forward(False)
                for name, t in event_ms(launches, args.reps).items():
                    row[name + "_ms"] = t
                    if name in SHAPES:
                        row[name + "_us_per_move"] = t["median"] * 1e3 / max(1, moves)
                    else:
                        row[name + "_us_per_sweep"] = t["median"] * 1e3 / K
                row.update(device=torch.cuda.get_device_name(dev), compute_units=props.multi_processor_count,
                           timing="device events around one call, after 2 warm-up calls, the shapes in turn inside every repetition")
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
                f.flush()
            del tape
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
