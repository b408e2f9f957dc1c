#!/usr/bin/env python3
"""What sampling routes from the TILED soft field's checkpointed tape costs (include/nastar_soft_routes_tiled.h): time per call of
``nastar_soft_routes_tiled`` from a given tape, next to the tiled forward ``nastar_soft_cost_to_go_tiled`` that wrote the tape of the SAME
maps (the call rebuilds every segment of the tape with the forward's sweeps: the forward is its yardstick) and, where the one-workgroup
kernels take the maps, next to ``nastar_soft_routes`` from the one-workgroup forward's full tape.  Random maps (25 % obstacles, costs
U(0.1, 1), Moore-8, tau = 0.25, the default horizon 2 (H + W)), S = 4 starts per map on passable cells, N samples each, rows of
horizon + 1 cells (no replay), costs, log-probabilities and visit counts all asked for.

The workloads are (B, H x W, S * N) = (a) (4, 96x128, 64), (b) (4, 512x512, 64), (c) (4, 512x512, 4096), (d) (1, 1024x1024, 64), with
``checkpoint_every`` = ceil(sqrt(horizon)), the default; (b) also with 1, where every plane is kept and nothing is rebuilt.  Each figure is
the median / min / max of device events around ONE call, after warm-up, the calls taken in turn inside every repetition.  A probe, not a
gate: there is no target.  Writes one JSON line per workload.

Usage:  python tools/probe_soft_routes_tiled.py [--reps 10] [--out profiles/soft_routes_tiled/probe.jsonl] [--small]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neural_astar import _native  # noqa: E402
from probe_soft_routes import event_ms  # noqa: E402

MOORE8 = 0x1EF
TAU, S, SEED = 0.25, 4, 2026
WORKLOADS = (("a", 4, 96, 128, 64, (None,)), ("b", 4, 512, 512, 64, (1, None)), ("c", 4, 512, 512, 4096, (None,)), ("d", 1, 1024, 1024, 64, (None,)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_routes_tiled", "probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="a quarter of every side and of every walker count (a rehearsal)")
    args = ap.parse_args()
    import soft_fields_oracle as SO
    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(dev)
    one_limit = lib.nastar_soft_routes_max_cells()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name, B, H, W, SN, spacings in WORKLOADS:
            if args.small:
                H, W, SN = H // 4, W // 4, max(S, SN // 4)
            K, N = 2 * (H + W), SN // S
            cost, passable, goal = SO.random_maps(H * W, B, H, W)
            rng = np.random.default_rng(3)
            starts = np.stack([rng.choice(np.flatnonzero(passable[b].reshape(-1) != 0), S) for b in range(B)]).astype(np.int32)
            c, p, g = (torch.from_numpy(a).to(dev) for a in (cost, passable, goal))
            st = torch.from_numpy(starts).to(dev)
            dist = torch.empty_like(c)
            mst = torch.zeros((B,), dtype=torch.int32, device=dev)
            routes = torch.empty((B, S, N, K + 1), dtype=torch.int32, device=dev)
            lens = torch.empty((B, S, N), dtype=torch.int32, device=dev)
            costs, logp = (torch.empty((B, S, N), dtype=torch.float32, device=dev) for _ in range(2))
            visits = torch.empty((B, S, H, W), dtype=torch.int32, device=dev)
            qst = torch.empty((B, S), dtype=torch.int32, device=dev)
            outs = (routes, lens, costs, logp, visits, qst)
            fws_bytes = int(lib.nastar_soft_fields_tiled_workspace_bytes(B, H, W))
            fws = torch.empty((fws_bytes,), dtype=torch.uint8, device=dev)
            ref = None
            for every in spacings:
                cev = max(1, math.isqrt(K - 1) + 1) if every is None else every
                tape_bytes = int(lib.nastar_soft_fields_tiled_tape_bytes(B, H, W, K, cev))
                tape = torch.empty((tape_bytes,), dtype=torch.uint8, device=dev)
                ws_bytes = int(lib.nastar_soft_routes_tiled_workspace_bytes(B, S, N, H, W, K, cev))
                ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)

                def forward(with_tape=True):
                    _native.check(lib.nastar_soft_cost_to_go_tiled(c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, TAU, K, dist.data_ptr(), None,
                                                                   mst.data_ptr(), tape.data_ptr() if with_tape else None,
                                                                   tape_bytes if with_tape else 0, cev, fws.data_ptr(), fws_bytes, stream),
                                  "nastar_soft_cost_to_go_tiled")

                def sample():
                    _native.check(lib.nastar_soft_routes_tiled(
                        c.data_ptr(), g.data_ptr(), p.data_ptr(), tape.data_ptr(), tape_bytes, cev, st.data_ptr(), B, S, N, H, W, MOORE8, TAU, K, SEED,
                        None, routes.data_ptr(), K + 1, lens.data_ptr(), costs.data_ptr(), logp.data_ptr(), visits.data_ptr(), qst.data_ptr(),
                        ws.data_ptr(), ws_bytes, stream), "nastar_soft_routes_tiled")

                forward()
                sample()
                torch.cuda.synchronize()
                got = [x.clone() for x in outs]
                if ref is not None:  # the spacing of the checkpoints does not change a bit
                    assert all(torch.equal(x, y) for x, y in zip(got, ref)), (name, every)
                ref = got
                launches = {"routes_tiled": sample, "forward_tiled_tape": forward, "forward_tiled": lambda: forward(False)}
                row = {"workload": name, "maps": f"rand{H}x{W}", "B": B, "H": H, "W": W, "horizon": K, "tau": TAU, "neighbor_mask": MOORE8,
                       "starts_per_map": S, "samples_per_start": N, "walkers_per_map": SN, "checkpoint_every": cev, "segments": -(-K // cev),
                       "reps": args.reps, "queries_solved": int((qst == 0).sum()), "queries": B * S, "moves": int(lens.max()) - 1,
                       "mean_route_cells": float(lens[lens > 0].float().mean()) if int((qst == 0).sum()) else 0.0, "tape_bytes": tape_bytes,
                       "workspace_bytes": ws_bytes}
                if H * W <= one_limit:  # the one-workgroup pair on the same maps: the same bits, from the full tape
                    full_bytes = int(lib.nastar_soft_fields_tape_bytes(B, H, W, K))
                    full = torch.empty((full_bytes,), dtype=torch.uint8, device=dev)

                    def forward_one():
                        _native.check(lib.nastar_soft_cost_to_go(c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, TAU, K, dist.data_ptr(), None,
                                                                 mst.data_ptr(), full.data_ptr(), full_bytes, stream), "nastar_soft_cost_to_go")

                    def sample_one():
                        _native.check(lib.nastar_soft_routes(
                            c.data_ptr(), g.data_ptr(), p.data_ptr(), full.data_ptr(), full_bytes, st.data_ptr(), B, S, N, H, W, MOORE8, TAU, K, SEED,
                            None, routes.data_ptr(), K + 1, lens.data_ptr(), costs.data_ptr(), logp.data_ptr(), visits.data_ptr(), qst.data_ptr(),
                            stream), "nastar_soft_routes")

                    forward_one()
                    sample_one()
                    torch.cuda.synchronize()
                    assert all(torch.equal(x, y) for x, y in zip(outs, ref)), name
                    row["full_tape_bytes"] = full_bytes
                    launches.update(routes_one_workgroup=sample_one, forward_one_workgroup_tape=forward_one)
                for what, t in event_ms(launches, args.reps).items():
                    row[what + "_ms"] = t
                row["routes_tiled_over_forward_tiled_tape"] = row["routes_tiled_ms"]["median"] / row["forward_tiled_tape_ms"]["median"]
                if "routes_one_workgroup_ms" in row:
                    row["routes_tiled_over_routes_one_workgroup"] = row["routes_tiled_ms"]["median"] / row["routes_one_workgroup_ms"]["median"]
                row.update(device=torch.cuda.get_device_name(dev), compute_units=props.multi_processor_count,
                           timing="device events around one call, after 2 warm-up calls, the calls in turn inside every repetition")
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
                f.flush()
                del tape, ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
