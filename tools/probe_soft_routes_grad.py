#!/usr/bin/env python3
"""What the score-function backward of the sampled routes costs (include/nastar_soft_routes_grad.h): time per call of
``nastar_soft_routes_backward`` -- its five launches: the scale, the histogram, the seed plane, the field's backward, the store -- next to
``nastar_soft_fields_backward`` ALONE on the same seed plane (the K-plane recursion the new call contains: the ratio of the two is what the
histogram and the three small launches add) and next to the walkers' call ``nastar_soft_routes`` that wrote the routes.  Random maps
(25 % obstacles, costs U(0.1, 1), Moore-8, tau = 0.25, the default horizon 2 (H + W)), S = 4 starts per map on passable cells, N samples
each, rows of horizon + 1 cells, standard normal weights.

The workloads are (B, H x W) = (64, 32x32), (16, 64x64), (4, 96x64) -- 6144 cells, the backward's limit -- with 16, 64 and 1024 walkers per
map.  Each figure is the median / min / max of device events around ONE call, after warm-up, the calls taken in turn inside every
repetition.  Before anything is timed two calls of the backward are compared bit for bit.  A probe, not a gate: there is no target.  Writes
one JSON line per workload.

Usage:  python tools/probe_soft_routes_grad.py [--reps 10] [--out profiles/soft_routes/probe_grad.jsonl] [--small]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neural_astar import _native  # noqa: E402
from probe_soft_routes import MOORE8, S, SEED, TAU, event_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_routes", "probe_grad.jsonl"))
    ap.add_argument("--small", action="store_true", help="a quarter of every batch (a rehearsal)")
    args = ap.parse_args()
    import soft_fields_oracle as SO
    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for B, H, W in ((64, 32, 32), (16, 64, 64), (4, 96, 64)):
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
            _native.check(lib.nastar_soft_cost_to_go(c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, TAU, K, dist.data_ptr(), None,
                                                     mst.data_ptr(), tape.data_ptr(), tape_bytes, stream), "nastar_soft_cost_to_go")
            ws_bytes = int(lib.nastar_soft_routes_grad_workspace_bytes(B, H, W))
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
            grad, field_grad = torch.empty_like(c), torch.empty_like(c)
            gst = torch.empty((B,), dtype=torch.int32, device=dev)
            for SN in (16, 64, 1024):
                N = SN // S
                routes = torch.empty((B, S, N, K + 1), dtype=torch.int32, device=dev)
                lens = torch.empty((B, S, N), dtype=torch.int32, device=dev)
                logp = torch.empty((B, S, N), dtype=torch.float32, device=dev)
                qst = torch.empty((B, S), dtype=torch.int32, device=dev)
                up = torch.from_numpy(np.random.default_rng(SN).standard_normal((B, S, N)).astype(np.float32)).to(dev)

                def walkers():
                    _native.check(lib.nastar_soft_routes(c.data_ptr(), g.data_ptr(), p.data_ptr(), tape.data_ptr(), tape_bytes, st.data_ptr(), B, S, N,
                                                         H, W, MOORE8, TAU, K, SEED, None, routes.data_ptr(), K + 1, lens.data_ptr(), None,
                                                         logp.data_ptr(), None, qst.data_ptr(), stream), "nastar_soft_routes")

                def backward():
                    _native.check(lib.nastar_soft_routes_backward(c.data_ptr(), g.data_ptr(), p.data_ptr(), tape.data_ptr(), tape_bytes, st.data_ptr(),
                                                                  routes.data_ptr(), K + 1, lens.data_ptr(), qst.data_ptr(), up.data_ptr(), B, S, N, H,
                                                                  W, MOORE8, TAU, K, grad.data_ptr(), gst.data_ptr(), ws.data_ptr(), ws_bytes, stream),
                                  "nastar_soft_routes_backward")

                walkers()
                backward()
                torch.cuda.synchronize()
                first = grad.clone()
                # the seed plane the call left in its workspace (behind the two int64 planes): what the field's backward alone is timed on
                seed = ws[16 * B * H * W:20 * B * H * W].view(torch.float32).clone()
                backward()
                torch.cuda.synchronize()
                assert torch.equal(first.view(torch.int32), grad.view(torch.int32)), (H, W, SN)

                def field_backward():
                    _native.check(lib.nastar_soft_fields_backward(c.data_ptr(), g.data_ptr(), p.data_ptr(), tape.data_ptr(), tape_bytes, seed.data_ptr(),
                                                                  B, H, W, MOORE8, TAU, K, field_grad.data_ptr(), gst.data_ptr(), stream),
                                  "nastar_soft_fields_backward")

                solved = int((qst == 0).sum())
                row = {"workload": f"rand{H}x{W}", "B": B, "H": H, "W": W, "horizon": K, "tau": TAU, "neighbor_mask": MOORE8, "starts_per_map": S,
                       "samples_per_start": N, "walkers_per_map": SN, "reps": args.reps, "queries_solved": solved, "queries": B * S,
                       "mean_route_cells": float(lens[lens > 0].float().mean()) if solved else 0.0,
                       "row_bytes": B * SN * (K + 1) * 4, "library": os.path.basename(_native.LIB_PATH)}
                for name, t in event_ms({"routes_backward": backward, "field_backward": field_backward, "walkers": walkers}, args.reps).items():
                    row[name + "_ms"] = t
                row["backward_over_field_backward"] = row["routes_backward_ms"]["median"] / row["field_backward_ms"]["median"]
                row.update(device=torch.cuda.get_device_name(dev), compute_units=props.multi_processor_count,
                           timing="device events around one call, after 2 warm-up calls, the calls in turn inside every repetition")
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
                f.flush()
            del tape
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
