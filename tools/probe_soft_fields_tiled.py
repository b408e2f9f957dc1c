#!/usr/bin/env python3
"""What the TILED entropy-regularised cost-to-go field costs (include/nastar_soft_fields_tiled.h): the time of a whole call of
``nastar_soft_cost_to_go_tiled`` (without a tape and with one) and of ``nastar_soft_fields_backward_tiled``, for the sweeps per launch
1, 2, 4, .. S and the checkpoint spacings 1 (every plane) and ceil(sqrt(K)) (the Python default), on random maps (25 % obstacles, costs
U(0.1, 1), Moore-8, tau = 0.25): 4096 maps of 96x128 at a horizon of 64 -- the largest map of the one-workgroup kernel, which is run beside
it -- and 256 of 128x128, 16 of 512x512 and one of 1024x1024 at their default horizons 2 * (H + W).  The sibling of
tools/probe_soft_fields.py, with its method: each figure is the median / min / max of device events around ONE call, after warm-up.
At 96x128 the bits of the one-workgroup kernel are checked before anything is timed.  A probe, not a gate: there is no target.  Writes
one JSON line per workload.

Usage:  python tools/probe_soft_fields_tiled.py [--reps 10] [--out profiles/soft_fields/probe_tiled.jsonl] [--small]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "neural-astar_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neural_astar import _native, ops  # noqa: E402

MOORE8 = 0x1EF
TAU = 0.25


def event_ms(launch, reps, warmup=2):
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
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_fields", "probe_tiled.jsonl"))
    ap.add_argument("--small", action="store_true", help="a sixteenth of every batch and of every horizon (a rehearsal)")
    args = ap.parse_args()
    import soft_fields_oracle as SO
    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(dev)
    th, tw, S = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.nastar_soft_fields_tile(ctypes.addressof(th), ctypes.addressof(tw), ctypes.addressof(S))
    S = S.value
    sweeps = sorted({1, S} | {s for s in (2, 4, 8, 16) if s < S})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for H, W, B, K in ((96, 128, 4096, 64), (128, 128, 256, None), (512, 512, 16, None), (1024, 1024, 1, None)):
            K = 2 * (H + W) if K is None else K
            if args.small:
                B, K = max(1, B // 16), max(4, K // 16)
            cost, passable, goal = SO.random_maps(H * W, B, H, W)
            up = np.random.default_rng(1).standard_normal((B, H, W)).astype(np.float32)
            c, p, g, u = (torch.from_numpy(a).to(dev) for a in (cost, passable, goal, up))
            dist, grad = torch.empty_like(c), torch.empty_like(c)
            st = torch.zeros((B,), dtype=torch.int32, device=dev)
            spacings = {"every_plane": 1, "sqrt": math.isqrt(K - 1) + 1}
            ws = torch.empty((int(lib.nastar_soft_fields_tiled_workspace_bytes(B, H, W)),), dtype=torch.uint8, device=dev)
            tapes = {n: torch.empty((int(lib.nastar_soft_fields_tiled_tape_bytes(B, H, W, K, ck)),), dtype=torch.uint8, device=dev)
                     for n, ck in spacings.items()}
            bws = {n: torch.empty((int(lib.nastar_soft_fields_tiled_backward_workspace_bytes(B, H, W, K, ck)),), dtype=torch.uint8, device=dev)
                   for n, ck in spacings.items()}

            def forward(per_launch, spacing=None):
                tape = tapes[spacing] if spacing else None
                _native.check(lib.nastar_soft_cost_to_go_tiled_with_sweeps(
                    c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, TAU, K, dist.data_ptr(), None, st.data_ptr(),
                    tape.data_ptr() if spacing else None, tape.numel() if spacing else 0, spacings[spacing] if spacing else 1, ws.data_ptr(), ws.numel(),
                    per_launch, stream), "nastar_soft_cost_to_go_tiled_with_sweeps")

            def backward(spacing):
                _native.check(lib.nastar_soft_fields_backward_tiled(
                    c.data_ptr(), g.data_ptr(), p.data_ptr(), tapes[spacing].data_ptr(), tapes[spacing].numel(), spacings[spacing], u.data_ptr(), B, H, W,
                    MOORE8, TAU, K, grad.data_ptr(), st.data_ptr(), bws[spacing].data_ptr(), bws[spacing].numel(), stream),
                    "nastar_soft_fields_backward_tiled")

            row = {"workload": f"rand{H}x{W}", "B": B, "H": H, "W": W, "horizon": K, "tau": TAU, "neighbor_mask": MOORE8, "reps": args.reps,
                   "tile": [th.value, tw.value], "sweeps_per_launch_shipped": S, "checkpoint_every": spacings,
                   "tape_bytes": {n: t.numel() for n, t in tapes.items()}, "backward_workspace_bytes": {n: t.numel() for n, t in bws.items()}}
            one_wg = H * W <= ops.SOFT_FIELDS_MAX_CELLS
            if one_wg:
                ref = torch.empty_like(c)

                def one_workgroup():
                    _native.check(lib.nastar_soft_cost_to_go(c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, TAU, K, ref.data_ptr(), None,
                                                             st.data_ptr(), None, 0, stream), "nastar_soft_cost_to_go")
                one_workgroup()
                forward(S)
                torch.cuda.synchronize()
                assert torch.equal(ref.view(torch.int32), dist.view(torch.int32)), "the tiled field is not the one-workgroup kernel's bits"
                row["one_workgroup_forward_ms"] = event_ms(one_workgroup, args.reps)
            for s in sweeps:
                row[f"forward_s{s}_ms"] = event_ms(lambda: forward(s), args.reps)
            for n in spacings:
                for s in (1, S):
                    row[f"forward_tape_{n}_s{s}_ms"] = event_ms(lambda: forward(s, n), args.reps)
                forward(S, n)
                row[f"backward_{n}_ms"] = event_ms(lambda: backward(n), args.reps)
            best = min(sweeps, key=lambda s: row[f"forward_s{s}_ms"]["median"])
            row["forward_fastest_sweeps_per_launch"] = best
            row["forward_us_per_sweep"] = row[f"forward_s{S}_ms"]["median"] * 1e3 / K
            row["backward_every_plane_us_per_step"] = row["backward_every_plane_ms"]["median"] * 1e3 / K
            row["backward_sqrt_over_every_plane"] = row["backward_sqrt_ms"]["median"] / row["backward_every_plane_ms"]["median"]
            if one_wg:
                row["tiled_over_one_workgroup"] = row[f"forward_s{S}_ms"]["median"] / row["one_workgroup_forward_ms"]["median"]
            row.update(device=torch.cuda.get_device_name(dev), compute_units=props.multi_processor_count,
                       timing="device events around one call (all its launches), after 2 warm-up calls")
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
            del tapes, bws, ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
