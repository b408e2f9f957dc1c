#!/usr/bin/env python3
"""What the entropy-regularised cost-to-go field costs (include/nastar_soft_fields.h): time per launch and per sweep of
``nastar_soft_cost_to_go`` (without a tape, with a tape and, where asked, with the policy planes) and of ``nastar_soft_fields_backward``,
for B = 4096 random maps (25 % obstacles, costs U(0.1, 1), Moore-8, tau = 0.25) and a horizon of 64 at 32x32, 64x64 and the limits
(96x128 forward, 64x96 forward and backward), with the exact field ``nastar_cost_to_go_sweeps`` of the SAME maps beside it.  Each figure is
the median / min / max of device events around ONE launch, after warm-up.  Before anything is timed the first map of every workload is
checked against the numpy definition (tests/soft_fields_oracle.py).  A probe, not a gate: there is no target.  Writes one JSON line per
workload.

``cycles_per_wave_cell``: the launch's time x the NOMINAL clock (--clock-mhz, 2400: the real one is not read) x the SIMDs of the device /
the (cell, sweep) pairs a wavefront computed -- what one SIMD spends on 64 cells of one sweep, to be set beside the instruction count of
the sweep.

Usage:  python tools/probe_soft_fields.py [--reps 10] [--out profiles/soft_fields/probe.jsonl] [--small]
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

from neural_astar import _native, ops  # noqa: E402

MOORE8 = 0x1EF
TAU, HORIZON = 0.25, 64


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_fields", "probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="a sixteenth of every batch (a rehearsal)")
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="the clock the cycle figures are computed with (nominal: nothing here reads the real one)")
    args = ap.parse_args()
    import soft_fields_oracle as SO
    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(dev)
    simds, clock_hz = props.multi_processor_count * 4, args.clock_mhz * 1e6
    B, K = (256 if args.small else 4096), HORIZON
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for H, W, backward in ((32, 32, True), (64, 64, True), (64, 96, True), (96, 128, False)):
            cost, passable, goal = SO.random_maps(H * W, B, H, W)
            up = np.random.default_rng(1).standard_normal((B, H, W)).astype(np.float32)
            c, p, g, u = (torch.from_numpy(a).to(dev) for a in (cost, passable, goal, up))
            dist, grad, hard = torch.empty_like(c), torch.empty_like(c), torch.empty_like(c)
            pol = torch.empty((B, 8, H, W), dtype=torch.float32, device=dev)
            st, sw = (torch.zeros((B,), dtype=torch.int32, device=dev) for _ in range(2))
            tape_bytes = int(lib.nastar_soft_fields_tape_bytes(B, H, W, K)) if backward else 0
            tape = torch.empty((tape_bytes,), dtype=torch.uint8, device=dev) if backward else None

            def soft(with_tape=False, with_policy=False):
                _native.check(lib.nastar_soft_cost_to_go(c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, TAU, K, dist.data_ptr(),
                                                         pol.data_ptr() if with_policy else None, st.data_ptr(),
                                                         tape.data_ptr() if with_tape else None, tape_bytes if with_tape else 0, stream),
                              "nastar_soft_cost_to_go")

            def soft_backward():
                _native.check(lib.nastar_soft_fields_backward(c.data_ptr(), g.data_ptr(), p.data_ptr(), tape.data_ptr(), tape_bytes, u.data_ptr(), B, H, W,
                                                              MOORE8, TAU, K, grad.data_ptr(), st.data_ptr(), stream), "nastar_soft_fields_backward")

            def exact():
                _native.check(lib.nastar_cost_to_go_sweeps(c.data_ptr(), g.data_ptr(), p.data_ptr(), B, H, W, MOORE8, hard.data_ptr(), None, st.data_ptr(),
                                                           sw.data_ptr(), stream), "nastar_cost_to_go_sweeps")

            row = {"workload": f"rand{H}x{W}", "B": B, "H": H, "W": W, "horizon": K, "tau": TAU, "neighbor_mask": MOORE8, "reps": args.reps}
            soft(with_tape=backward, with_policy=True)
            torch.cuda.synchronize()
            ref = SO.soft_field(cost[0], goal[0], passable[0], TAU, K)
            row["forward_rel_err_map0"] = SO.rel_err(dist[0].cpu().numpy(), ref.dist)
            assert np.array_equal(np.isfinite(dist[0].cpu().numpy()), np.isfinite(ref.dist)) and row["forward_rel_err_map0"] <= SO.FWD_RTOL, row
            if backward:
                soft_backward()
                torch.cuda.synchronize()
                row["backward_rel_err_map0"] = SO.rel_err(grad[0].cpu().numpy(), SO.soft_field_grad(cost[0], goal[0], passable[0], up[0], TAU, K).grad)
                assert row["backward_rel_err_map0"] <= SO.BWD_RTOL, row
            pairs = B * H * W * K / 64.0  # (cell, sweep) pairs per lane of a wavefront, summed over the device
            timed = [("soft_forward", lambda: soft()), ("soft_forward_policy", lambda: soft(with_policy=True))]
            if backward:
                timed += [("soft_forward_tape", lambda: soft(with_tape=True)), ("soft_backward", soft_backward)]
            for name, launch in timed:
                t = event_ms(launch, args.reps)
                row[name + "_ms"] = t
                row[name + "_us_per_sweep"] = t["median"] * 1e3 / K
                row[name + "_cycles_per_wave_cell"] = t["median"] * 1e-3 * clock_hz * simds / pairs
            row["exact_field_ms"] = event_ms(exact, args.reps)
            swn = sw.cpu().numpy()
            row["exact_field_sweeps_median"], row["exact_field_sweeps_max"] = float(np.median(swn)), int(swn.max())
            row["exact_field_us_per_sweep"] = row["exact_field_ms"]["median"] * 1e3 / max(1, int(swn.max()))
            row.update(device=torch.cuda.get_device_name(dev), compute_units=props.multi_processor_count, nominal_clock_mhz=args.clock_mhz,
                       timing="device events around one launch, after 2 warm-up launches", tape_bytes=tape_bytes)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
            del tape, pol
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
