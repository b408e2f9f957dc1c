#!/usr/bin/env python3
"""What the gradient of the cost-to-go field costs beside the field itself: the forward launch (``nastar_cost_to_go_sweeps``, field alone)
and the backward launch (``nastar_fields_backward``), each timed by device events around ONE launch, after warm-up, median / min / max of
the reps, with the sweeps both loops took on the device, on
  * 4096 mazes of 32x32            (U(0.5, 1.5) costs, Moore-8; one wavefront per map),
  * 64 random maps of 128x128      (25 % obstacles, U(0.5, 1.5) costs, Moore-8; sixteen wavefronts per map, the size limit),
  * 64 serpentines of 128x128      (a one-cell corridor of 8256 cells, unit cost, 4-connected: the highest forest a map of that size has).
The upstream gradient is N(0, 1).  The backward's result is checked against the numpy definition on the first map of each workload
(tests/fields_grad_oracle.py) before anything is timed.  Writes one JSON document.

Usage:  python tools/probe_fields_grad.py [--reps 20] [--out profiles/fields_grad.json] [--small]
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
from neural_astar.utils import synthetic as syn  # noqa: E402

MOORE8, VON_NEUMANN = 0x1EF, 0x0AA


def mazes(n, size, rng):
    maps = np.stack([syn._carve_maze(rng, size, 0.1) for _ in range(n)]).astype(np.float32)
    return (0.5 + rng.random((n, size, size))).astype(np.float32), maps, (rng.random((n, size * size)) * maps.reshape(n, -1)).argmax(1), MOORE8


def random_maps(n, size, rng):
    maps = (rng.random((n, size, size)) > 0.25).astype(np.float32)
    return (0.5 + rng.random((n, size, size))).astype(np.float32), maps, (rng.random((n, size * size)) * maps.reshape(n, -1)).argmax(1), MOORE8


def serpentines(n, size, rng):
    one = np.zeros((size, size), np.float32)
    one[0::2] = 1
    one[1::4, size - 1] = 1
    one[3::4, 0] = 1
    maps = np.stack([one if b % 2 == 0 else one[::-1] for b in range(n)])  # the chain runs down every other map and up the rest
    return maps.copy(), maps, np.array([0 if b % 2 == 0 else (size - 1) * size for b in range(n)]), VON_NEUMANN


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
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a sixteenth of every batch (a rehearsal)")
    args = ap.parse_args()
    import fields_grad_oracle as GO
    dev = torch.device("cuda:0")
    lib = _native.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    for name, make, n, size in (("maze32", mazes, 4096, 32), ("rand128", random_maps, 64, 128), ("serpentine128", serpentines, 64, 128)):
        n = max(4, n // 16) if args.small else n
        rng = np.random.Generator(np.random.PCG64(23))
        cost, passable, gidx, mask = make(n, size, rng)
        goal = np.zeros((n, size * size), np.float32)
        goal[np.arange(n), gidx] = 1
        up = rng.standard_normal((n, size, size)).astype(np.float32)
        c, p, g, u = (torch.from_numpy(a).to(dev).reshape(n, size, size).contiguous() for a in (cost, passable, goal, up))
        dist, grad = torch.empty_like(c), torch.empty_like(c)
        st_f, st_b, sw_f, sw_b = (torch.zeros((n,), dtype=torch.int32, device=dev) for _ in range(4))

        def forward():
            _native.check(lib.nastar_cost_to_go_sweeps(c.data_ptr(), g.data_ptr(), p.data_ptr(), n, size, size, mask, dist.data_ptr(), None,
                                                       st_f.data_ptr(), sw_f.data_ptr(), stream), "nastar_cost_to_go_sweeps")

        def backward():
            _native.check(lib.nastar_fields_backward(dist.data_ptr(), g.data_ptr(), p.data_ptr(), u.data_ptr(), n, size, size, mask, grad.data_ptr(),
                                                     st_b.data_ptr(), sw_b.data_ptr(), stream), "nastar_fields_backward")

        forward()
        backward()
        torch.cuda.synchronize()
        assert not st_f.any() and not st_b.any(), (st_f.tolist()[:8], st_b.tolist()[:8])
        ref = GO.field_grad(cost[0], goal[0].reshape(size, size), passable[0], up[0], mask)
        err = np.abs(grad[0].cpu().numpy().astype(np.float64) - ref.A)
        tol = 2.0 ** -23 * np.abs(ref.A) + 1e-9 * np.abs(up[0][ref.live].astype(np.float64)).sum()
        assert ref.status == 0 and (err <= tol).all(), f"{name}: the backward differs from the definition (max err {err.max():.3e})"
        t_f, t_b = event_ms(forward, args.reps), event_ms(backward, args.reps)
        swf, swb = sw_f.cpu().numpy(), sw_b.cpu().numpy()
        rows.append({"workload": name, "B": n, "H": size, "W": size, "neighbor_mask": mask, "reps": args.reps, "forward_ms": t_f, "backward_ms": t_b,
                     "forward_sweeps_median": float(np.median(swf)), "forward_sweeps_max": int(swf.max()),
                     "backward_sweeps_median": float(np.median(swb)), "backward_sweeps_max": int(swb.max()),
                     "forest_height_map0": int(ref.hops.max()) - 1, "live_cells_map0": int(ref.live.sum())})
        print(json.dumps(rows[-1]), flush=True)
    doc = {"probe": "tools/probe_fields_grad.py", "device": torch.cuda.get_device_name(dev), "timing": "device events around one launch, after 3 warm-up launches",
           "small": bool(args.small), "fields_grad_max_cells": ops.FIELDS_GRAD_MAX_CELLS, "workloads": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
