"""Bare back-to-back search launches: bench.Runner's nastar_forward_ex calls on preallocated outputs -- no event, no proof launch, no
allocation -- on never-searched batches with the loader's placement.  The program to trace when the boundary between two search launches
is the question (rocprofv3 --kernel-trace -- python tools/probe_bare_launches.py; then tools/launch_gaps.py on the trace).
Usage (GPU box): python tools/probe_bare_launches.py [--steps 200] [--warmup 20] [--workload maze32] [--batch 4096] [--placement dataset]
Prints one JSON line: host-clock microseconds per launch over the timed steps (one synchronise at the end)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "neural-astar_amd"), ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="maze32")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--placement", default="dataset", choices=["dataset", "natural"])
    a = ap.parse_args()
    import torch
    import bench
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    prs = bench.make_problems([(a.workload, bench.B_PER_GPU, 1234 + 1000 * k) for k in range(bench.N_ROTATE)])
    pool = bench.FreshBatches(a.workload, dev, prs, seed=4321)
    sets = [pool.batch(a.batch) for _ in range(min(a.steps + a.warmup, bench.MAX_FRESH_SETS))]
    run = bench.Runner(sets, dev, placement=a.placement)
    warm = bench.Runner([pool.batch(a.batch) for _ in range(bench.N_ROTATE)], dev, placement=a.placement)
    bench.prewarm(warm, dev)
    for _ in range(a.warmup):
        run.step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        run.step()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    assert int(run.status.abs().sum().item()) == 0
    print(json.dumps({"workload": a.workload, "batch": a.batch, "placement": a.placement, "steps": a.steps, "us_per_launch": dt / a.steps * 1e6,
                      "lib": os.environ.get("NASTAR_LIB", "product")}))


if __name__ == "__main__":
    main()
