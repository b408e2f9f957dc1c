#!/usr/bin/env python3
"""What the multi-source search costs: one search launch per configuration, timed with HIP events (median of --reps launches), for
  (a) masked_moore8   the MASKED instantiations with the Moore-8 mask on one-hot start maps (nastar_forward_ex_masked) -- the yardstick: the
                      multi-source kernels are these plus a seeding pass;
  (b) sources_onehot  the MULTI-SOURCE instantiations (nastar_forward_sources) on the same one-hot inputs: the selection overhead;
  (c) sources_k8      the same batch with 8 start cells per map (7 more random passable cells): shorter searches, a longer seeding pass.
Workloads: 4096 mazes of 32x32 and 256 random maps of 512x512 (15 % obstacles, U(0,1) costs), as tools/probe_heuristic.py.
  (d) seed_*          the large-map kernel's seeding pass alone: launches with a budget of ONE step (fill + seeding + one step + store), masked
                      against multi-source, at 512x512 (256 maps) and 1024x1024 (16 maps).  The pass runs in the searching wavefront
                      (csrc/nastar_search_hybrid.hip.h: hybrid_open_sources); a fill-launch variant does not exist in the tree.
  (e) replay_*        the replay backward (HBM state) of 16 of the 512x512 searches: masked against multi-source (one-hot starts).
One JSON line per configuration: median, min and max of the reps.

Usage:  python tools/probe_multisource.py [--reps 5]
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


def timed(run, reps):
    out = run()  # warm-up (and the outputs)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return out, ts


def more_starts(s, p, g, k, seed):
    """k start cells per map: the given one plus k - 1 random passable cells other than the goal"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sn, pn, gn = (x.cpu().numpy().copy() for x in (s, p, g))
    B = sn.shape[0]
    for b in range(B):
        cand = np.flatnonzero((pn[b].reshape(-1) != 0) & (gn[b].reshape(-1) == 0) & (sn[b].reshape(-1) == 0))
        sn[b].reshape(-1)[rng.choice(cand, k - 1, replace=False)] = 1
    return torch.from_numpy(sn).to(s.device)


def report(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind, nmaps in (("maze32", 4096), ("rand512", 256)):
        cost, s, g, p = (x[:nmaps].contiguous() for x in problems(kind, dev))
        if kind == "maze32":
            p = cost  # (one tensor, as VanillaAstar hands it over)
        B, H, W = cost.shape
        s8 = more_starts(s, p, g, 8, seed=9)
        ref = None
        for label, start, kw in (("masked_moore8", s, {"neighbor_mask": ops.NEIGHBORS_MOORE8}), ("masked_moore8_again", s, {"neighbor_mask": ops.NEIGHBORS_MOORE8}),
                                 ("sources_onehot", s, {"multi_source": True}), ("sources_k8", s8, {"multi_source": True})):
            out, ts = timed(lambda: ops.search_nograd(cost, start, g, p, 0.5, W * W, **kw), args.reps)
            h = out[0].cpu()
            same = None if ref is None else bool(torch.equal(ref, h))
            ref = h if ref is None else ref
            report(workload=kind, B=B, H=H, W=W, config=label, ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)),
                   maps_per_s=B / (float(np.median(ts)) * 1e-3), expansions=int(out[0].sum().item()), unsolved=int((out[3] != 0).sum().item()),
                   equal_to_masked=same)
        if kind == "rand512":
            for label, start, kw in (("seed_masked_1step", s, {"neighbor_mask": ops.NEIGHBORS_MOORE8}), ("seed_sources_1step", s, {"multi_source": True}),
                                     ("seed_sources_k8_1step", s8, {"multi_source": True})):
                out, ts = timed(lambda: ops.search_nograd(cost, start, g, p, 0.5, 1, **kw), args.reps)
                report(workload=kind, B=B, H=H, W=W, config=label, ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))
            # the replay backward of the same searches (HBM state; 16 maps): the masked replay against the multi-source replay, whose
            # wavefront reads the whole start map before its first step
            nb = 16
            c16, s16, g16, p16 = (x[:nb].contiguous() for x in (cost, s, g, p))
            hist, _, iters, _, log = ops.search_nograd(c16, s16, g16, p16, 0.5, W * W, True, neighbor_mask=ops.NEIGHBORS_MOORE8)
            up = torch.ones_like(hist)
            tb = ops.BatchCoupling.t_batch(iters)
            ref = None
            for label, kw in (("replay_masked", {"neighbor_mask": ops.NEIGHBORS_MOORE8}), ("replay_sources", {"multi_source": True})):
                out, ts = timed(lambda: ops._replay(c16, s16, g16, p16, log, 0.5, W * W, iters, tb, None, 0, label, grad_hist=up, **kw), args.reps)
                same = None if ref is None else bool(torch.equal(ref, out))
                ref = out if ref is None else ref
                report(workload=kind, B=nb, H=H, W=W, config=label, ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)),
                       steps_max=int(iters.max().item()), equal_to_masked=same)
    # 1024 x 1024: the largest map the kernels take; one-hot starts, a budget of one step
    B, H = 16, 1024
    rng = np.random.Generator(np.random.PCG64(17))
    cost = torch.from_numpy(rng.random((B, H, H)).astype(np.float32)).to(dev)
    p = torch.ones_like(cost)
    s = torch.zeros_like(cost)
    g = torch.zeros_like(cost)
    s[:, 3, 5] = 1
    g[:, H - 4, H - 6] = 1
    for label, kw in (("seed_masked_1step", {"neighbor_mask": ops.NEIGHBORS_MOORE8}), ("seed_sources_1step", {"multi_source": True})):
        out, ts = timed(lambda: ops.search_nograd(cost, s, g, p, 0.5, 1, **kw), args.reps)
        report(workload="ones1024", B=B, H=H, W=H, config=label, ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))


if __name__ == "__main__":
    main()
