#!/usr/bin/env python3
"""Generate tests/golden/multisource/*.npz by RUNNING THE REFERENCE ITSELF on MULTI-HOT start maps.

The reference's ``DifferentiableAstar.forward()`` never asks for a one-hot start map: ``open_maps = start_maps``, so a map with K start cells is
searched from all of them at once and ``backtrack`` marks the route from the goal to whichever start reached it.  These vectors pin that:
histories, paths, the selection of every loop step, the loop index at which the batch stopped and, for the ``grad_*`` files, the reference's
fp32 autograd gradient of an L1 loss w.r.t. the cost maps (and the heuristic).  Sizes and placements take every kernel family: several
starts in one 16-cell chunk, starts at cell 0 and HW-1, every cell a start, the goal among the starts, a re-parented start on a path
(signed costs), the lock-step batch loop (g_ratio 0.2), a von Neumann filter, a caller's heuristic, and large maps with starts inside one
64-cell chunk, inside one 4096-cell super-chunk and across super-chunks.

The reference module depends on torch only and is loaded by file path (``gen_golden_neighbors.load_reference``); no reference program text
enters the tree.  Every file stores its inputs (bit-packed masks, indices, fp32 costs and heuristics), never an RNG stream.

A seed is REJECTED (the next one is tried) when the reference produces a NaN or raises, or when the restatement (tests/multisource_oracle.py)
leaves the reference -- the tie class of DESIGN.md section 2, item 5.  At most 1 seed in 10 per vector; the counts are stored in the file.
A vector that is CONSTRUCTED for a property (a path through two start cells, a map that leaves its fixed point) first looks for a seed with
that property using the restatement alone; those looks are not rejections.

Usage:  python tools/gen_golden_multisource.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import multisource_oracle as MO  # noqa: E402
from gen_golden_neighbors import load_reference, pack, random_problems  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "multisource")
MOORE = [[1, 1, 1], [1, 0, 1], [1, 1, 1]]
VON_NEUMANN = [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
MAX_REJECT = 0.1


def mask_of(filt) -> int:
    return int(sum(1 << i for i, v in enumerate(np.asarray(filt).reshape(-1)) if v == 1))


def reference_run(ref, filt, maps, start, goal, cost, h0, g_ratio, Tmax, training, target, h0_only):
    m = ref.DifferentiableAstar(g_ratio=g_ratio, Tmax=Tmax)
    with torch.no_grad():
        m.neighbor_filter.copy_(torch.tensor(filt, dtype=torch.float32).reshape(1, 1, 3, 3))
    m.train(training)
    c = torch.from_numpy(cost.copy()).requires_grad_(target is not None and not h0_only)
    h = None
    if h0 is not None:
        h = torch.from_numpy(h0.copy()).requires_grad_(target is not None)
        m.get_heuristic = lambda goal_maps: h[:, 0]
    s, g, p = (torch.from_numpy(x) for x in (start, goal, maps))
    out = m(c, s, g, p, True)
    grads = None
    if target is not None:
        torch.nn.L1Loss()(out.histories, torch.from_numpy(target)).backward()
        grads = (None if h0_only else c.grad.detach().numpy().astype(np.float32), None if h is None else h.grad.detach().numpy().astype(np.float32))
    B = maps.shape[0]
    sel = np.stack([st["paths"].reshape(B, -1).argmax(1).numpy() for st in out.intermediate_results[:-1]], 1).astype(np.int32)
    return out.histories.detach().numpy(), out.paths.detach().numpy(), sel, grads


def sources(maps, start, goal, K, seed, place=None):
    """the one-hot ``start`` of random_problems (its goal is reachable from it) plus K-1 further start cells per map: ``place(b, H, W, s0, rng)
    -> cells`` or, by default, distinct random passable cells other than the goal"""
    rng = np.random.Generator(np.random.PCG64(seed))
    B, _, H, W = maps.shape
    out = start.copy()
    for b in range(B):
        s0 = int(start[b].reshape(-1).argmax())
        gi = int(goal[b].reshape(-1).argmax())
        if place is not None:
            extra = [int(c) for c in place(b, H, W, s0, rng)]
        else:
            cand = np.flatnonzero(maps[b].reshape(-1))
            cand = cand[(cand != s0) & (cand != gi)]
            extra = [int(c) for c in rng.choice(cand, size=min(K - 1, cand.size), replace=False)]
        out[b].reshape(-1)[extra] = 1
    return out


def case(ref, name, make, filt=MOORE, g_ratio=0.5, Tmax=1.0, training=False, with_target=None, h0_only=False, seed=1, prop=None, alone=False):
    """``make(seed) -> (maps, start, goal, cost or None, h0 or None)`` with multi-hot ``start``; ``with_target``: density of the random L1 target;
    ``prop(result, maps_state, inputs) -> bool``: the property the vector is constructed for (looked for with the restatement, then asserted);
    ``alone``: also store the reference's run of every map on its own."""
    mask = mask_of(filt)
    tried = rejected = 0
    while True:
        maps, start, goal, cost, h0 = make(seed)
        B, _, H, W = maps.shape
        cst = maps if cost is None else cost
        max_iters = int((Tmax if training else 1.0) * W * W)
        o, states = MO.search(cst, start, goal, maps, h0, g_ratio, max_iters, mask, lockstep=B > 1, with_maps=True)
        if (o.status != 0).any() or (prop is not None and not prop(o, states, (cst, start, goal, maps, h0, max_iters, g_ratio, mask))):
            seed += 1  # (a look for the property, or an unsolvable draw: not a rejection)
            continue
        tried += 1
        target = None
        if with_target is not None:
            target = (np.random.Generator(np.random.PCG64(seed + 7919)).random((B, 1, H, W)) < with_target).astype(np.float32)
        try:
            hist, paths, sel, grads = reference_run(ref, filt, maps, start, goal, cst, h0, g_ratio, Tmax, training, target, h0_only)
            bad = (not np.isfinite(hist).all()) or (grads is not None and not all(np.isfinite(x).all() for x in grads if x is not None))
            bad = bad or any(o.sel[b] != sel[b].tolist() for b in range(B)) or not np.array_equal(o.histories, hist[:, 0]) \
                or not np.array_equal(o.paths, paths[:, 0])
        except (IndexError, RuntimeError) as e:
            print(f"{name}: the reference raised {type(e).__name__}: {e}")
            bad = True
        if not bad:
            break
        rejected += 1
        print(f"{name}: seed {seed} rejected (NaN, an exception, or the restatement left the reference)")
        assert tried < 40, f"{name}: {rejected} of {tried} seeds rejected"
        seed += 1000
    assert rejected <= MAX_REJECT * tried, f"{name}: {rejected} of {tried} seeds rejected (the cap is 1 in 10)"
    assert set(np.unique(hist)).issubset({0.0, 1.0}), "histories must be exact 0/1"
    d = dict(H=H, W=W, B=B, g_ratio=np.float64(g_ratio), Tmax=np.float64(Tmax), training=bool(training), mask=np.int32(mask),
             map_bits=pack(maps), start_bits=pack(start), goal_idx=goal.reshape(B, -1).argmax(1).astype(np.int32),
             hist_bits=pack(hist), path_bits=pack(paths), sel_log=sel, t_batch=np.int32(sel.shape[1] - 1), h0_only=bool(h0_only),
             seeds_tried=np.int32(tried), seeds_rejected=np.int32(rejected), seed=np.int32(seed))
    if cost is not None:
        d["cost"] = cost.astype(np.float32)
    if h0 is not None:
        d["h0"] = h0.astype(np.float32)
    if target is not None:
        d["target_bits"] = pack(target)
        if grads[0] is not None:
            d["grad_cost"] = grads[0]
        if grads[1] is not None:
            d["grad_h0"] = grads[1]
    if alone:
        ah, ap = [], []
        for b in range(B):
            sl = slice(b, b + 1)
            h1, p1, _, _ = reference_run(ref, filt, maps[sl], start[sl], goal[sl], cst[sl], None if h0 is None else h0[sl], g_ratio, Tmax, training,
                                         None, False)
            o1 = MO.search(cst[sl], start[sl], goal[sl], maps[sl], None if h0 is None else h0[sl], g_ratio, max_iters, mask)
            assert np.array_equal(o1.histories, h1[:, 0]) and np.array_equal(o1.paths, p1[:, 0]), f"{name}: map {b} alone leaves the restatement"
            ah.append(h1)
            ap.append(p1)
        d["alone_hist_bits"] = pack(np.concatenate(ah))
        d["alone_path_bits"] = pack(np.concatenate(ap))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) < 256 * 1024, f"{name}: {os.path.getsize(path)} bytes"
    print(f"{name}: B={B} {H}x{W} g_ratio={g_ratio} mask={mask:#x} t_batch={sel.shape[1] - 1} seed={seed} tried={tried} rejected={rejected} "
          f"K={start.reshape(B, -1).sum(1).astype(int).tolist()} hist_sum={hist.reshape(B, -1).sum(1).astype(int).tolist()} "
          f"{os.path.getsize(path)} bytes")


def problems(B, H, W, K, filt=MOORE, cost="unit", h0=None, max_dist=None, p=0.2, place=None):
    """cost: "unit" (cost map = map design), "u01" U(0,1), "signed" U(-0.5, 1), "scaled" 1.5 + 2 U(0,1); h0: None or "field" U(-1, 4)"""
    def make(seed):
        rng = np.random.Generator(np.random.PCG64(seed))
        maps, start, goal = random_problems(B, H, W, filt, seed=seed + 1, p=p, max_dist=max_dist)
        u = rng.random((B, 1, H, W))
        c = {"unit": None, "u01": u, "signed": 1.5 * u - 0.5, "scaled": 1.5 + 2.0 * u}[cost]
        c = None if c is None else c.astype(np.float32)
        h = (rng.random((B, 1, H, W)) * 5.0 - 1.0).astype(np.float32) if h0 == "field" else None
        return maps, sources(maps, start, goal, K, seed + 2, place), goal, c, h
    return make


def same_chunk(b, H, W, s0, rng):
    """16x16: a start pair adjacent in one row (one 16-cell chunk), and the corner cells 0 and HW-1 (whatever they hold)"""
    r, c = divmod(s0, W)
    return [r * W + (c + 1 if c + 1 < W else c - 1), 0, H * W - 1]


def clustered(b, H, W, s0, rng):
    """two more starts next to the first one: with signed costs one of them is often re-parented and ends up on the path"""
    r, c = divmod(s0, W)
    nb = [(r + dr) * W + c + dc for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr or dc) and 0 <= r + dr < H and 0 <= c + dc < W]
    return rng.choice(nb, size=2, replace=False)


def large_spread(b, H, W, s0, rng):
    """96x96 (three 4096-cell super-chunks): a start in the first start's 64-cell chunk, one in its super-chunk but another chunk, one in
    another super-chunk"""
    C, S = s0 >> 6, s0 >> 12
    in_chunk = C * 64 + ((s0 & 63) + 5) % 64
    other_chunk = (S << 12) + ((((C & 63) + 17) % 64) << 6) + 9
    other_super = (((S + 1) % ((H * W + 4095) >> 12)) << 12) + 70
    return [min(x, H * W - 1) for x in (in_chunk, other_chunk, other_super)]


def dense8(seed):
    """map 0: every passable non-goal cell is a start; map 1: three starts, the goal among them"""
    maps, start, goal = random_problems(2, 8, 8, MOORE, seed=seed + 1, p=0.2)
    g = goal.reshape(2, -1).argmax(1)
    start[0].reshape(-1)[:] = maps[0].reshape(-1)
    start[0].reshape(-1)[g[0]] = 0
    cand = np.flatnonzero(maps[1].reshape(-1))
    start[1].reshape(-1)[[int(g[1]), int(cand[len(cand) // 2])]] = 1
    return maps, start, goal, None, None


def two_starts_on_a_path(o, states, inputs):
    start = inputs[1]
    B = start.shape[0]
    return any(int((o.paths[b].reshape(-1) * (start[b].reshape(-1) != 0)).sum()) >= 2 for b in range(B))


def leaves_fixed_point(o, states, inputs):
    cst, start, goal, maps, h0, max_iters, g_ratio, mask = inputs
    al = MO.search(cst, start, goal, maps, h0, g_ratio, max_iters, mask, lockstep=False)
    return any(not np.array_equal(al.histories[b], o.histories[b]) for b in range(start.shape[0]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a reference checkout (holds src/neural_astar/planner/differentiable_astar.py)")
    ap.add_argument("--only", nargs="+", help="write only these vectors")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)

    def run(name, *a, **k):
        if args.only is None or name in args.only:
            case(ref, name, *a, **k)

    # forward vectors
    run("unit16_samechunk", problems(4, 16, 16, 4, place=same_chunk), seed=31)
    run("unit32_k4", problems(3, 32, 32, 4, p=0.4), seed=32)
    run("unit64_k8", problems(2, 64, 64, 8, p=0.42), seed=33)
    run("field20x45_k3", problems(3, 20, 45, 3, cost="u01"), seed=34)
    run("dense8_allstarts", dense8, seed=35)
    run("signed12_reparent", problems(4, 12, 12, 3, cost="signed", place=clustered), seed=36, prop=two_starts_on_a_path)
    run("coupled16_g020", problems(4, 16, 16, 3, cost="scaled"), g_ratio=0.2, seed=37, prop=leaves_fixed_point, alone=True)
    run("vn20_k3", problems(3, 20, 20, 3, filt=VON_NEUMANN, cost="u01"), filt=VON_NEUMANN, seed=38)
    run("heur24_k3", problems(3, 24, 24, 3, cost="u01", h0="field"), seed=39)
    run("large96_k4", problems(2, 96, 96, 4, cost="u01", max_dist=30, p=0.3, place=large_spread), seed=40)
    run("large140x150_k3", problems(2, 140, 150, 3, cost="u01", max_dist=40, p=0.3), seed=41)
    # gradient vectors: the reference's fp32 autograd
    run("grad_unit32_train_T025_k3", problems(4, 32, 32, 3, p=0.4), Tmax=0.25, training=True, with_target=0.2, seed=51)
    run("grad_field20x45_eval_k4", problems(3, 20, 45, 4, cost="u01"), with_target=0.2, seed=52)
    run("grad_coupled16_g020_k3", problems(4, 16, 16, 3, cost="scaled"), g_ratio=0.2, with_target=0.2, seed=37, prop=leaves_fixed_point)
    run("grad_large96_k3", problems(2, 96, 96, 3, cost="u01", max_dist=24, p=0.3), with_target=0.05, seed=54)
    # (96x96 replays with its state in LDS; 120x120 is the smallest square whose replay state lives in the HBM workspace)
    run("grad_large120_k3", problems(1, 120, 120, 3, cost="u01", max_dist=24, p=0.3), with_target=0.02, seed=55)
    run("grad_h0only_24_k3", problems(3, 24, 24, 3, h0="field"), with_target=0.2, h0_only=True, seed=56)


if __name__ == "__main__":
    main()
