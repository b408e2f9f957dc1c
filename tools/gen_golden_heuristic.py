#!/usr/bin/env python3
"""Generate tests/golden/heuristics/*.npz by RUNNING THE REFERENCE ITSELF with a replaced ``get_heuristic``.

The reference keeps its heuristic in an instance attribute and reads it once per call (``h = self.get_heuristic(goal_maps) + cost_maps``);
these vectors pin what the search does with ``get_heuristic = lambda goal_maps: h0`` for a caller's tensor ``h0``: zero (Dijkstra), twice the
default (weighted A*), random fields with negative values (an arbitrary learned output), alone and with a von Neumann filter, on sizes that
take every kernel family -- histories, paths, the selection of every loop step, the loop index at which the batch stopped, and for the
``grad_*`` files the reference's autograd gradient of an L1 loss w.r.t. the cost maps AND w.r.t. ``h0``.

The reference module depends on torch only and is loaded by file path; no reference program text enters the tree.  Every file stores its
inputs (bit-packed masks, indices, fp32 costs and heuristics), never an RNG stream.

A seed is REJECTED (the next one is tried) when the reference produces a NaN or when one of its picks leaves the quotient rule (DESIGN.md
section 2, item 5: the first flat index of the smallest fl(f / fl32(sqrt(W))), checked against tests/heuristic_oracle.py step by step);
the run fails when more than 1 seed in 20 is rejected.

Usage:  python tools/gen_golden_heuristic.py --reference <reference checkout>
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
import heuristic_oracle as HO  # noqa: E402
from gen_golden_neighbors import load_reference, pack, random_problems  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "heuristics")
MOORE = [[1, 1, 1], [1, 0, 1], [1, 1, 1]]
VON_NEUMANN = [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
STATS = {"tried": 0, "rejected": 0}


def mask_of(filt) -> int:
    return int(sum(1 << i for i, v in enumerate(np.asarray(filt).reshape(-1)) if v == 1))


def reference_run(ref, filt, maps, start, goal, cost, h0, g_ratio, Tmax, training, target, h0_only):
    m = ref.DifferentiableAstar(g_ratio=g_ratio, Tmax=Tmax)
    with torch.no_grad():
        m.neighbor_filter.copy_(torch.tensor(filt, dtype=torch.float32).reshape(1, 1, 3, 3))
    m.train(training)
    c = torch.from_numpy(cost.copy()).requires_grad_(target is not None and not h0_only)
    h = torch.from_numpy(h0.copy()).requires_grad_(target is not None)
    m.get_heuristic = lambda goal_maps: h[:, 0]
    s, g, p = (torch.from_numpy(x) for x in (start, goal, maps))
    out = m(c, s, g, p, True)
    grads = None
    if target is not None:
        torch.nn.L1Loss()(out.histories, torch.from_numpy(target)).backward()
        grads = (None if h0_only else c.grad.detach().numpy().astype(np.float32), h.grad.detach().numpy().astype(np.float32))
    return out, grads


def case(ref, name, make, filt=MOORE, g_ratio=0.5, Tmax=1.0, training=False, with_target=None, h0_only=False, seed=1, check=None):
    """``make(seed) -> (maps, start, goal, cost or None, h0)``; ``with_target``: density of the random L1 target (grad_* vectors);
    ``check(d, inputs)``: an extra condition on the accepted vector (asserted)."""
    while True:
        STATS["tried"] += 1
        maps, start, goal, cost, h0 = make(seed)
        B, _, H, W = maps.shape
        cst = maps if cost is None else cost
        target = None
        if with_target is not None:
            target = (np.random.Generator(np.random.PCG64(seed + 7919)).random((B, 1, H, W)) < with_target).astype(np.float32)
        out, grads = reference_run(ref, filt, maps, start, goal, cst, h0, g_ratio, Tmax, training, target, h0_only)
        hist = out.histories.detach().numpy()
        paths = out.paths.detach().numpy()
        steps = out.intermediate_results[:-1]
        sel = np.stack([st["paths"].reshape(B, -1).argmax(1).numpy() for st in steps], 1).astype(np.int32)  # [B, t_batch + 1]
        max_iters = int((Tmax if training else 1.0) * W * W)
        o = HO.search(cst, start, goal, maps, h0, g_ratio, max_iters, mask_of(filt), lockstep=B > 1)
        bad = (not np.isfinite(hist).all()) or (grads is not None and not all(np.isfinite(x).all() for x in grads if x is not None))
        bad = bad or any(o.sel[b] != sel[b].tolist() for b in range(B))
        if not bad:
            break
        STATS["rejected"] += 1
        print(f"{name}: seed {seed} rejected (NaN, or a pick of the reference outside the quotient rule)")
        seed += 1000
    assert set(np.unique(hist)).issubset({0.0, 1.0}), "histories must be exact 0/1"
    d = dict(H=H, W=W, B=B, g_ratio=np.float64(g_ratio), Tmax=np.float64(Tmax), training=bool(training), mask=np.int32(mask_of(filt)),
             map_bits=pack(maps), start_idx=start.reshape(B, -1).argmax(1).astype(np.int32), goal_idx=goal.reshape(B, -1).argmax(1).astype(np.int32),
             h0=h0.astype(np.float32), hist_bits=pack(hist), path_bits=pack(paths), sel_log=sel, t_batch=np.int32(sel.shape[1] - 1),
             h0_only=bool(h0_only))
    if cost is not None:
        d["cost"] = cost.astype(np.float32)
    if target is not None:
        d["target_bits"] = pack(target)
        if grads[0] is not None:
            d["grad_cost"] = grads[0]
        d["grad_h0"] = grads[1]
    if check is not None:
        check(d, (cst, start, goal, maps, h0, max_iters))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    print(f"{name}: B={B} {H}x{W} g_ratio={g_ratio} mask={mask_of(filt):#x} t_batch={sel.shape[1] - 1} seed={seed} "
          f"hist_sum={hist.reshape(B, -1).sum(1).astype(int).tolist()}")


def default_h0(ref, goal):
    return ref.get_heuristic(torch.from_numpy(goal[:, 0])).numpy()[:, None].astype(np.float32)


def problems(ref, B, H, W, kind, filt=MOORE, ucost=True, max_dist=None, p=0.2):
    def make(seed):
        rng = np.random.Generator(np.random.PCG64(seed))
        maps, start, goal = random_problems(B, H, W, filt, seed=seed + 1, p=p, max_dist=max_dist)
        cost = rng.random((B, 1, H, W)).astype(np.float32) if ucost else None
        if kind == "zero":
            h0 = np.zeros((B, 1, H, W), np.float32)
        elif kind == "w2":
            h0 = (2.0 * default_h0(ref, goal)).astype(np.float32)
        elif kind == "field":  # an arbitrary learned output: U(-1, 4)
            h0 = (rng.random((B, 1, H, W)) * 5.0 - 1.0).astype(np.float32)
        elif kind == "noisy":  # the default heuristic plus U(-0.5, 0.5): searches stay short on large maps
            h0 = (default_h0(ref, goal) + rng.random((B, 1, H, W)).astype(np.float32) - np.float32(0.5)).astype(np.float32)
        else:
            raise ValueError(kind)
        return maps, start, goal, cost, h0
    return make


def leaves_fixed_point(d, inputs):
    """the exact pipeline's class is hit: some map searched ALONE differs from its row in the batch"""
    cst, start, goal, maps, h0, max_iters = inputs
    B = int(d["B"])
    alone = HO.search(cst, start, goal, maps, h0, float(d["g_ratio"]), max_iters, int(d["mask"]), lockstep=False)
    differs = [b for b in range(B) if not np.array_equal(pack(alone.histories[b:b + 1]), d["hist_bits"][b:b + 1])]
    assert differs, "no map of this batch leaves its fixed point: pick another seed"
    print(f"    maps that leave their fixed point: {differs}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a reference checkout (holds src/neural_astar/planner/differentiable_astar.py)")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)

    # Dijkstra: long searches, many exact ties
    case(ref, "zero32_binary_g050", problems(ref, 2, 32, 32, "zero", ucost=False), seed=11)
    case(ref, "zero32_ucost_g050", problems(ref, 2, 32, 32, "zero"), seed=12)
    # weighted A* on a size that runs a hand-scheduled stream by default
    case(ref, "w2_64_ucost_g050", problems(ref, 2, 64, 64, "w2", p=0.35), seed=13)
    # an arbitrary field with negative values, a non-power-of-two shape
    case(ref, "field20x45_ucost_g050", problems(ref, 3, 20, 45, "field"), seed=14)
    case(ref, "field20x45_ucost_g020", problems(ref, 3, 20, 45, "field"), g_ratio=0.2, seed=15)
    # a batch in which a map leaves its fixed point at g_ratio 0.5: the exact pipeline
    case(ref, "coupled_field24_ucost_g050", problems(ref, 6, 24, 24, "field"), seed=16, check=leaves_fixed_point)
    # composition with neighbor_filter
    case(ref, "zero32_vn_ucost_g050", problems(ref, 2, 32, 32, "zero", filt=VON_NEUMANN), filt=VON_NEUMANN, seed=17)
    # the large-map kernel
    case(ref, "noisy96_ucost_g050", problems(ref, 2, 96, 96, "noisy", max_dist=40, p=0.3), seed=18)
    case(ref, "w2_140x150_ucost_g050", problems(ref, 2, 140, 150, "w2", max_dist=60, p=0.35), seed=19)
    # gradients: every replay route
    case(ref, "grad_field32_train_T025", problems(ref, 4, 32, 32, "field"), Tmax=0.25, training=True, with_target=0.2, seed=21)
    case(ref, "grad_noisy80_eval_g050", problems(ref, 2, 80, 80, "noisy", max_dist=30, p=0.3), with_target=0.05, seed=22)
    case(ref, "grad_coupled_field24_g050", problems(ref, 6, 24, 24, "field"), with_target=0.2, seed=16, check=leaves_fixed_point)
    case(ref, "grad_h0only_field32_binary_g050", problems(ref, 3, 32, 32, "field", ucost=False), with_target=0.2, h0_only=True, seed=24)
    case(ref, "grad_w2_140x150_eval_g050", problems(ref, 1, 140, 150, "w2", max_dist=40, p=0.35), with_target=0.02, seed=25)

    print(f"seeds tried {STATS['tried']}, rejected {STATS['rejected']}")
    assert STATS["rejected"] * 20 <= STATS["tried"], "the reference left the quotient rule (or produced NaN) on more than 1 seed in 20"


if __name__ == "__main__":
    main()
