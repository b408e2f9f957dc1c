#!/usr/bin/env python3
"""Generate tests/golden/neighbors/*.npz by RUNNING THE REFERENCE ITSELF with a non-default ``neighbor_filter``.

The reference's ``DifferentiableAstar`` convolves every expansion with its ``neighbor_filter`` parameter; these vectors pin
what another 3x3 filter (von Neumann, an asymmetric move set) does there: histories, paths, the selection of every loop step,
the loop index at which the batch stopped, and L1 gradients w.r.t. the cost maps in training mode.

The reference module (``src/neural_astar/planner/differentiable_astar.py`` of a reference checkout) depends on torch only and is
loaded by file path.  The vectors live in a subdirectory so that the Moore-8 suites, which glob ``tests/golden/*.npz``, never see
them.  Every file stores its inputs (bit-packed masks, indices, fp32 costs), never an RNG stream.

Usage:  python tools/gen_golden_neighbors.py --reference <reference checkout>
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "neighbors")

VON_NEUMANN = [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
DOWN_RIGHT = [[1, 1, 0], [1, 0, 0], [0, 0, 0]]  # the issue's "down / right moves only": opens offsets (+1,+1), (+1,0), (0,+1)
ASYM = [[1, 1, 0], [1, 0, 1], [0, 1, 0]]        # von Neumann + the down-right diagonal (filter cell (0,0) opens offset (+1,+1))
# filters that set cells (0,2), (2,0), (2,2) -- bits 2, 6, 8, the offsets (+1,-1), (-1,+1), (-1,-1) -- without being Moore-8
UP_LEFT = [[0, 0, 0], [0, 0, 1], [0, 1, 1]]     # up, left and the up-left diagonal only: offsets (-1,0), (0,-1), (-1,-1)
MOORE_NO_DR = [[0, 1, 1], [1, 0, 1], [1, 1, 1]]  # Moore-8 without the down-right diagonal (filter cell (0,0))
MOORE_NO_DL = [[1, 1, 0], [1, 0, 1], [1, 1, 1]]  # Moore-8 without the down-left diagonal (filter cell (0,2)): cell (2,0) without (0,2)
ANTI = [[0, 0, 1], [0, 0, 1], [0, 1, 0]]        # directed: (+1,-1), (0,-1), (-1,0) -- cell (0,2) without (2,0)


def load_reference(checkout: str):
    path = os.path.join(checkout, "src", "neural_astar", "planner", "differentiable_astar.py")
    spec = importlib.util.spec_from_file_location("ref_differentiable_astar", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pack(mask: np.ndarray) -> np.ndarray:
    B = mask.shape[0]
    return np.packbits(mask.reshape(B, -1).astype(np.uint8), axis=1)


def moves(filt) -> list:
    """offsets (dr, dc) a filter opens: conv2d is a cross-correlation, filter cell (a, b) opens offset (1 - a, 1 - b)"""
    return [(1 - a, 1 - b) for a in range(3) for b in range(3) if filt[a][b]]


def reachable(passable: np.ndarray, s: int, filt) -> np.ndarray:
    """cells the search can open from s under the filter (the start is expanded even on an obstacle)"""
    H, W = passable.shape
    seen = np.zeros(H * W, bool)
    seen[s] = True
    frontier = [s]
    mv = moves(filt)
    while frontier:
        nxt = []
        for i in frontier:
            r, c = divmod(i, W)
            for dr, dc in mv:
                nr, nc = r + dr, c + dc
                if 0 <= nr < H and 0 <= nc < W and passable[nr, nc] and not seen[nr * W + nc]:
                    seen[nr * W + nc] = True
                    nxt.append(nr * W + nc)
        frontier = nxt
    return seen


def random_problems(B, H, W, filt, seed, p=0.2, max_dist=None):
    """i.i.d. obstacles with probability p; start / goal passable, the goal reachable from the start under `filt`
    (max_dist: |dr|, |dc| <= max_dist between them -- keeps the reference's loop on a large map short)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = np.zeros((B, H, W), np.float32)
    sidx = np.zeros(B, np.int64)
    gidx = np.zeros(B, np.int64)
    b = 0
    while b < B:
        m = rng.random((H, W)) > p
        cells = np.flatnonzero(m.reshape(-1))
        s = int(cells[rng.integers(cells.size)])
        reach = reachable(m, s, filt)
        reach[s] = False
        cand = np.flatnonzero(reach)
        if max_dist is not None:
            sr, sc = divmod(s, W)
            cr, cc = np.divmod(cand, W)
            cand = cand[(np.abs(cr - sr) <= max_dist) & (np.abs(cc - sc) <= max_dist) & ((np.abs(cr - sr) + np.abs(cc - sc)) >= max_dist // 2)]
        if cand.size == 0:
            continue
        maps[b], sidx[b], gidx[b] = m, s, int(cand[rng.integers(cand.size)])
        b += 1
    onehot = lambda idx: np.eye(H * W, dtype=np.float32)[idx].reshape(B, 1, H, W)  # noqa: E731
    return maps[:, None], onehot(sidx), onehot(gidx)


def fixture(B=1):
    """the reference's test fixture (tests/astar_test.py:5-14): 64x64, square obstacle, corner to corner"""
    m = np.ones((B, 1, 64, 64), np.float32)
    m[:, :, 24:48, 24:48] = 0
    s = np.zeros_like(m)
    s[:, :, 0, 0] = 1
    g = np.zeros_like(m)
    g[:, :, -1, -1] = 1
    return m, s, g


ONLY = None  # --only: the names to (re)write; every other case is still run (its asserts hold) but its file is left as it is


def run(ref, name, filt, maps, start, goal, cost=None, g_ratio=0.5, Tmax=1.0, training=False, target=None, store=False):
    B, _, H, W = maps.shape
    m = ref.DifferentiableAstar(g_ratio=g_ratio, Tmax=Tmax)
    with torch.no_grad():
        m.neighbor_filter.copy_(torch.tensor(filt, dtype=torch.float32).reshape(1, 1, 3, 3))
    m.train(training)
    cst = maps if cost is None else cost
    c = torch.from_numpy(cst.copy()).requires_grad_(target is not None)
    s, g, p = (torch.from_numpy(x) for x in (start, goal, maps))
    out = m(c, s, g, p, True)  # (store_intermediate_results: the per-step selections; no effect on the search)
    d = dict(H=H, W=W, B=B, g_ratio=np.float64(g_ratio), Tmax=np.float64(Tmax), training=bool(training),
             filter=np.asarray(filt, np.float32), map_bits=pack(maps),
             start_idx=start.reshape(B, -1).argmax(1).astype(np.int32), goal_idx=goal.reshape(B, -1).argmax(1).astype(np.int32))
    if cost is not None:
        d["cost"] = cost.astype(np.float32)
    hist = out.histories.detach().numpy()
    paths = out.paths.detach().numpy()
    assert set(np.unique(hist)).issubset({0.0, 1.0}), "histories must be exact 0/1"
    steps = out.intermediate_results[:-1]
    sel = np.stack([st["paths"].reshape(B, -1).argmax(1).numpy() for st in steps], 1).astype(np.int32)  # [B, t_batch + 1]
    d.update(hist_bits=pack(hist), path_bits=pack(paths), sel_log=sel, t_batch=np.int32(sel.shape[1] - 1),
             hist_sum=hist.reshape(B, -1).sum(1).astype(np.int32), path_sum=paths.reshape(B, -1).sum(1).astype(np.int32))
    if store:  # the reference's intermediate results themselves (store_intermediate_results=True), bit-packed
        d["inter_hist_bits"] = np.stack([pack(st["histories"].numpy()) for st in out.intermediate_results])
        d["inter_path_bits"] = np.stack([pack(st["paths"].numpy().astype(np.float32)) for st in out.intermediate_results])
    if target is not None:
        loss = torch.nn.L1Loss()(out.histories, torch.from_numpy(target))
        loss.backward()
        d["target_bits"] = pack(target)
        d["grad_cost"] = c.grad.detach().numpy().astype(np.float32)
    if ONLY is not None and name not in ONLY:
        return d
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
    print(f"{name}: B={B} {H}x{W} g_ratio={g_ratio} filter={np.asarray(filt).reshape(-1).tolist()} t_batch={sel.shape[1] - 1} "
          f"hist_sum[:4]={d['hist_sum'][:4]} path_sum[:4]={d['path_sum'][:4]}")
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="root of a reference checkout (holds src/neural_astar/planner/differentiable_astar.py)")
    ap.add_argument("--only", nargs="+", help="write only these vectors (the others stay byte-identical)")
    args = ap.parse_args()
    global ONLY
    ONLY = set(args.only) if args.only else None
    ref = load_reference(args.reference)
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)

    # 1. the reference's fixture: von Neumann 3395 / 127, down/right moves 1169 / 88 (Moore-8: 1169 / 88)
    d = run(ref, "fixture64_vn_g050", VON_NEUMANN, *fixture(), store=True)
    assert (int(d["hist_sum"][0]), int(d["path_sum"][0])) == (3395, 127)
    d = run(ref, "fixture64_dr_g050", DOWN_RIGHT, *fixture())
    assert (int(d["hist_sum"][0]), int(d["path_sum"][0])) == (1169, 88)
    # 2. an asymmetric filter on solvable random maps: pins the orientation (point reflection of the filter)
    run(ref, "rand32_asym_g050", ASYM, *random_problems(8, 32, 32, ASYM, seed=101))
    # 3. U(0,1) costs, B > 1, g_ratio 0.5 and 0.2 (0.2: the batch-coupled class is reachable -- the exact pipeline)
    rng = np.random.Generator(np.random.PCG64(7))
    pr = random_problems(8, 32, 32, VON_NEUMANN, seed=202)
    cost = rng.random((8, 1, 32, 32)).astype(np.float32)
    run(ref, "rand32_vn_ucost_g050", VON_NEUMANN, *pr, cost=cost, g_ratio=0.5)
    run(ref, "rand32_vn_ucost_g020", VON_NEUMANN, *pr, cost=cost, g_ratio=0.2)
    pr = random_problems(8, 32, 32, ASYM, seed=203)
    run(ref, "rand32_asym_ucost_g020", ASYM, *pr, cost=rng.random((8, 1, 32, 32)).astype(np.float32), g_ratio=0.2)
    # 4. a non-power-of-two shape, and a map of >= 6400 cells (the large-map kernel)
    pr = random_problems(4, 20, 45, VON_NEUMANN, seed=303)
    run(ref, "rand20x45_vn_ucost_g050", VON_NEUMANN, *pr, cost=rng.random((4, 1, 20, 45)).astype(np.float32))
    pr = random_problems(2, 80, 80, ASYM, seed=404, max_dist=10)
    run(ref, "rand80_asym_ucost_g050", ASYM, *pr, cost=rng.random((2, 1, 80, 80)).astype(np.float32))
    # 5. training mode (Tmax 0.25): L1 gradients w.r.t. the cost maps
    pr = random_problems(4, 32, 32, VON_NEUMANN, seed=505)
    tgt = (rng.random((4, 1, 32, 32)) < 0.2).astype(np.float32)
    run(ref, "grad_rand32_vn_train_T025", VON_NEUMANN, *pr, cost=rng.random((4, 1, 32, 32)).astype(np.float32), Tmax=0.25, training=True,
        target=tgt)
    pr = random_problems(2, 80, 80, ASYM, seed=606, max_dist=12)
    tgt = (rng.random((2, 1, 80, 80)) < 0.05).astype(np.float32)
    run(ref, "grad_rand80_asym_train_T025", ASYM, *pr, cost=rng.random((2, 1, 80, 80)).astype(np.float32), Tmax=0.25, training=True,
        target=tgt)
    # ... and one whose replay state no longer fits LDS (the fill / replay / sweep launches over the HBM workspace)
    pr = random_problems(2, 120, 120, VON_NEUMANN, seed=707, max_dist=10)
    tgt = (rng.random((2, 1, 120, 120)) < 0.02).astype(np.float32)
    run(ref, "grad_rand120_vn_train_T025", VON_NEUMANN, *pr, cost=rng.random((2, 1, 120, 120)).astype(np.float32), Tmax=0.25, training=True,
        target=tgt)
    # 6. the filter cells no filter above sets (0,2), (2,0), (2,2): small maps, U(0,1) costs (an RNG of its own: the vectors above stay as they are)
    rng = np.random.Generator(np.random.PCG64(808))
    pr = random_problems(6, 16, 16, UP_LEFT, seed=809)
    run(ref, "rand16_upleft_ucost_g050", UP_LEFT, *pr, cost=rng.random((6, 1, 16, 16)).astype(np.float32))
    pr = random_problems(6, 24, 20, MOORE_NO_DR, seed=810)
    run(ref, "rand24x20_moorenodr_ucost_g050", MOORE_NO_DR, *pr, cost=rng.random((6, 1, 24, 20)).astype(np.float32))
    pr = random_problems(6, 20, 20, ANTI, seed=811)
    run(ref, "rand20_antidl_ucost_g050", ANTI, *pr, cost=rng.random((6, 1, 20, 20)).astype(np.float32))
    # ... and g_ratio 0.8 with costs up to 10
    pr = random_problems(6, 18, 22, MOORE_NO_DL, seed=812)
    run(ref, "rand18x22_moorenodl_u10cost_g080", MOORE_NO_DL, *pr, cost=(10.0 * rng.random((6, 1, 18, 22))).astype(np.float32), g_ratio=0.8)
    pr = random_problems(4, 16, 16, UP_LEFT, seed=813)
    tgt = (rng.random((4, 1, 16, 16)) < 0.2).astype(np.float32)
    run(ref, "grad_rand16_upleft_train_T050", UP_LEFT, *pr, cost=rng.random((4, 1, 16, 16)).astype(np.float32), Tmax=0.5, training=True,
        target=tgt)


if __name__ == "__main__":
    main()
