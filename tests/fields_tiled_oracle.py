"""The TILED relaxation of include/nastar_fields_tiled.h in numpy: the scheme the kernels follow, with the
freedom the hardware has made explicit -- tiles of a round run in a random order, and every halo cell a tile reads is, at random, either
what it holds NOW (another tile of this round may already have lowered it) or what it held when the round BEGAN (stale).  The claim under
test is that none of this changes a bit of the result: ``tiled_field`` == ``fields_oracle.field``.

Also here, shared by the CPU and the GPU tests: the serpentine of corridors, whose cheapest routes cross tile borders dozens of times.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_oracle as FO  # noqa: E402
from heuristic_oracle import MOORE8, offsets  # noqa: E402

f32 = np.float32
STATUS_NO_CONVERGENCE = 10
NEIGHBOUR_TILES = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def _local_fixed_point(win, c, moves):
    """win [(rows+2),(cols+2)]: the tile with its halo (halo fixed), c [rows,cols] the cost with obstacles as +inf -> the relaxed interior"""
    rows, cols = c.shape
    with np.errstate(invalid="ignore"):
        while True:
            nb = np.min([win[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols] for dy, dx in moves], axis=0) if moves else np.full_like(c, np.inf)
            new = np.minimum(win[1:-1, 1:-1], (c + nb).astype(f32))
            if np.array_equal(new, win[1:-1, 1:-1]):
                return new
            win[1:-1, 1:-1] = new


def tiled_field(cost, goal, passable, mask=MOORE8, tile=(64, 64), rng=None, max_rounds=None, init="halo"):
    """[H,W] arrays -> (D [H,W] f32, status, rounds, tile visits).  ``rng``: None = every halo read fresh, tiles in index order; a numpy
    Generator = random order, every halo CELL fresh or one round stale at random.  ``init``: "halo" marks every tile whose interior plus
    one-cell halo holds a passable goal (the kernels' rule); "own" only the tile that holds it -- the WRONG rule, kept to show the trap."""
    cost, ok, goal = np.asarray(cost, f32), np.asarray(passable) != 0, np.asarray(goal) != 0
    H, W = cost.shape
    th, tw = tile
    ty, tx = -(-H // th), -(-W // tw)
    if (ok & ~(cost >= 0)).any():
        return np.full((H, W), np.inf, f32), FO.STATUS_BAD_COST, 0, 0
    moves = offsets(mask)
    c = np.where(ok, cost, f32(np.inf)).astype(f32)
    pad = np.full((H + 2, W + 2), np.inf, f32)      # R with a ring of +inf: pad[y + 1, x + 1] = R[y, x]
    pad[1:-1, 1:-1] = np.where(goal & ok, f32(0), f32(np.inf))
    pg = np.zeros((H + 2, W + 2), bool)
    pg[1:-1, 1:-1] = goal & ok
    active = np.zeros((ty, tx), bool)
    for i in range(ty):
        for j in range(tx):
            y0, x0, y1, x1 = i * th, j * tw, min(H, (i + 1) * th), min(W, (j + 1) * tw)
            active[i, j] = pg[y0:y1 + 2, x0:x1 + 2].any() if init == "halo" else pg[y0 + 1:y1 + 1, x0 + 1:x1 + 1].any()
    bound = H * W + 1
    limit = bound if max_rounds is None else min(max_rounds, bound)
    rounds = visits = 0
    while active.any() and rounds < limit:
        rounds += 1
        old = pad.copy()                           # what every cell held when the round began
        nxt = np.zeros_like(active)
        todo = np.argwhere(active)
        if rng is not None:
            rng.shuffle(todo)
        for i, j in todo:
            visits += 1
            y0, x0, y1, x1 = i * th, j * tw, min(H, (i + 1) * th), min(W, (j + 1) * tw)
            win = pad[y0:y1 + 2, x0:x1 + 2].copy()
            if rng is not None:
                stale = rng.random(win.shape) < 0.5
                stale[1:-1, 1:-1] = False          # the interior is the tile's own: nobody else writes it
                win = np.where(stale, old[y0:y1 + 2, x0:x1 + 2], win)
            before = pad[y0 + 1:y1 + 1, x0 + 1:x1 + 1].copy()
            new = _local_fixed_point(win, c[y0:y1, x0:x1], moves)
            low = new < before
            pad[y0 + 1:y1 + 1, x0 + 1:x1 + 1] = new
            for dy, dx in NEIGHBOUR_TILES:
                rows = slice(0, 1) if dy < 0 else slice(-1, None) if dy > 0 else slice(None)
                cols = slice(0, 1) if dx < 0 else slice(-1, None) if dx > 0 else slice(None)
                if 0 <= i + dy < ty and 0 <= j + dx < tx and low[rows, cols].any():
                    nxt[i + dy, j + dx] = True
        active = nxt
    r = pad[1:-1, 1:-1]
    status = STATUS_NO_CONVERGENCE if active.any() else FO.STATUS_OK if goal.any() else FO.STATUS_NO_GOAL
    return np.where(goal, f32(0), r), status, rounds, visits


def serpentine(H, W):
    """cost (ones), goal (at (0, 0)), passable: a wall on every third row with ONE opening, at the right end, then the left end, and so on
    -> (cost, goal, passable, the number of walls).  The only route from the bottom runs every corridor from end to end."""
    passable = np.ones((H, W), f32)
    walls = 0
    for r in range(2, H - 1, 3):
        passable[r, :] = 0
        passable[r, W - 1 if walls % 2 == 0 else 0] = 1
        walls += 1
    goal = np.zeros((H, W), f32)
    goal[0, 0] = 1
    return np.ones((H, W), f32), goal, passable, walls
