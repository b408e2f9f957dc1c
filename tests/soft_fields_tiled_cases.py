"""The cases tests/test_soft_fields_tiled.py (CPU) and tests/test_soft_fields_tiled_gpu.py share: the maps above the one-workgroup limits
that are compared with the float64 definition of tests/soft_fields_oracle.py, and the far corner of the index range."""
import functools

import numpy as np

import soft_fields_oracle as SO

f32, f64 = np.float32, np.float64

# (H, W, B, seed, K): 48x130 is over the one-workgroup backward's 6144 cells, 130x140 over the forward's 12288 too.  NOT the default horizon:
# at 2 * (H + W) = 356 the float32 restatement of 48x130 reaches 1.2e-6 / 3.6e-5, too close to the bounds for a kernel to be judged by them
ABOVE = ((48, 130, 2, 11, 60), (130, 140, 1, 14, 97))
ABOVE_MASKS = (SO.MOORE8, 0x0AA)


@functools.lru_cache(maxsize=None)
def maps(H, W, B, seed):
    return SO.random_maps(seed, B, H, W)


def upstream(seed, live):
    """a random upstream gradient with a NaN on every cell that is not live at the horizon"""
    G = np.random.default_rng(seed).standard_normal(live.shape)
    return np.where(live, G, np.nan)


# ---- the maximum-entropy loss: two 130x140 maps, K = 97, a start 40 moves from the goal ------------------------------------------------------------
MAXENT_TAUS = (0.05, 0.5)


@functools.lru_cache(maxsize=None)
def maxent_maps():
    """cost, passable, goal, start: [2,H,W] each"""
    H, W, _, seed, _ = ABOVE[1]
    cost, passable, goal = maps(H, W, 2, seed + 100)
    start = np.zeros_like(goal)
    for b in range(2):
        start[b][tuple(np.argwhere(SO.hops(goal[b], passable[b]) == 40)[b])] = 1
    return cost, passable, goal, start


# ---- the far corner: one 1024 x 1152 map (the limit, 1179648 cells), K = 8, the goal in the last row ------------------------------------------
CORNER_H, CORNER_W, CORNER_K, CORNER_TAU, CORNER_C = 1024, 1152, 8, 0.5, 3
CORNER_GOAL = (CORNER_H - 1, CORNER_W - 3)
CORNER_START = (CORNER_H - 2, CORNER_W - 5)     # two moves from the goal: the one-hot upstream gradient sits here
# No cell more than K moves from the goal is finite or live (tests/test_soft_fields.py holds the definition to that), so the definition
# is evaluated on the WINDOW of the last 24 rows and 48 columns: the goal is more than K cells from the window's two inner edges, where the
# cut reads as +inf exactly as the cells beyond it do, and the other two edges are the map's own
CORNER_WINDOW = (slice(CORNER_H - 24, CORNER_H), slice(CORNER_W - 48, CORNER_W))


@functools.lru_cache(maxsize=None)
def corner_maps():
    """cost, passable, goal: [1,H,W] each; the start, the goal and the cells between them are passable"""
    cost, passable, goal = SO.random_maps(17, 1, CORNER_H, CORNER_W)
    goal[:] = 0
    goal[0][CORNER_GOAL] = 1
    passable[0, CORNER_H - 3:, CORNER_W - 6:CORNER_W - 1] = 1
    return cost, passable, goal


def corner_window(a):
    """[1,H,W] -> the window [1,24,48]"""
    return np.ascontiguousarray(np.asarray(a)[(slice(None),) + CORNER_WINDOW])


def corner_upstream():
    G = np.zeros((1, CORNER_H, CORNER_W), f32)
    G[0][CORNER_START] = 1
    return G
