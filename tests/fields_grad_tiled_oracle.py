"""The TILED subtree sum of include/nastar_fields_grad_tiled.h in plain Python floats (IEEE binary64): the
scheme the kernels follow, with the freedom the hardware has made explicit -- the tiles of a round run in a random order, and every halo word
a tile reads is, at random, either what it holds NOW (another tile of this round may already have rewritten it) or what it held when the
round BEGAN (stale).  The tile size is a parameter.  The claim under test is that none of this changes a bit: ``tiled_grad`` ==
``in_order``, the untiled evaluation in which every cell is computed once, after its children, as G(v) + A(c_0) + A(c_1) + ... with the
children in the row-major order of their position relative to v -- the bit-level reference of the kernels.

Why the claim holds (restated from DESIGN 6h).  SAME BITS IN ANY ORDER: a cell is a pure function of its children's values and the forest has
no cycle (a successor has a strictly smaller dist), so there is ONE fixed point.  A tile that read a stale halo word has been marked by the
tile that wrote it; a state with no tile marked is therefore that fixed point, whatever intermediate values raced past.  The values are NOT
monotone (G has both signs), unlike item 6f: the argument is uniqueness, not bounds.  TERMINATION: take the non-final cell of smallest
height.  All its children are final.  If they lie in its tile, the local fixed point settles it in this round; if one lies in another
tile, that tile marked this one when it last wrote it.  So every round with an active tile makes at least one more cell final: H*W + 1
rounds bound the count, whatever the input.
"""
import os
import struct
import sys
from typing import NamedTuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fields_oracle as FO  # noqa: E402
from heuristic_oracle import MOORE8, offsets  # noqa: E402

f32 = np.float32
STATUS_OK, STATUS_NO_CONVERGENCE, STATUS_PLATEAU = 0, 10, 11
CHILD_ORDER = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))  # row-major, relative to the parent


class Forest(NamedTuple):
    live: np.ndarray      # [H,W] bool
    succ: np.ndarray      # [H*W] flat index of s(n) on live cells, -1 elsewhere and on a live cell without a successor
    kids: list            # per flat index: the children's flat indices in CHILD_ORDER
    order: np.ndarray     # the live cells in decreasing dist: a child before its parent
    plateau: bool


def forest(dist, goal, passable, mask=MOORE8) -> Forest:
    """the policy forest from dist, goal and passable alone, by the header's words: the successor is the FIRST action, in ACTION_MOVES order,
    among the allowed moves whose target has the smallest READABLE value, taken only if that value is strictly below dist[n]"""
    d = np.asarray(dist, f32)
    H, W = d.shape
    live = (np.asarray(goal) == 0) & (d < np.inf)
    readable = np.where(np.asarray(passable) != 0, d, f32(np.inf)).astype(f32)
    allowed = set(offsets(mask))
    best = np.full((H, W), np.inf, f32)
    act = np.full((H, W), -1, np.int64)
    for k, (dy, dx) in enumerate(FO.ACTION_MOVES):
        if (dy, dx) not in allowed:
            continue
        v = FO._shifted(readable, dy, dx)
        better = v < best
        best, act = np.where(better, v, best), np.where(better, k, act)
    act = np.where(live & (best < d), act, -1)
    succ = np.full(H * W, -1, np.int64)
    kids = [[] for _ in range(H * W)]
    ys, xs = np.nonzero(act >= 0)
    for y, x in zip(ys.tolist(), xs.tolist()):
        dy, dx = FO.ACTION_MOVES[act[y, x]]
        succ[y * W + x] = (y + dy) * W + (x + dx)
    for y, x in zip(*(a.tolist() for a in np.nonzero(live))):   # the children of a LIVE cell (a goal is nobody's parent)
        for dy, dx in CHILD_ORDER:
            cy, cx = y + dy, x + dx
            if 0 <= cy < H and 0 <= cx < W and succ[cy * W + cx] == y * W + x:
                kids[y * W + x].append(cy * W + cx)
    flat = d.reshape(-1)
    order = np.argsort(-flat, kind="stable")
    order = order[live.reshape(-1)[order]]
    return Forest(live, succ, kids, order, bool((live.reshape(-1) & (succ < 0)).any()))


def _bits(x: float) -> bytes:
    return struct.pack("<d", x)


def in_order(dist, goal, passable, G, mask=MOORE8):
    """[H,W] arrays -> (A [H,W] f64, grad [H,W] f32, status): every live cell once, after its children, the children in CHILD_ORDER"""
    F = forest(dist, goal, passable, mask)
    H, W = F.live.shape
    if F.plateau:
        return np.zeros((H, W)), np.zeros((H, W), f32), STATUS_PLATEAU
    g = np.asarray(G, f32).reshape(-1).astype(np.float64).tolist()
    A = [0.0] * (H * W)
    for n in F.order.tolist():
        v = g[n]
        for c in F.kids[n]:
            v += A[c]
        A[n] = v
    A = np.array(A).reshape(H, W)
    return A, np.where(F.live, A, 0.0).astype(f32), STATUS_OK


def tiled_grad(dist, goal, passable, G, mask=MOORE8, tile=(64, 64), rng=None, max_rounds=None, mark="successor"):
    """[H,W] arrays -> (A [H,W] f64, grad [H,W] f32, status, rounds, tile visits).  ``rng``: None = every halo read fresh, tiles in index
    order; a numpy Generator = random order, every halo WORD fresh or one round stale at random.  ``mark``: "successor" marks the tile that
    holds the successor of a changed cell (the kernels' rule); "none" marks nobody -- the WRONG rule, kept to show that the tests see it."""
    F = forest(dist, goal, passable, mask)
    H, W = F.live.shape
    th, tw = tile
    ty, tx = -(-H // th), -(-W // tw)
    zeros = (np.zeros((H, W)), np.zeros((H, W), f32))
    if F.plateau:
        return zeros + (STATUS_PLATEAU, 0, 0)
    tile_of = lambda n: ((n // W) // th) * tx + (n % W) // tw  # noqa: E731
    g = np.asarray(G, f32).reshape(-1).astype(np.float64).tolist()
    live = F.live.reshape(-1)
    A = [g[n] if live[n] else 0.0 for n in range(H * W)]          # init: A = G on live cells
    work = [[] for _ in range(ty * tx)]                            # per tile: its cells that have a child, a child before its parent
    halo = [set() for _ in range(ty * tx)]                         # per tile: the children that live in another tile
    active = [False] * (ty * tx)
    for n in F.order.tolist():
        t = tile_of(n)
        active[t] = True                                           # init: a tile that holds a live cell starts active
        if F.kids[n]:
            work[t].append(n)
            halo[t].update(c for c in F.kids[n] if tile_of(c) != t)
    bound = H * W + 1
    limit = bound if max_rounds is None else min(max_rounds, bound)
    rounds = visits = 0
    while any(active) and rounds < limit:
        rounds += 1
        old = A[:]                                                 # what every word held when the round began
        nxt = [False] * (ty * tx)
        todo = [t for t in range(ty * tx) if active[t]]
        if rng is not None:
            rng.shuffle(todo)
        for t in todo:
            visits += 1
            loc = A[:]                                             # the tile's LDS copy
            if rng is not None:
                for c in halo[t]:
                    if rng.random() < 0.5:
                        loc[c] = old[c]
            for n in work[t]:                                      # the local fixed point, the halo fixed
                v = g[n]
                for c in F.kids[n]:
                    v += loc[c]
                loc[n] = v
            for n in work[t]:                                      # store what changed; mark the tile that reads it
                if _bits(loc[n]) != _bits(A[n]):
                    A[n] = loc[n]
                    s = tile_of(int(F.succ[n]))
                    if s != t and mark == "successor":
                        nxt[s] = True
        active = nxt
    if any(active):
        return zeros + (STATUS_NO_CONVERGENCE, rounds, visits)
    A = np.array(A).reshape(H, W)
    return A, np.where(F.live, A, 0.0).astype(f32), STATUS_OK, rounds, visits
