"""Scenarios aimed at the seams of the large-map search's two-level open list (csrc/nastar_search_hybrid.hip.h,
csrc/nastar_forward_hybrid_body.inc), and the census that shows from a selection log alone that a scenario reaches them.  numpy only.

Geometry of the kernel: a CHUNK is 64 cells (one ``cmin`` entry), a SUPER-CHUNK 64 chunks = 4,096 cells (one ``smin`` entry); lane ``l`` of the
searching wavefront owns the ``smin`` entries ``[l*spl, (l+1)*spl)``, ``spl = ceil(ceil(ceil(HW/64)/64)/64)`` -- 1 up to 262,144 cells, 5 at the
largest map the library takes (1024x1152).  The fill launch looks at 256 cells per block and 64 blocks per grid-stride trip (16,384 cells).

A scenario is ``(name, cost, start, goal, passable, g_ratio, max_iters)`` with ``[B,H,W]`` fp32 arrays; ``table()`` maps each name to its builder
and to the CONDITIONS its oracle log has to meet (tests/test_hybrid_edges.py checks them on the CPU oracle alone):

  min_steps / status                                  the search's own length and verdict
  min_supers, min_lanes, all_entries                  distinct super-chunks / owner lanes selected; every entry position 0..spl-1 selected
  min_entry_changes                                   consecutive selections in one lane's range but in different entries of it
  min_super_cross                                     in-map neighbours of selected cells in another super-chunk than the selected cell
  min_last_chunk                                      selections in the map's last chunk (the one with padded cells)
  min_coupled_cell                                    lock-step rows: the literal batch loop closes cells of map 0 that its own search leaves alone,
                                                      all of them at or above this flat index
"""
from __future__ import annotations

import functools
from typing import Callable, Dict, NamedTuple, Optional

import numpy as np

f32 = np.float32
CHUNK, SUPER, TRIP = 64, 4096, 16384
MAX_ITERS = 4096  # every scenario but the budget rows: far above any search here (the reference's W*W is 1 on a map one cell wide)


def geometry(H: int, W: int):
    """-> (HW, nchunks, nsuper, spl) as csrc/nastar_capi.hip forward_hybrid computes them"""
    HW = H * W
    nchunks = (HW + 63) // 64
    nsuper = (nchunks + 63) // 64
    return HW, nchunks, nsuper, (nsuper + 63) // 64


class Scenario(NamedTuple):
    name: str
    cost: np.ndarray
    start: np.ndarray
    goal: np.ndarray
    passable: np.ndarray
    g_ratio: float
    max_iters: int


# ---- census of a selection log ------------------------------------------------------------------------------------------------------------
def census(sel_log, iters: int, H: int, W: int) -> dict:
    """what the selections ``sel_log[:iters]`` of one map touch, in the kernel's geometry"""
    HW, nchunks, nsuper, spl = geometry(H, W)
    s = np.asarray(sel_log[:iters], np.int64)
    S = s >> 12
    lane = S // spl
    same_lane = lane[1:] == lane[:-1]
    r, c = s // W, s % W
    cross12 = cross6 = 0
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            inb = (r + dr >= 0) & (r + dr < H) & (c + dc >= 0) & (c + dc < W)
            n = s + dr * W + dc
            cross12 += int((inb & ((n >> 12) != S)).sum())
            cross6 += int((inb & ((n >> 6) != (s >> 6))).sum())
    return {
        "steps": int(iters),
        "supers": int(np.unique(S).size),
        "lanes": int(np.unique(lane).size),
        "entries": sorted(int(x) for x in np.unique(S % spl)),
        "lane_changes": int((~same_lane).sum()),
        "entry_changes": int((same_lane & (S[1:] != S[:-1])).sum()),
        "super_cross": cross12,
        "chunk_cross": cross6,
        "last_chunk": int(((s >> 6) == nchunks - 1).sum()),
    }


def unmet(cond: dict, cen: dict, status: int, H: int, W: int) -> list:
    """the conditions of ``cond`` that census ``cen`` / ``status`` do not meet (empty = the scenario does what it is there for)"""
    spl = geometry(H, W)[3]
    bad = []
    if status != cond.get("status", 0):
        bad.append(f"status {status} != {cond.get('status', 0)}")
    for key, field in (("min_steps", "steps"), ("min_supers", "supers"), ("min_lanes", "lanes"), ("min_entry_changes", "entry_changes"),
                       ("min_super_cross", "super_cross"), ("min_last_chunk", "last_chunk")):
        if key in cond and cen[field] < cond[key]:
            bad.append(f"{field} {cen[field]} < {cond[key]}")
    if cond.get("all_entries") and cen["entries"] != list(range(spl)):
        bad.append(f"entry positions {cen['entries']} of {spl}")
    return bad


# ---- builders -----------------------------------------------------------------------------------------------------------------------------
def _onehot(H, W, *cells):
    m = np.zeros((1, H, W), f32)
    for cell in cells:
        m.reshape(-1)[cell] = 1.0
    return m


def _costs(H, W, seed, lo=0.01, hi=2.0, B=1):
    return np.random.Generator(np.random.PCG64(seed)).uniform(lo, hi, (B, H, W)).astype(f32)


def _ones(H, W):
    return np.ones((1, H, W), f32)


def last_onehot(m):
    """one-hot maps of the HIGHEST non-zero cell of every map: the kernels' contract for start / goal maps that are not one-hot"""
    m = np.asarray(m)
    out = np.zeros_like(m)
    for b in range(m.shape[0]):
        nz = np.flatnonzero(m[b].reshape(-1))
        if nz.size:
            out[b].reshape(-1)[nz[-1]] = 1.0
    return out


def seam(H, W):
    """(row, col) of the first cell of a lane's owned range, 4096 * spl * l, for a lane near the middle of the map whose border cell is not at the
    map's edge (a border that falls on a row's first cell -- W a divisor of 4096 * spl -- is met at the middle column instead)"""
    HW, _, nsuper, spl = geometry(H, W)
    lanes = (nsuper + spl - 1) // spl
    best = None
    for l in range(1, lanes):
        r, c = divmod(SUPER * spl * l, W)
        if r + 40 >= H:
            continue
        mid_col = W // 4 <= c <= 3 * W // 4
        score = (0 if (mid_col or c == 0) else 1, abs(l - lanes / 2.0))
        if best is None or score < best[0]:
            best = (score, r, c if mid_col else W // 2)
    return best[1], best[2]


def ladder(H, W, tie, g_ratio=None, seed=1):
    """start and goal on either side of ``seam(H, W)``: 12 rows and 13 columns apart on the unit-cost map at g_ratio 1 (every step ties across
    the whole frontier, which floods several super-chunks), 28 rows and 21 columns on the random-cost map (a narrow search along the route)"""
    r, c = seam(H, W)
    dr, dc_s, dc_g = (6, 5, 8) if tie else (14, 9, 12)
    if not tie and geometry(H, W)[3] == 1:
        r, dr, dc_s, dc_g = r - 0.5, 0.5, 12, 13  # (two super-chunks, one border: the route runs along it, in the rows on either side)
    s, g = int(r - dr) * W + (c - dc_s), int(r + dr) * W + (c + dc_g)
    kind = "tie" if tie else "rnd"
    if g_ratio is None:
        g_ratio = 1.0 if tie else 0.5
    cost = _ones(H, W) if tie else _costs(H, W, seed + H + W)
    name = f"spl{geometry(H, W)[3]}_{H}x{W}_{kind}" + ("" if g_ratio in (0.5, 1.0) else f"_g{g_ratio:g}")
    return Scenario(name, cost, _onehot(H, W, s), _onehot(H, W, g), _ones(H, W), g_ratio, MAX_ITERS)


def thin(H, W, goal_last):
    """start and goal 24 cells apart at one end of a map of at most three columns (or one row): the far end is where (i + 0.5) * fl(1 / W) is furthest off"""
    HW = H * W
    goal = HW - 1 if goal_last else 0
    step = 24 * (W if W <= 3 else 1)  # 24 rows of a narrow map, 24 cells of a single row
    start = goal - step if goal_last else step
    name = f"thin_{H}x{W}_{'far' if goal_last else 'near'}"
    return Scenario(name, _costs(H, W, 7 + (HW % 1000) + goal_last), _onehot(H, W, start), _onehot(H, W, goal), _ones(H, W), 0.5, MAX_ITERS)


def padded(H, W, tie, swap):
    """start on the map's last cell, the goal 20 (random costs: 28) columns to its left in the last row: both in the last chunk, next to its padded cells"""
    a, b = H * W - 1, H * W - (21 if tie else 29)
    if swap:
        a, b = b, a
    name = f"pad_{H}x{W}_{'tie' if tie else 'rnd'}{'_swap' if swap else ''}"
    cost = _ones(H, W) if tie else _costs(H, W, 3 * H + W)
    if not tie:
        cost[0, H - 1, :] *= f32(0.25)  # (a cheap last row: the search stays in it, that is, in the last chunk)
    return Scenario(name, cost, _onehot(H, W, a), _onehot(H, W, b), _ones(H, W), 1.0 if tie else 0.5, MAX_ITERS)


def walled(H=513, W=512):
    """the start in a 12x30 room across the border of super-chunks 31 | 32 (row 256: lanes 15 | 16), closed by a ring of obstacles; the goal outside"""
    p = _ones(H, W)
    p[0, 249:263, 239:271] = 0.0
    p[0, 250:262, 240:270] = 1.0
    return Scenario(f"wall_{H}x{W}", _costs(H, W, 21), _onehot(H, W, 255 * W + 250), _onehot(H, W, 300 * W + 300), p, 0.5, MAX_ITERS)


def budget(max_iters):
    sc = ladder(513, 512, True)
    return sc._replace(name=f"budget_{max_iters}", max_iters=int(max_iters))


def lockstep(g_ratio, H=90, W=91, goal_cell=4106):
    """B = 2.  Map 0: a goal that costs 10 in the first chunk of super-chunk 1, everything at or above its row an obstacle but a 2x3 room that
    holds the start: the goal is reached in a few steps, and its expansion opens cheaper cells below it -- the reference's batch loop goes on
    closing them (all in super-chunk 1) while map 1 searches from (5,5) to (85,85)."""
    gr, gc = divmod(goal_cell, W)
    cost = _costs(H, W, 5, 0.0, 1.0, B=2)
    cost[0, gr, gc] = 10.0
    p = np.ones((2, H, W), f32)
    p[0, :gr + 1, :] = 0.0
    p[0, gr, gc] = 1.0
    p[0, gr - 2:gr, gc - 1:gc + 2] = 1.0
    start = np.concatenate([_onehot(H, W, (gr - 2) * W + gc), _onehot(H, W, 5 * W + 5)])
    goal = np.concatenate([_onehot(H, W, goal_cell), _onehot(H, W, 85 * W + 85)])
    return Scenario(f"lock_g{g_ratio:g}", cost, start, goal, p, g_ratio, W * W)


def not_one_hot(far):
    """the spl 2 random-cost map with a decoy start and a decoy goal at LOWER indices: `far` False -- 300 / 600 cells below (another 256-cell block
    of the same grid-stride trip of the fill launch); True -- 16,384 (the same thread, one trip earlier) / 20,000 cells below (another thread
    and trip).  The highest non-zero cell wins."""
    sc = ladder(513, 512, False)
    H, W = sc.cost.shape[1:]
    s, g = int(np.flatnonzero(sc.start)[0]), int(np.flatnonzero(sc.goal)[0])
    ds, dg = (TRIP, 20000) if far else (300, 600)
    assert (s // TRIP == (s - ds) // TRIP) != far and (g // TRIP == (g - dg) // TRIP) != far and s // 256 != (s - ds) // 256
    return sc._replace(name=f"multihot_{'far' if far else 'near'}", start=_onehot(H, W, s - ds, s), goal=_onehot(H, W, g - dg, g))


def swapped(sc: Scenario) -> Scenario:
    """the same maps searched the other way round: a second, distinct map of the scenario's shape, g_ratio and budget"""
    return sc._replace(name=sc.name + "~", start=sc.goal, goal=sc.start)


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
class Row(NamedTuple):
    build: Callable[[], Scenario]
    cond: dict
    lock: bool = False  # checked against the oracle's literal batch loop (mode="dense"), not only the state machine


LADDER_SHAPES = [(90, 91), (513, 512), (512, 514), (700, 1100), (1024, 1024), (1024, 1152)]  # spl 1, 2 (fast division), 2 (IEEE), 3, 4, 5
THIN_SHAPES = [(393216, 3), (589824, 2), (1179648, 1), (1, 1179648), (6400, 1), (1, 6400)]
PAD_SHAPES = [(81, 81), (83, 79)]  # 33 / 29 real cells in the last chunk; 83x79: HW % 4 != 0
SPL_COND = {"min_lanes": 2, "all_entries": True, "min_entry_changes": 1, "min_super_cross": 10}
SPL1_COND = {"min_supers": 2, "min_super_cross": 10}


@functools.lru_cache(maxsize=None)
def table() -> Dict[str, Row]:
    t: Dict[str, Row] = {}
    for H, W in LADDER_SHAPES:
        spl = geometry(H, W)[3]
        base = SPL1_COND if spl == 1 else SPL_COND
        t[f"spl{spl}_{H}x{W}_tie"] = Row(functools.partial(ladder, H, W, True), {**base, "min_steps": 100})
        t[f"spl{spl}_{H}x{W}_rnd"] = Row(functools.partial(ladder, H, W, False), dict(base))
    t["spl5_1024x1152_rnd_g0"] = Row(functools.partial(ladder, 1024, 1152, False, 0.0), {"min_supers": 2, "min_super_cross": 10})
    for H, W in THIN_SHAPES:
        for goal_last in (True, False):
            t[f"thin_{H}x{W}_{'far' if goal_last else 'near'}"] = Row(functools.partial(thin, H, W, goal_last), {"min_steps": 5})
    for H, W in PAD_SHAPES:
        for tie in (False, True):
            for swap in (False, True):
                t[f"pad_{H}x{W}_{'tie' if tie else 'rnd'}{'_swap' if swap else ''}"] = Row(functools.partial(padded, H, W, tie, swap), {"min_last_chunk": 10})
    t["wall_513x512"] = Row(walled, {"status": 3, "min_supers": 2, "min_steps": 200})
    for g in (0.2, 0.0):
        t[f"lock_g{g:g}"] = Row(functools.partial(lockstep, g), {"min_coupled_cell": SUPER}, lock=True)
    for far in (False, True):
        t[f"multihot_{'far' if far else 'near'}"] = Row(functools.partial(not_one_hot, far), {"min_steps": 5})
    return t


BUDGETS = (31, 32, 33, "steps-1")  # of the spl 2 tie scenario; "steps-1": the oracle's step count of the whole search, less one


def build(name: str, steps_of: Optional[Callable[[str], int]] = None) -> Scenario:
    """the scenario `name` of ``table()``, or a budget row ``budget_<n>`` / ``budget_steps-1`` (``steps_of(name)``: the oracle's step count)"""
    if name.endswith("~"):
        return swapped(build(name[:-1], steps_of))
    if name.startswith("budget_"):
        n = name[len("budget_"):]
        if n == "steps-1":
            return budget(steps_of("spl2_513x512_tie") - 1)._replace(name=name)
        return budget(int(n))
    return table()[name].build()
