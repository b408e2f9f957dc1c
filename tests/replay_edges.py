"""Degenerate and batch-coupled problems for the replay backward (nastar_backward_replay*): the problems, the oracle's answers and the bars
that tests/test_replay_edges.py (CPU: the oracle alone) and tests/test_replay_edges_gpu.py (the kernels) share.  No test functions here.

The batch is the three-map one of tests/test_edge_cases_gpu.py -- start == goal, start next to the goal, a far goal -- so the two short
maps get ALL of their gradient from the `extra = t_batch - tau` copies of the fixed-point term (csrc/nastar_backward_replay.hip.h): run
alone their gradient is exactly zero.  Every shape is paired with the replay route it must reach (csrc/nastar_capi.hip
backward_replay_impl; tools/fuzz_parity.replay_route names the compiled ones, "asm" is the hand-scheduled 32x32 / 16x16 loop).

PER-MAP RELATIVE ERROR, measured on an MI355X: the largest max|got_b - ref_b| / max|ref_b| per route over everything
tests/test_replay_edges_gpu.py runs (every shape x variant through the C ABI, the t_batch, placement, fused-L1 and module tests; maps with
max|ref_b| >= 1e-3 only), and where it was met.  rel_bar() asserts 4 x these figures, never more than 1e-5:

    asm                        2.213e-07   16x16 T3, map 2
    replay_lds_hist_fastdiv    3.242e-07   20x45 T3, map 2
    replay_lds_hist_ieee       2.208e-07   33x31 3xmap_g0, map 0
    replay_lds_state_fastdiv   2.060e-07   64x64 u01, map 2
    replay_lds_state_ieee      2.835e-07   60x66 3xmap_g0, map 2
    replay_hbm16_fastdiv       2.097e-07   112x128 Tgoal, map 2
    replay_hbm16_ieee          2.451e-07   110x110 3xmap_g0, map 1
    replay_hbm32_fastdiv       1.825e-07   257x256 Tgoal-1, map 0
    replay_hbm32_ieee          1.480e-07   256x257 3xmap_g0, map 1

(Before the start cell took stamp 1 in the compiled loops -- csrc/nastar_backward_replay_body.inc -- replay_lds_hist_fastdiv measured
5.306e-07 on the 2x2 T3 batch, most of it step 0's fp32 noise on the start cell; every other route measured the same figure.)  For scale:
rounding the float64 reference to fp32 alone is up to 6e-08, the project has measured 5.5e-07 to 2.2e-06 on ordinary cases.
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "neural-astar_amd"), ROOT):
    if _p not in sys.path:
        sys.path.append(_p)

GRAD_TOL = 1e-5      # the project's bar: max|got - ref| <= GRAD_TOL * max(1, max|ref|) -- applied per map here
REL_FLOOR = 1e-3     # maps whose max|ref_b| is at least this also meet the relative bar of their route
# route -> the largest per-map relative error measured on the device (the table of the module docstring)
MEASURED_REL = {"asm": 2.213e-07, "replay_lds_hist_fastdiv": 3.242e-07, "replay_lds_hist_ieee": 2.208e-07, "replay_lds_state_fastdiv": 2.060e-07,
                "replay_lds_state_ieee": 2.835e-07, "replay_hbm16_fastdiv": 2.097e-07, "replay_hbm16_ieee": 2.451e-07,
                "replay_hbm32_fastdiv": 1.825e-07, "replay_hbm32_ieee": 1.480e-07}
REL_CAP = 1e-5


def rel_bar(route):
    """the asserted per-map relative bar of `route`: 4 x the measured value (the order of the fp32 atomic adds and v_exp_f32 may differ
    between runs and boxes), never above 1e-5"""
    return min(4.0 * MEASURED_REL[route], REL_CAP)


def problems(H, W, seed, reach=None, p=0.15):
    """-> (maps, starts, goals), each [3, 1, H, W] float32.  map 0: start == goal at the middle cell; map 1: start (0, 0), goal
    (min(1, H-1), min(1, W-1)); map 2: start (0, 0), goal at the opposite corner, or at (min(reach, H-1), min(reach, W-1)).  Obstacles
    with probability `p` (one-row and one-column maps: none -- an obstacle there cuts the corner map in two, and the oracle's backward
    returns rc 3 for an unsolvable map); start and goal cells are free."""
    rng = np.random.default_rng(seed)
    if H == 1 or W == 1:
        p = 0.0
    m = (rng.random((3, 1, H, W)) > p).astype(np.float32)
    s, g = np.zeros_like(m), np.zeros_like(m)
    mid = (H // 2, W // 2)
    adj = (min(1, H - 1), min(1, W - 1))
    far = (H - 1, W - 1) if reach is None else (min(reach, H - 1), min(reach, W - 1))
    s[0, 0][mid] = 1; g[0, 0][mid] = 1; m[0, 0][mid] = 1
    s[1, 0, 0, 0] = 1; g[1, 0][adj] = 1; m[1, 0, 0, 0] = 1; m[1, 0][adj] = 1
    s[2, 0, 0, 0] = 1; g[2, 0][far] = 1; m[2, 0, 0, 0] = 1; m[2, 0][far] = 1
    return m, s, g


def opened_superset(sel_log, iters, start, passable):
    """bool [B, H, W]: the start cell, or a passable Moore neighbour of any of the first iters[b] logged selections -- every cell the
    search can have opened.  The oracle's gradient is exactly 0.0 outside it."""
    passable = np.asarray(passable).reshape((len(iters),) + np.asarray(passable).shape[-2:])
    B, H, W = passable.shape
    out = np.asarray(start).reshape(B, H, W) > 0
    for b in range(B):
        sel = np.zeros((H + 2, W + 2), bool)
        cells = np.asarray(sel_log[b, :iters[b]], np.int64)
        sel[cells // W + 1, cells % W + 1] = True
        near = np.zeros((H, W), bool)
        for dr in (0, 1, 2):
            for dc in (0, 1, 2):
                if (dr, dc) != (1, 1):
                    near |= sel[dr:dr + H, dc:dc + W]
        out[b] |= near & (passable[b] > 0)
    return out


# name -> (cost kind, g_ratio, budget).  budget: None = the eval budget W * W; an int; "goal" = iters[2] of the u01 search at the eval
# budget (the far goal is selected on the LAST step of the budget); "goal-1" = one step less (the budget ends one step before the far goal:
# no fixed-point term for that map), at least 1.
VARIANTS = {
    "u01": ("u01", 0.5, None),
    "zeros": ("zeros", 0.2, None),         # every priority ties in g: the first-index rule decides
    "3xmap_g0": ("3xmap", 0.0, None),      # best-first: kfac = -1 / sqrt(W), the largest
    "u01_g1": ("u01", 1.0, None),          # kfac = 0: the gradient is exactly zero everywhere
    "T1": ("u01", 0.5, 1),                 # only the start is selected: exactly zero everywhere
    "T3": ("u01", 0.5, 3),
    "Tgoal": ("u01", 0.5, "goal"),
    "Tgoal-1": ("u01", 0.5, "goal-1"),
}
EXACTLY_ZERO = ("u01_g1", "T1")

# id -> (H, W, reach, cost 4 bytes past a 16-byte boundary, the route at the eval budget)
SHAPES = {
    "32x32": (32, 32, None, False, "asm"),
    "16x16": (16, 16, None, False, "asm"),
    "32x32+4B": (32, 32, None, True, "replay_lds_hist_fastdiv"),
    "33x31": (33, 31, None, False, "replay_lds_hist_ieee"),
    "20x45": (20, 45, None, False, "replay_lds_hist_fastdiv"),
    "64x64": (64, 64, None, False, "replay_lds_state_fastdiv"),
    "60x66": (60, 66, None, False, "replay_lds_state_ieee"),
    "110x110": (110, 110, 24, False, "replay_hbm16_ieee"),
    "112x128": (112, 128, 24, False, "replay_hbm16_fastdiv"),
    "256x257": (256, 257, 24, False, "replay_hbm32_ieee"),
    "257x256": (257, 256, 24, False, "replay_hbm32_fastdiv"),
    "1x40": (1, 40, None, False, "replay_lds_hist_fastdiv"),
    "40x1": (40, 1, None, False, "replay_lds_hist_fastdiv"),   # (the budget W * W is ONE step there)
    "2x2": (2, 2, None, False, "replay_lds_hist_fastdiv"),
    "1x1": (1, 1, None, False, "replay_lds_hist_fastdiv"),
}


def route(shape, max_iters):
    """the replay route of `shape` at this budget: backward_replay_impl takes the hand-scheduled loop for aligned 32x32 / 16x16 batches at
    any budget; everything else is what tools/fuzz_parity.replay_route says (a short budget moves the step history into LDS)"""
    from fuzz_parity import replay_route
    H, W, _, misaligned, at_eval = SHAPES[shape]
    return "asm" if at_eval == "asm" and not misaligned else replay_route(H, W, max_iters)


def _seed(shape):
    H, W = SHAPES[shape][:2]
    return 100 * H + W


@functools.lru_cache(maxsize=None)
def batch(shape):
    H, W, reach = SHAPES[shape][:3]
    pr = problems(H, W, _seed(shape), reach)
    for a in pr:
        a.setflags(write=False)
    return pr


def _cost(kind, m, seed):
    if kind == "zeros":
        return np.zeros_like(m)
    if kind == "3xmap":
        return (m * 3).astype(np.float32)
    return np.random.default_rng(seed + 1).random(m.shape, dtype=np.float32)


def budget(shape, variant):
    W = SHAPES[shape][1]
    T = VARIANTS[variant][2]
    if T is None:
        return W * W
    if isinstance(T, int):
        return T
    far = int(case(shape, "u01").fwd.iters[2])
    return far if T == "goal" else max(1, far - 1)


@functools.lru_cache(maxsize=None)
def case(shape, variant):
    """one batch with the oracle's answers, computed once, shared by every test and never modified: m, s, g, cost, up [3,1,H,W]; gr, T;
    fwd = oracle.forward(mode="sm") with its selection log; ref = oracle.backward(up, ...) [3,H,W]; opened = opened_superset(...);
    route = the replay route this case must take"""
    from oracle import oracle as O
    m, s, g = batch(shape)
    kind, gr, _ = VARIANTS[variant]
    T = budget(shape, variant)
    cost = _cost(kind, m, _seed(shape))
    up = np.random.default_rng(_seed(shape) + 2).standard_normal(m.shape).astype(np.float32)
    fwd = O.forward(cost, s, g, m, gr, T, mode="sm", want_log=True)
    ref = O.backward(up, cost, s, g, m, gr, T)
    opened = opened_superset(fwd.sel_log, fwd.iters, s, m)
    for a in (cost, up, ref, opened, fwd.histories, fwd.paths, fwd.iters, fwd.sel_log):
        a.setflags(write=False)
    return SimpleNamespace(shape=shape, variant=variant, H=m.shape[2], W=m.shape[3], m=m, s=s, g=g, cost=cost, up=up, gr=gr, T=T, fwd=fwd,
                           ref=ref, opened=opened, route=route(shape, T), misaligned=SHAPES[shape][3])


def alone(c):
    """the oracle's gradient of every map of case `c` as a batch of its own, concatenated: no map waits for another, so no `extra` copies"""
    from oracle import oracle as O
    return np.concatenate([O.backward(c.up[b:b + 1], c.cost[b:b + 1], c.s[b:b + 1], c.g[b:b + 1], c.m[b:b + 1], c.gr, c.T) for b in range(3)])


def per_map_errors(got, ref):
    """-> (abs error, max|ref|) per map"""
    B = ref.shape[0]
    return np.abs(got - ref).reshape(B, -1).max(1), np.abs(ref).reshape(B, -1).max(1)


def check_grad(got, ref, opened, route_name, what, measured=None):
    """the assertions every gradient of these tests meets: no NaN, exactly 0.0 outside the opened cells, the project's bar per map, and the
    route's relative bar on maps with a gradient of at least REL_FLOOR.  `measured`: a list that receives (route, what, map, relative error)"""
    assert not np.isnan(got).any(), f"{what}: NaN in the gradient (a cell was not written)"
    stray = np.argwhere((got != 0) & ~opened)
    assert stray.size == 0, f"{what}: non-zero gradient outside the opened cells at (map, row, col) {stray[:8].tolist()}"
    err, scale = per_map_errors(got, ref)
    for b in range(ref.shape[0]):
        print(f"replay_edges {what} route={route_name} map={b} err={err[b]:.3e} scale={scale[b]:.3e}")
        assert err[b] <= GRAD_TOL * max(1.0, scale[b]), f"{what}: map {b} err {err[b]:.3e} at scale {scale[b]:.3e}"
        if scale[b] >= REL_FLOOR:
            rel = err[b] / scale[b]
            if measured is not None:
                measured.append((route_name, what, b, float(rel)))
            assert rel <= rel_bar(route_name), f"{what}: map {b} relative error {rel:.3e} above the {route_name} bar {rel_bar(route_name):.3e}"
