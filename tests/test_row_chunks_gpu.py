"""GPU tests (-m gpu) of the row-wide chunks of the hand-scheduled 32x32 search kernels (csrc/nastar_search_asm.hip.h: AsmLayout::CCL, ROWS).

At 32x32 a chunk minimum covers a whole map ROW: 32 minima in lanes 0-31, two DPP rows.  The selection ends after its row stages with one
v_readlane per DPP row (map rows 0-15 and 16-31) and one scalar minimum; the chunk lanes are lanes 32-63, cell (s* & ~31) | (lane & 31).  At
16x16 the 16 minima sit in one DPP row and one v_readlane finishes; 64x64 keeps its code.  What can go wrong, and the case that shows it:

1. a missing or wrong second v_readlane -- every open cell in map rows 0-15, and every open cell in rows 16-31 (a wall keeps the search there);
2. the tie-break across rows -- maps that are symmetric about the line from start to goal hold the SAME minimal key in several rows at once
   (checked here on the CPU from the oracle's selection log before the case is relied on: obstacle-free maps alone never tie, the Euclidean
   term of the heuristic tells their cells apart), and the lowest cell index must win; the obstacle-free maps of the issue run as well;
3. the empty open list -- an enclosed start: lane 0's idle entry must leave through the goal exit, status unsolvable, whichever half holds the goal;
4. the start on an obstacle, the start equal to the goal;
5. mazes through every stream: stored heuristic at g_ratio 0.5 and 0.3 / 0.8, U(0, 1) costs (general stream), costs in [-2, 1) (signed
   stream), and budgets of 7 and 40 steps (the budget exit);
6. the same at 16x16; 7. one 64x64 map.

Every case runs through the plain kernel with the selection log, the plain kernel without it and the ranked kernel (the one bench.py times),
and is compared bit for bit with the CPU oracle: histories, paths, iters, status, and the selection log where the launch returns one.
"""
import numpy as np
import pytest
import torch

from test_stored_heuristic_gpu import _Out, _dev, _stream, _t

pytestmark = pytest.mark.gpu


# ---- one launch through the C ABI ---------------------------------------------------------------------------------------------------------------
def _launch(cost, s, g, passable, *, which, g_ratio, max_iters, log):
    """cost / passable [B, W, W]; passable None: ONE tensor is cost map and obstacle map (the stored-heuristic stream, VanillaAstar's call)"""
    from neural_astar import _native, ops
    lib = _native.load()
    B, H, W = cost.shape
    HW = H * W
    ct, st, gt = _t(cost), _t(s), _t(g)
    pt = ct if passable is None else _t(passable)
    outs = {"histories": _Out(B * HW, torch.float32, -3.0), "paths": _Out(B * HW, torch.int64, -3), "iters": _Out(B, torch.int32, -3),
            "status": _Out(B, torch.int32, -3), "packed": _Out(B * 2 * ((HW + 7) // 8), torch.uint8, 0xA5),
            "summary": _Out(ops.SUMMARY_WORDS, torch.int32, 0)}
    if log:
        outs["sel_log"] = _Out(B * max_iters, torch.int32, -3)
    counter = torch.zeros(65, dtype=torch.int32, device=_dev())
    head = (ct.data_ptr(), st.data_ptr(), gt.data_ptr(), pt.data_ptr(), B, H, W, float(g_ratio), int(max_iters), outs["histories"].ptr(),
            outs["paths"].ptr(), outs["sel_log"].ptr() if log else None, outs["iters"].ptr(), outs["status"].ptr(), outs["packed"].ptr(), None, 0, 0)
    tail = (outs["summary"].ptr(), counter.data_ptr())
    if which == "levels":
        levels = _t(np.random.default_rng(B).integers(0, 40, B).astype(np.int32))
        rc = lib.nastar_forward_levels(*head, levels.data_ptr(), *tail, _stream())
    else:
        rc = lib.nastar_forward_ex(*head, None, None, *tail, _stream())
    assert rc == 0, (which, rc, lib.nastar_last_error())
    torch.cuda.synchronize()
    return {k: o.take(k) for k, o in outs.items()}


def _check(what, cost, s, g, passable=None, g_ratio=0.5, max_iters=None):
    """the three launches against the oracle -> (oracle output, status of the logging launch)"""
    from oracle import oracle as O
    B, H, W = cost.shape
    T = H * W if max_iters is None else max_iters
    o = O.forward(cost, s, g, cost if passable is None else passable, g_ratio, T, mode="sm", want_log=True)
    status = None
    for which, log in (("ex", True), ("ex", False), ("levels", False)):
        got = _launch(cost, s, g, passable, which=which, g_ratio=g_ratio, max_iters=T, log=log)
        tag = (what, which, log)
        assert np.array_equal(got["iters"], o.iters), (tag, got["iters"].tolist(), o.iters.tolist())
        assert np.array_equal(got["status"], o.map_status), (tag, got["status"].tolist(), o.map_status.tolist())
        assert np.array_equal(got["histories"].reshape(B, H, W), o.histories), tag
        assert np.array_equal(got["paths"].reshape(B, H, W), o.paths), tag
        if log:
            sel = got["sel_log"].reshape(B, T)
            for b in range(B):
                assert np.array_equal(sel[b, :o.iters[b]], o.sel_log[b, :o.iters[b]]), (tag, b)
            status = got["status"]
    return o, status


def _problem(cases, W):
    """[(map, (r, c) start, (r, c) goal)] -> maps, starts, goals [B, W, W] float32"""
    B = len(cases)
    m = np.empty((B, W, W), np.float32)
    s = np.zeros((B, W, W), np.float32)
    g = np.zeros((B, W, W), np.float32)
    for b, (mm, a, z) in enumerate(cases):
        m[b] = mm
        s[b][a] = 1
        g[b][z] = 1
    return m, s, g


def _rand_map(rng, W, *keep, p=0.2):
    m = (rng.random((W, W)) > p).astype(np.float32)
    for q in keep:
        m[q] = 1
    return m


# ---- 1. every open cell in one half of the map rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", ["rows0-15", "rows16-31"])
def test_open_cells_in_one_half_of_the_rows(half):
    W = 32
    rng = np.random.default_rng(11)
    lo = 0 if half == "rows0-15" else 16
    wall = 16 if half == "rows0-15" else 15  # a full row of obstacles: nothing beyond it is ever opened
    cases = []
    for a, z in (((lo, 0), (lo + 15, 31)), ((lo + 15, 3), (lo, 28)), ((lo + 7, 31), (lo + 8, 0)), ((lo + 15, 15), (lo + 15, 16)), ((lo, 31), (lo + 14, 1))):
        m = _rand_map(rng, W, a, z)
        m[wall, :] = 0
        cases.append((m, a, z))
    m = np.ones((W, W), np.float32)
    m[wall, :] = 0
    cases.append((m, (lo + 15, 0), (lo, 31)))
    cases.append((m, (lo, 16), (lo + 15, 16)))
    cost, s, g = _problem(cases, W)
    o, _ = _check(half, cost, s, g)
    closed_rows = np.flatnonzero(o.histories.sum(axis=(0, 2)))
    assert closed_rows.min() >= lo and closed_rows.max() < lo + 16  # the walls did confine the searches
    assert (o.map_status == 0).sum() >= 4


# ---- 2. equal minimal keys in several rows ----------------------------------------------------------------------------------------------------------
def _cross_row_ties(m, si, gi, log, iters):
    """replays one 32x32 unit-cost search at g_ratio 0.5 from its selection log (the arithmetic of reference differentiable_astar.py:206-207 in
    fp32) -> the number of steps at which open cells of MORE THAN ONE ROW hold the minimal key; asserts that every logged selection is the
    lowest cell index among them"""
    from oracle import oracle as O
    W = m.shape[0]
    h0 = O.heuristic(W, W, gi // W, gi % W).reshape(-1).astype(np.float32)
    flat = m.reshape(-1)
    gv = np.full(W * W, np.inf, np.float32)
    opn = np.zeros(W * W, bool)
    closed = np.zeros(W * W, bool)
    gv[si] = 0
    opn[si] = True
    root = np.float32(np.sqrt(np.float32(W)))
    count = 0
    for t in range(iters):
        f = np.float32(0.5) * gv + np.float32(0.5) * (h0 + np.float32(1.0))
        q = (f / root).astype(np.float32)
        q[~opn] = np.inf
        tie = np.flatnonzero(q == q.min())
        sel = int(log[t])
        assert sel == tie[0], (t, sel, tie[:4].tolist())
        count += len(set((tie // W).tolist())) > 1
        if sel == gi:
            break
        opn[sel] = False
        closed[sel] = True
        r, c = divmod(sel, W)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                rr, cc = r + dr, c + dc
                n = rr * W + cc
                if (dr or dc) and 0 <= rr < W and 0 <= cc < W and flat[n] != 0 and not closed[n] and (not opn[n] or gv[n] > gv[sel] + 1):
                    gv[n] = gv[sel] + np.float32(1)
                    opn[n] = True
    return count


def test_equal_minimal_keys_in_several_rows():
    W = 32
    ones = np.ones((W, W), np.float32)
    bar_v = ones.copy()  # a bar across the straight line between start and goal: the ways round it above and below mirror each other
    bar_v[10:23, 16] = 0
    block = ones.copy()  # a block on the diagonal: cell (a, b) mirrors cell (b, a)
    block[10:21, 10:21] = 0
    block2 = ones.copy()
    block2[11:21, 11:21] = 0
    bar_h = ones.copy()  # the mirror images share their rows: ties inside one chunk
    bar_h[16, 10:23] = 0
    sym = [(bar_v, (16, 2), (16, 29)), (bar_v, (16, 29), (16, 2)), (block, (0, 0), (31, 31)), (block, (31, 31), (0, 0)),
           (block2, (31, 0), (0, 31)), (bar_h, (2, 16), (29, 16))]
    # the obstacle-free maps: the goal in each corner and at the centre, the start at several cells
    free = [(ones, a, z) for z in ((0, 0), (0, 31), (31, 0), (31, 31), (16, 16)) for a in ((5, 20), (20, 5), (12, 12), (30, 2), (16, 0), (0, 16))]
    cost, s, g = _problem(sym + free, W)
    o, status = _check("ties", cost, s, g)
    assert (status == 0).all()
    # the precondition, from the oracle's log on the CPU: the symmetric maps do hold equal minimal keys in different rows, many times over
    ties = [_cross_row_ties(cost[b], int(s[b].argmax()), int(g[b].argmax()), o.sel_log[b], int(o.iters[b])) for b in range(len(sym))]
    assert ties[0] >= 5 and ties[1] >= 5 and min(ties[2:5]) >= 50, ties


# ---- 3. an enclosed start: the open list runs empty ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4])
def test_enclosed_start_leaves_through_the_goal_exit(B):
    W = 32
    cases = []
    for a, z in (((8, 8), (0, 5)), ((20, 20), (31, 30)), ((24, 7), (9, 9)), ((5, 25), (22, 3)))[:B]:
        m = np.ones((W, W), np.float32)
        m[a[0] - 2:a[0] + 3, a[1] - 2:a[1] + 3] = 0
        m[a[0] - 1:a[0] + 2, a[1] - 1:a[1] + 2] = 1  # nine free cells inside a closed ring
        cases.append((m, a, z))
    cost, s, g = _problem(cases, W)
    o, status = _check("enclosed", cost, s, g)
    assert (status == 3).all() and (o.iters == 9).all()  # NASTAR_ERR_UNSOLVABLE after the nine cells
    lone = np.zeros((W, W), np.float32)
    lone[17, 17] = lone[0, 0] = 1
    _, status = _check("lone start", *_problem([(lone, (17, 17), (0, 0)), (lone, (0, 0), (17, 17))], W))
    assert (status == 3).all()


# ---- 4. the start on an obstacle, the start equal to the goal ----------------------------------------------------------------------------------------
def test_start_on_an_obstacle_and_start_equal_to_goal():
    W = 32
    rng = np.random.default_rng(4)
    cases = []
    for a, z in (((3, 3), (28, 28)), ((16, 0), (15, 31)), ((31, 31), (0, 0)), ((15, 16), (16, 15))):
        m = _rand_map(rng, W, z)
        m[a] = 0
        cases.append((m, a, z))
    for a in ((0, 0), (15, 31), (16, 0), (31, 31)):
        cases.append((_rand_map(rng, W, a), a, a))
    m = _rand_map(rng, W)
    m[20, 11] = 0
    cases.append((m, (20, 11), (20, 11)))  # both at once
    cost, s, g = _problem(cases, W)
    o, _ = _check("blocked start / start == goal", cost, s, g)
    assert (o.iters[4:] == 1).all()


# ---- 5. / 6. mazes through every stream, 32x32 and 16x16 -------------------------------------------------------------------------------------------------
_MAZES = {}


def _mazes(W, B):
    if (W, B) not in _MAZES:
        from neural_astar.utils import synthetic as syn
        mz = syn.maze_maps(B, W, seed=500 + W)
        _MAZES[W, B] = (np.ascontiguousarray(mz.map_designs[:, 0]), np.ascontiguousarray(mz.start_maps[:, 0]), np.ascontiguousarray(mz.goal_maps[:, 0]))
    return _MAZES[W, B]


@pytest.mark.parametrize("W,B", [(32, 67), (16, 3)])
def test_mazes_stored_heuristic(W, B):
    m, s, g = _mazes(W, B)
    o, _ = _check("half", m, s, g)
    assert (o.map_status == 0).any()
    _check("0.3", m[:5], s[:5], g[:5], g_ratio=0.3)
    _check("0.8", m[:5], s[:5], g[:5], g_ratio=0.8)


@pytest.mark.parametrize("W,B", [(32, 5), (16, 3)])
def test_mazes_general_and_signed_streams(W, B):
    m, s, g = _mazes(W, B)
    rng = np.random.default_rng(60 + W)
    _check("uniform costs", rng.random(m.shape, dtype=np.float32), s, g, passable=m)
    _check("uniform costs 0.3", rng.random(m.shape, dtype=np.float32), s, g, passable=m, g_ratio=0.3)
    _check("unit costs, two tensors", m, s, g, passable=m.copy())
    _check("signed costs", (rng.random(m.shape, dtype=np.float32) * 3 - 2).astype(np.float32), s, g, passable=m)


@pytest.mark.parametrize("W,B", [(32, 5), (16, 3)])
@pytest.mark.parametrize("T", [7, 40])
def test_mazes_truncated_budget(W, B, T):
    m, s, g = _mazes(W, B)
    o, _ = _check("budget", m, s, g, max_iters=T)
    assert (o.iters == T).any()  # some search did run out of steps
    rng = np.random.default_rng(70 + W + T)
    _check("budget, uniform costs", rng.random(m.shape, dtype=np.float32), s, g, passable=m, max_iters=T)
    _check("budget, signed costs", (rng.random(m.shape, dtype=np.float32) * 3 - 2).astype(np.float32), s, g, passable=m, max_iters=T)


def test_small_map_special_cases():
    """cases 1-4 at 16x16: the one-row finish reads lane 0 alone"""
    W = 16
    rng = np.random.default_rng(16)
    ones = np.ones((W, W), np.float32)
    block = ones.copy()
    block[5:11, 5:11] = 0
    ring = ones.copy()
    ring[6:11, 6:11] = 0
    ring[7:10, 7:10] = 1
    blocked = _rand_map(rng, W, (14, 14))
    blocked[2, 2] = 0
    cost, s, g = _problem([(block, (0, 0), (15, 15)), (ring, (8, 8), (0, 3)), (blocked, (2, 2), (14, 14))], W)
    _, status = _check("16x16", cost, s, g)
    assert status.tolist()[:2] == [0, 3]
    _check("16x16 start == goal", *_problem([(ones, (0, 0), (0, 0)), (block, (15, 15), (15, 15)), (ring, (8, 8), (8, 8))], W))


# ---- 7. 64x64 keeps its path ---------------------------------------------------------------------------------------------------------------------------
def test_one_large_map():
    m, s, g = _mazes(64, 1)
    _check("64x64", m, s, g)
    _check("64x64 uniform costs", np.random.default_rng(64).random(m.shape, dtype=np.float32), s, g, passable=m)
