"""GPU tests (-m gpu) of the proof kernel (include/nastar_verdict.h) where its mask assembly, its load pipeline and its flood can go wrong,
all through the C ABI with ``proved_out`` prefilled with -1:

  1. batches larger than the largest grid (4 x 256 wavefronts): a wavefront takes two or three trips of its grid-stride loop, the loads of
     one trip are in flight during the flood of the trip before, and the last wavefront has a half without a map
  2. every bit of a row mask lands where it belongs (one map per cell: start there, goal beside it, nothing else passable)
  3. nothing leaks between the two maps of a wavefront, nothing wraps between rows
  4. flood lengths around the exit test (every 8 levels)
  5. the cost range at every position of a 16-byte load, in the first and last row and round
  6. forward() at B = 4099 with the proof on and off

The oracle is a batched numpy flood (one [B, H + 2, W + 2] bool array, 9 shifts a level), computed once per pool of maps and shared.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_COST = {32: 60.0, 64: 15.0}  # bound (b) of include/nastar_verdict.h: 61440 / (H * W)


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@contextlib.contextmanager
def early_verdict(on):
    from neural_astar import _native
    prev = _native.EARLY_VERDICT
    _native.EARLY_VERDICT = bool(on)
    try:
        yield
    finally:
        _native.EARLY_VERDICT = prev


def _prove(cost, start, goal, passable=None):
    """(proved[B], word, counter) of one launch; passable None: the cost tensor is the passable tensor (one pointer)"""
    from neural_astar import _native
    lib = _native.load()
    dev = _dev()
    B, W = cost.shape[0], cost.shape[-1]
    ct, st, gt = _t(cost), _t(start), _t(goal)
    pt = ct if passable is None else _t(passable)
    proved = torch.full((B,), -1, dtype=torch.int32, device=dev)
    word = torch.zeros(16, dtype=torch.int32).pin_memory()
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = lib.nastar_solvable_proof(ct.data_ptr(), st.data_ptr(), gt.data_ptr(), pt.data_ptr(), B, W, W, proved.data_ptr(), word.data_ptr(),
                                   counter.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    assert lib.nastar_solvable_proof_sync() == 0
    return proved.cpu().numpy(), int(word[0]), int(counter.item())


def _top(x):
    """(has[B], index[B]): the non-zero cell with the highest index of each map"""
    f = x.reshape(x.shape[0], -1) != 0
    return f.any(1), f.shape[1] - 1 - f[:, ::-1].argmax(1)


def _flood_levels(passable, start):
    """[B, H, W] int32: the level at which the flood from the start cell (highest non-zero index) first holds each cell, -1 where it never
    does; 8-connected over cells whose passable value is non-zero, the start cell itself need not be passable.  Batched."""
    B, H, W = passable.shape
    hs, si = _top(start)
    ok = np.zeros((B, H + 2, W + 2), bool)
    ok[:, 1:-1, 1:-1] = passable != 0
    vis = np.zeros_like(ok)
    idx = np.flatnonzero(hs)
    vis[idx, 1 + si[idx] // W, 1 + si[idx] % W] = True
    lev = np.where(vis, 0, -1).astype(np.int32)
    act = idx  # maps whose flood still moves
    n = 0
    while act.size:
        n += 1
        v = vis[act]
        grow = v.copy()
        for dr in (0, 1, 2):
            for dc in (0, 1, 2):
                if (dr, dc) != (1, 1):
                    grow[:, 1:-1, 1:-1] |= v[:, dr:dr + H, dc:dc + W]
        grow &= ok[act]
        grow |= v
        new = grow & ~v
        moved = new.reshape(act.size, -1).any(1)
        lev[act] = np.where(new, n, lev[act])
        vis[act] = grow
        act = act[moved]
    return lev[:, 1:-1, 1:-1]


def _want(passable, start, goal, in_range=None):
    """proved[B] by the definition: both cells exist, the goal is in the start's closure, the costs are in range"""
    B, H, W = passable.shape
    hs, si = _top(start)
    hg, gi = _top(goal)
    # (one flood per distinct pair of passable map and start cell: the batches repeat a few maps many times)
    first, of = {}, np.empty(B, np.int64)
    for b in range(B):
        of[b] = first.setdefault((passable[b].tobytes(), int(si[b]), bool(hs[b])), len(first))
    uniq = np.array([np.flatnonzero(of == k)[0] for k in range(len(first))]) if B > 4 * len(first) else None
    if uniq is None:
        lev = _flood_levels(passable, start)
    else:
        lev = _flood_levels(passable[uniq], start[uniq])[of]
    reached = lev.reshape(B, -1)[np.arange(B), gi] >= 0
    ok = hs & hg & reached
    return (ok if in_range is None else ok & in_range).astype(np.int32)


# ---- 1. several trips per wavefront --------------------------------------------------------------------------------------------------------
def _specials(W):
    """the special maps of test_verdict_proof_gpu._case_batch: (passable, start, goal, cost or None, in_range) each; cost None = the passable map"""
    out = []

    def blank(fill):
        return np.full((W, W), fill, np.float32), np.zeros((W, W), np.float32), np.zeros((W, W), np.float32)

    p, s, g = blank(1)  # a full wall between start and goal
    p[W // 2, :] = 0
    s[0, 0] = 1
    g[W - 1, W - 1] = 1
    out.append((p, s, g, None, True))
    p, s, g = blank(0)  # start == goal
    p[3, 4] = s[3, 4] = g[3, 4] = 1
    out.append((p, s, g, None, True))
    p, s, g = blank(1)  # start on an obstacle (still the source)
    p[2, 2] = 0
    s[2, 2] = 1
    g[9, 9] = 1
    out.append((p, s, g, None, True))
    p, s, g = blank(1)  # goal on an obstacle: never opened
    p[9, 9] = 0
    s[2, 2] = 1
    g[9, 9] = 1
    out.append((p, s, g, None, True))
    p, s, g = blank(1)  # an empty start map
    g[9, 9] = 1
    out.append((p, s, g, None, True))
    p, s, g = blank(1)  # two start cells: the higher index counts, and only that one is walled in with the goal
    p[W // 2, :] = 0
    s[0, 0] = s[W - 1, 0] = 1
    g[W - 1, W - 1] = 1
    out.append((p, s, g, None, True))
    for bad, ok in ((-1.0, False), (np.nan, False), (np.inf, False), (2e30, False), (1e30, False),
                    (np.nextafter(np.float32(MAX_COST[W]), np.float32(np.inf)), False), (MAX_COST[W], True)):
        p, s, g = blank(0)  # one corridor, one cost value on it
        p[5, :] = 1
        s[5, 0] = 1
        g[5, W - 1] = 1
        c = p.copy()
        c[5, 7] = bad
        out.append((p, s, g, c, ok))
    return out


@functools.lru_cache(maxsize=None)
def _pool(W):
    """a few dozen mazes (32x32) and random maps with p in 0.25-0.5 (start and goal anywhere: a good share unsolvable), with their proved
    values by the oracle: (passable, start, goal, want), [P, W, W] / [P]"""
    from neural_astar.utils import synthetic as syn
    rng = np.random.default_rng(7 + W)
    n_rand = 160 if W == 32 else 96
    pas = (rng.random((n_rand, W, W)) > rng.uniform(0.25, 0.5, (n_rand, 1, 1))).astype(np.float32)
    s = np.zeros_like(pas)
    g = np.zeros_like(pas)
    s.reshape(n_rand, -1)[np.arange(n_rand), rng.integers(W * W, size=n_rand)] = 1
    g.reshape(n_rand, -1)[np.arange(n_rand), rng.integers(W * W, size=n_rand)] = 1
    if W == 32:
        mz = syn.maze_maps(40, 32, seed=3)
        pas = np.concatenate([mz.map_designs[:, 0], pas])
        s = np.concatenate([mz.start_maps[:, 0], s])
        g = np.concatenate([mz.goal_maps[:, 0], g])
    want = _want(pas, s, g)
    assert 0.2 < want.mean() < 0.9, want.mean()  # (a good share of each kind)
    return pas, s, g, want


def _big_batch(B, W, same, solvable_only):
    """(cost, start, goal, passable or None, want): pool maps at pseudo-random places, the specials at scattered indices and at B - 1"""
    pas_p, s_p, g_p, want_p = _pool(W)
    rng = np.random.default_rng(B + W + int(same))
    ids = np.flatnonzero(want_p == 1) if solvable_only else np.arange(want_p.size)
    pick = ids[rng.integers(ids.size, size=B)]
    pas, s, g, want = pas_p[pick].copy(), s_p[pick].copy(), g_p[pick].copy(), want_p[pick].copy()
    cost = pas.copy() if same else (rng.random((B, W, W)).astype(np.float32) + 0.01)
    if not solvable_only:
        sp = _specials(W)
        where = [1, 2, 1023, 1024, 2047, 2048, 2049, 2050, B - 2, B - 1] + list(range(300, B - 2, 331))
        sp_want = _want(np.stack([x[0] for x in sp]), np.stack([x[1] for x in sp]), np.stack([x[2] for x in sp]), np.array([x[4] for x in sp]))
        for n, b in enumerate(where):
            k = n % len(sp) if b != B - 1 else len(sp) - 1  # (the last map: the corridor at the bound itself, proved)
            p1, s1, g1, c1, _ = sp[k]
            s[b], g[b], want[b] = s1, g1, sp_want[k]
            if same:
                cost[b] = p1 if c1 is None else c1
                pas[b] = cost[b]
            else:
                pas[b] = p1
                cost[b] = 0.5 if c1 is None else np.where(p1 != 0, c1, 0.5)
    return cost, s, g, (None if same else pas), want


@pytest.mark.parametrize("B,W,same", [(4099, 32, True), (4099, 32, False), (2051, 64, True)], ids=["4099x32_one_tensor", "4099x32_two_tensors", "2051x64"])
def test_several_trips_equal_the_flood(B, W, same):
    cost, s, g, pas, want = _big_batch(B, W, same, solvable_only=False)
    pv, word, counter = _prove(cost, s, g, pas)
    assert np.array_equal(pv, want), f"proved != flood at maps {np.flatnonzero(pv != want)[:20].tolist()} (of {int((pv != want).sum())})"
    assert 0 < want.sum() < B and want[B - 1] == 1
    assert word == 2 and counter == 0


@pytest.mark.parametrize("B,W,same", [(4099, 32, True), (4099, 32, False), (2051, 64, True)], ids=["4099x32_one_tensor", "4099x32_two_tensors", "2051x64"])
def test_several_trips_of_solvable_maps_give_word_one(B, W, same):
    cost, s, g, pas, want = _big_batch(B, W, same, solvable_only=True)
    assert want.all()
    pv, word, counter = _prove(cost, s, g, pas)
    assert np.array_equal(pv, want), f"unproved: maps {np.flatnonzero(pv != want)[:20].tolist()}"
    assert word == 1 and counter == 0


# ---- 2. every bit lands where it belongs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,step", [(32, 1), (64, 3)])
@pytest.mark.parametrize("same", [True, False], ids=["one_tensor", "cost_and_passable"])
def test_every_bit_lands_where_it_belongs(W, step, same):
    cells = np.arange(0, W * W, step)
    B = cells.size
    r, c = cells // W, cells % W
    horizontal = (np.arange(B) % 2) == 0
    gr = np.where(horizontal, r, np.where(r == W - 1, r - 1, r + 1))
    gc = np.where(horizontal, np.where(c == W - 1, c - 1, c + 1), c)
    s = np.zeros((B, W, W), np.float32)
    g = np.zeros_like(s)
    pas = np.zeros_like(s)
    n = np.arange(B)
    s[n, r, c] = 1
    g[n, gr, gc] = 1
    pas[n, r, c] = 1
    pas[n, gr, gc] = 1
    ones = np.ones_like(pas)
    pv, word, counter = _prove(pas if same else ones, s, g, None if same else pas)
    assert np.array_equal(pv, np.ones(B, np.int32)), f"unproved: cells {cells[pv != 1][:20].tolist()}"
    assert word == 1 and counter == 0
    pas[n, gr, gc] = 0  # the goal is no longer passable: nothing may be proved
    pv, word, counter = _prove(pas if same else ones, s, g, None if same else pas)
    assert not pv.any(), f"proved without a passable goal: cells {cells[pv != 0][:20].tolist()}"
    assert word == 2 and counter == 0


# ---- 3. no leak between the maps of a wavefront, no wrap between rows -----------------------------------------------------------------------
def _ringed(W, start, goal, open_one):
    """fully passable but for the 8 cells around the start (one of them open in the twin); the goal far away"""
    p = np.ones((W, W), np.float32)
    s = np.zeros_like(p)
    g = np.zeros_like(p)
    r, c = start
    p[r - 1:r + 2, c - 1:c + 2] = 0
    p[r, c] = 1
    if open_one:
        p[r - 1, c] = 1
    s[r, c] = 1
    g[goal] = 1
    return p, s, g


def _leak_and_wrap_batch(W):
    """(passable, start, goal, want) as lists; 32x32: maps (2k, 2k + 1) share a wavefront"""
    maps, want = [], []

    def full(start, goal):
        p = np.ones((W, W), np.float32)
        s = np.zeros_like(p)
        g = np.zeros_like(p)
        s[start] = 1
        g[goal] = 1
        return p, s, g

    for col in (0, 13, W - 1):
        for twin in (False, True):
            # the first map floods its last row; the second has its goal in row 0 and a start that is walled off
            maps += [full((W - 1, col), (0, 0)), _ringed(W, (W // 2, W // 2), (0, col), twin)]
            want += [1, int(twin)]
            # the mirror: the second map floods its row 0; the first has its goal in the last row
            maps += [_ringed(W, (W // 2, W // 2), (W - 1, col), twin), full((0, col), (W - 1, W - 1))]
            want += [int(twin), 1]
    for r in (0, 7, 8, W // 2 - 1, W - 2):
        # a passable cell at the last column of row r, the goal at column 0 of row r + 1, otherwise obstacles
        p = np.zeros((W, W), np.float32)
        s = np.zeros_like(p)
        g = np.zeros_like(p)
        p[r, W - 1] = p[r + 1, 0] = 1
        s[r, W - 1] = 1
        g[r + 1, 0] = 1
        maps.append((p, s, g))
        want.append(0)
        for twin in (False, True):
            # ... and with row r + 1 passable up to column W - 3: one more cell (column W - 2) joins it to the start
            p2 = p.copy()
            p2[r + 1, :W - 2] = 1
            if twin:
                p2[r + 1, W - 2] = 1
            maps.append((p2, s, g))
            want.append(int(twin))
        # the same towards the row above: start at column 0 of row r + 1, goal at the last column of row r
        maps.append((p, g.copy(), s.copy()))
        want.append(0)
    return [np.stack([m[i] for m in maps]) for i in range(3)] + [np.array(want, np.int32)]


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("same", [True, False], ids=["one_tensor", "cost_and_passable"])
def test_no_leak_between_maps_and_no_wrap_between_rows(W, same):
    pas, s, g, want = _leak_and_wrap_batch(W)
    assert np.array_equal(_want(pas, s, g), want)  # (the oracle agrees with the construction)
    pv, word, counter = _prove(pas if same else np.ones_like(pas), s, g, None if same else pas)
    assert np.array_equal(pv, want), f"maps {np.flatnonzero(pv != want).tolist()}: proved {pv[pv != want].tolist()}"
    assert word == 2 and counter == 0


# ---- 4. flood lengths around the exit test --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _serpentine(W):
    """(passable, level of every cell from the start at (0, 0)): corridors along the even rows, joined at alternating ends"""
    p = np.ones((W, W), np.float32)
    for r in range(1, W, 2):
        p[r, :] = 0
        p[r, (W - 1) if (r // 2) % 2 == 0 else 0] = 1
    s = np.zeros_like(p)
    s[0, 0] = 1
    return p, _flood_levels(p[None], s[None])[0]


def _length_batch(W):
    p, lev = _serpentine(W)
    longest = int(lev.max())
    assert longest > W * W // 3
    dists = sorted({d for k in (1, 2, 3, longest // 16, longest // 8 - 1) for d in (8 * k - 1, 8 * k, 8 * k + 1)} | {1, longest - 1, longest})
    s0 = np.zeros_like(p)
    s0[0, 0] = 1
    near = (np.ones_like(p), s0, np.zeros_like(p))  # ends at level 1
    near[2][1, 1] = 1
    stall_p = np.zeros_like(p)  # stalls unsolved at once: nothing passable around the start
    stall = (stall_p, s0, np.zeros_like(p))
    stall[2][W - 1, W - 1] = 1
    maps, want = [], []
    for d in dists:
        g = np.zeros_like(p)
        cell = np.argwhere(lev == d)[0]
        g[cell[0], cell[1]] = 1
        route = (p, s0, g)
        # route first and second in its pair, beside a map that is over at level 1 and beside one that stalls unsolved
        maps += [route, near, near, route, route, stall, stall, route]
        want += [1, 1, 1, 1, 1, 0, 0, 1]
        # ... and a route one cell short: the cell before the goal is blocked (the goal at distance d is never reached)
        if d > 1:
            p2 = p.copy()
            prev = np.argwhere(lev == d - 1)
            for q in prev:
                p2[q[0], q[1]] = 0
            maps += [(p2, s0, g), near]
            want += [0, 1]
    return [np.stack([m[i] for m in maps]) for i in range(3)] + [np.array(want, np.int32), dists]


@pytest.mark.parametrize("W", [32, 64])
def test_flood_lengths_around_the_exit_test(W):
    pas, s, g, want, dists = _length_batch(W)
    assert np.array_equal(_want(pas, s, g), want)
    for same in (True, False):
        pv, word, counter = _prove(pas if same else np.ones_like(pas), s, g, None if same else pas)
        assert np.array_equal(pv, want), f"distances {dists}: maps {np.flatnonzero(pv != want).tolist()} proved {pv[pv != want].tolist()}"
        assert word == 2 and counter == 0


# ---- 5. the cost range at every position of a load ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("same", [True, False], ids=["one_tensor", "cost_and_passable"])
def test_cost_range_at_every_position_of_a_load(W, same):
    G = W // 4  # rows a group of lanes assembles: row k of a group is read in round k
    bound = np.float32(MAX_COST[W])
    values = [(np.float32(-1.0), 0), (np.float32(np.nan), 0), (np.nextafter(bound, np.float32(np.inf)), 0), (np.float32(-0.0), 1), (bound, 1),
              (np.float32(-np.nan), 0), (np.float32(-1e-45), 0)]
    rows = [0, G - 1, W - G, W - 1]  # first row = first round, last round of the first group, first round of the last group, last row = last round
    cols = [4 * j + e for j in (0, G // 2, G - 1) for e in range(4)]
    cases = [(r, c, v, ok) for r in rows for c in cols for v, ok in values]
    B = len(cases)
    cost = np.ones((B, W, W), np.float32)
    s = np.zeros_like(cost)
    g = np.zeros_like(cost)
    s[:, W // 2, W // 2] = 1
    g[:, W // 2, W // 2 + 1] = 1
    for b, (r, c, v, _) in enumerate(cases):
        cost[b, r, c] = v
    want = np.array([ok for *_, ok in cases], np.int32)
    pv, word, counter = _prove(cost, s, g, None if same else np.ones_like(cost))
    bad = np.flatnonzero(pv != want)
    assert bad.size == 0, f"(row, column, value, proved) {[(cases[b][0], cases[b][1], float(cases[b][2]), int(pv[b])) for b in bad[:12]]}"
    assert word == 2 and counter == 0


# ---- 6. forward() at B = 4099 ----------------------------------------------------------------------------------------------------------------
def test_forward_of_4099_maps_with_the_proof_equals_forward_without():
    from neural_astar.planner import VanillaAstar
    from neural_astar.utils import synthetic as syn
    mz = syn.maze_maps(40, 32, seed=3)
    pick = np.random.default_rng(5).integers(40, size=4099)
    m, s, g = (_t(x[pick]) for x in mz)
    va = VanillaAstar().to(_dev()).eval()
    res = {}
    for on in (False, True):
        with early_verdict(on), torch.no_grad():
            out = va(m, s, g)
        a = va.astar
        res[on] = (out.histories, out.paths, a.last_iters, a.last_status, a.last_verdict_source)
        torch.cuda.synchronize()
    assert res[False][4] in ("flag", "sync") and res[True][4] == "proof"
    for a, b in zip(res[True][:4], res[False][:4]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert int(res[True][3].abs().sum()) == 0
