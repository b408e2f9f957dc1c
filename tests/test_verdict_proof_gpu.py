"""GPU tests (-m gpu) of the early verdict (include/nastar_verdict.h): a side launch proves every map of a batch solvable and a checked
forward() returns on that proof while its searches are still running.

  1. the proof kernel alone, through the C ABI: sound (proved => the search ends with status 0) and complete (== a numpy flood fill on
     every map whose start / goal cells exist and whose costs are in range); the terminal word
  2. forward() with the proof == forward() without it, bit for bit
  3. an unsolvable map still raises in the same call, with the same text
  4. calls whose verdict is not a property of the inputs alone never take the proof
  5. status rows over many calls: no stale flag, nothing left behind
  6. the proof sees its inputs in the order of the caller's stream
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@contextlib.contextmanager
def early_verdict(on):
    """the switch NASTAR_EARLY_VERDICT as the package holds it after import"""
    from neural_astar import _native
    prev = _native.EARLY_VERDICT
    _native.EARLY_VERDICT = bool(on)
    try:
        yield
    finally:
        _native.EARLY_VERDICT = prev


@functools.lru_cache(maxsize=None)
def _mazes(B, size=32, seed=3):
    from neural_astar.utils import synthetic as syn
    return syn.maze_maps(B, size, seed=seed)


@functools.lru_cache(maxsize=None)
def _random_maps(B, H, W, seed=4):
    from neural_astar.utils import synthetic as syn
    return syn.random_obstacle_maps(B, H, W, 0.2, seed=seed)


# ---- 1. the proof kernel alone -----------------------------------------------------------------------------------------------------------
# bound (b) of include/nastar_verdict.h: 61440 / (H * W) -- every accumulated g stays below 2^16, where fp32 keeps the goal's key strictly
# below the key of every cell its expansion would open for g_ratio in [0.5, 0.75] (the error analysis is in csrc/nastar_verdict.hip.h)
MAX_COST = {32: 60.0, 64: 15.0}


def _summary_of_search(ct, st, gt, pt, W, g_ratio=0.5):
    """the summary cells 1..15 that ONE search launch of these maps sets (a list; [] = every map ended clean, no note)"""
    from neural_astar import ops
    board = ops.StatusBoard.of(_dev())
    row = board.acquire()
    ops.search_nograd(ct[:, None], st[:, None], gt[:, None], pt[:, None], g_ratio, W * W, summary_ptr=board.ptr(row))
    torch.cuda.synchronize()
    cells = [c for c in range(1, ops.SUMMARY_WORDS) if board.np[row, c]]
    board.release(row)
    return cells


def _flood(passable, start, goal):
    """(has_start, has_goal, reached): the flood closure of the start cell (the non-zero cell with the highest index) over cells whose
    passable value is non-zero, 8-connected, zero padding; the start cell itself need not be passable"""
    H, W = passable.shape
    si, gi = np.flatnonzero(start.ravel()), np.flatnonzero(goal.ravel())
    if si.size == 0 or gi.size == 0:
        return si.size > 0, gi.size > 0, False
    ok = (passable != 0)
    vis = np.zeros((H + 2, W + 2), bool)
    vis[1 + si[-1] // W, 1 + si[-1] % W] = True
    while True:
        grow = np.zeros_like(vis)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                grow |= np.roll(np.roll(vis, dr, 0), dc, 1)
        grow[1:-1, 1:-1] &= ok
        grow[0], grow[-1], grow[:, 0], grow[:, -1] = False, False, False, False
        grow |= vis
        if (grow == vis).all():
            break
        vis = grow
    return True, True, bool(vis[1 + gi[-1] // W, 1 + gi[-1] % W])


def _case_batch(B, W, same):
    """(cost, start, goal, passable, in_range[B]): mazes, random maps with p from 0.25 to 0.5 (a good share unsolvable: start and goal are
    drawn anywhere), and -- where the batch has room -- the special maps of the issue.  ``same``: cost IS the passable tensor"""
    rng = np.random.default_rng(100 * B + W + int(same))
    pas = np.zeros((B, W, W), np.float32)
    s = np.zeros((B, W, W), np.float32)
    g = np.zeros((B, W, W), np.float32)
    mz = _mazes(min(B, 40), W) if W == 32 else _random_maps(B, W, W)
    for b in range(B):
        if b % 3 == 0 and b // 3 < mz.map_designs.shape[0]:
            k = b // 3
            pas[b], s[b], g[b] = mz.map_designs[k, 0], mz.start_maps[k, 0], mz.goal_maps[k, 0]
        else:
            pas[b] = (rng.random((W, W)) > rng.uniform(0.25, 0.5)).astype(np.float32)
            s[b].flat[rng.integers(W * W)] = 1
            g[b].flat[rng.integers(W * W)] = 1
    cost = pas.copy() if same else (rng.random((B, W, W)).astype(np.float32) + 0.01)
    in_range = np.ones(B, bool)

    def corridor(b):  # one passable row between the start (left end) and the goal (right end): the only route
        pas[b], s[b], g[b] = 0, 0, 0
        pas[b, 5, :] = 1
        s[b, 5, 0] = 1
        g[b, 5, W - 1] = 1
        cost[b] = pas[b] if same else 0.5

    if B >= 16:
        last = B - 1  # (the unpaired half-wave of an odd batch gets a special too)
        pas[1], s[1], g[1] = 1, 0, 0  # a full wall between start and goal
        pas[1, W // 2, :] = 0
        s[1, 0, 0] = 1
        g[1, W - 1, W - 1] = 1
        s[2], g[2] = 0, 0  # start == goal
        pas[2, 3, 4] = 1
        s[2, 3, 4] = 1
        g[2, 3, 4] = 1
        pas[4], s[4], g[4] = 1, 0, 0  # start on an obstacle (still the source), goal reachable from it
        pas[4, 2, 2] = 0
        s[4, 2, 2] = 1
        g[4, 9, 9] = 1
        pas[5], s[5], g[5] = 1, 0, 0  # goal on an obstacle: never opened
        pas[5, 9, 9] = 0
        s[5, 2, 2] = 1
        g[5, 9, 9] = 1
        s[7] = 0  # an empty start map
        pas[8], s[8], g[8] = 1, 0, 0  # two non-zero start cells: the higher index is the start -- and only that one is walled in with the goal
        pas[8, W // 2, :] = 0
        s[8, 0, 0] = 1
        s[8, W - 1, 0] = 1
        g[8, W - 1, W - 1] = 1
        if same:
            cost[[1, 2, 4, 5, 8]] = pas[[1, 2, 4, 5, 8]]
        corridor(10)  # one negative cost
        cost[10, 5, 7] = -1.0
        corridor(11)  # one NaN cost
        cost[11, 5, 7] = np.nan
        corridor(13)  # one +inf cost
        cost[13, 5, 7] = np.inf
        corridor(14)  # 2e30 on the only corridor: above the bound that keeps every accumulated g finite
        cost[14, 5, 7] = 2e30
        corridor(16)  # 1e30: finite, and far above the bound
        cost[16, 5, 7] = 1e30
        corridor(17)  # the first float above the bound
        cost[17, 5, 7] = np.nextafter(np.float32(MAX_COST[W]), np.float32(np.inf))
        corridor(last)  # ... and the bound itself, the largest cost the proof accepts: proved, and solvable
        cost[last, 5, 7] = MAX_COST[W]
        in_range[[10, 11, 13, 14, 16, 17]] = False
        if same:
            pas = cost
    elif same:
        pas = cost
    return cost, s, g, pas, in_range


@pytest.mark.parametrize("B,W", [(1, 32), (3, 32), (130, 32), (5, 64)])
@pytest.mark.parametrize("same", [True, False], ids=["one_tensor", "cost_and_passable"])
def test_proved_is_sound_and_equals_the_flood(B, W, same):
    from neural_astar import _native, ops
    lib = _native.load()
    dev = _dev()
    cost, s, g, pas, in_range = _case_batch(B, W, same)
    ct, st, gt = _t(cost), _t(s), _t(g)
    pt = ct if same else _t(pas)
    proved = torch.full((B,), -1, dtype=torch.int32, device=dev)
    word = torch.zeros(16, dtype=torch.int32).pin_memory()
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = lib.nastar_solvable_proof(ct.data_ptr(), st.data_ptr(), gt.data_ptr(), pt.data_ptr(), B, W, W, proved.data_ptr(), word.data_ptr(),
                                   counter.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    assert lib.nastar_solvable_proof_sync() == 0
    pv = proved.cpu().numpy()
    assert int(counter.item()) == 0  # the cell is 0 again: the next launch can take it
    status = ops.search_nograd(ct[:, None], st[:, None], gt[:, None], pt[:, None], 0.5, W * W)[3].cpu().numpy()
    want = np.zeros(B, np.int32)
    for b in range(B):
        hs, hg, reached = _flood(pas[b], s[b], g[b])
        if hs and hg and in_range[b]:
            want[b] = int(reached)
    bad = np.flatnonzero((pv == 1) & (status != 0))
    assert bad.size == 0, f"proved but the search reported a status: maps {bad.tolist()} status {status[bad].tolist()}"
    assert np.array_equal(pv, want), f"proved != flood at maps {np.flatnonzero(pv != want).tolist()}"
    # ... and no summary cell: the launch of exactly the proved maps reports nothing, not even the COUPLED note
    idx = torch.from_numpy(np.flatnonzero(pv == 1)).to(dev)
    if idx.numel():
        sub = [x.index_select(0, idx).contiguous() for x in (ct, st, gt)]
        assert _summary_of_search(sub[0], sub[1], sub[2], sub[0] if same else pt.index_select(0, idx).contiguous(), W) == []
    assert int(word[0]) == (1 if want.all() else 2)
    if B >= 16:
        assert 0 < want.sum() < B and want[2] == 1 and want[4] == 1 and want[8] == 1 and want[B - 1] == 1
        assert not want[[1, 5, 7, 10, 11, 13, 14, 16, 17]].any()


def _long_route_maps(W, costs):
    """one map per cost value: a serpentine over the upper three quarters (a route of about W * W / 3 cells, so the accumulated g is large), a
    shaft down the left edge and a corridor along row W - 2 to the goal.  Behind the goal lies a pocket -- one passable cell above and to the
    right of it (a LOWER index), reachable through the goal only and free of charge: when the goal is selected it is unopened, and the keys
    of the fixed-point test differ by (1 - g_ratio) h0(pocket) alone -- exactly where fp32 lets them tie once g is large (the COUPLED note).
    Every other cell costs costs[b]."""
    B = len(costs)
    pas = np.ones((B, W, W), np.float32)
    top = 3 * W // 4
    for r in range(1, top, 2):
        pas[:, r, :] = 0
        pas[:, r, (W - 1) if (r // 2) % 2 == 0 else 0] = 1  # (the last wall row opens at column 0)
    pas[:, top:, :] = 0
    pas[:, top:W - 1, 0] = 1
    cg = W // 2
    pas[:, W - 2, :cg + 1] = 1
    pas[:, W - 3, cg + 1] = 1  # the pocket
    s = np.zeros_like(pas)
    g = np.zeros_like(pas)
    s[:, 0, 0] = 1
    g[:, W - 2, cg] = 1
    cost = np.empty_like(pas)
    for b, c in enumerate(costs):
        cost[b] = c
    cost[:, W - 3, cg + 1] = 0
    return cost, s, g, pas


@pytest.mark.parametrize("W", [32, 64])
@pytest.mark.parametrize("g_ratio", [0.5, 0.75])
def test_large_costs_on_a_long_route_never_prove_a_map_that_reports_a_note(W, g_ratio):
    """the fixed-point inequality in fp32: at the bound the search reports NOTHING (no status, no COUPLED note) at both ends of the g_ratio
    range the proof is used for; above it the proof abstains -- whatever the search then reports.  Then forward() with the proof on and off,
    including the row the proved launch leaves to the board."""
    from neural_astar import _native, ops
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    lib = _native.load()
    dev = _dev()
    cmax = np.float32(MAX_COST[W])
    costs = [cmax, np.nextafter(cmax, np.float32(np.inf)), np.float32(1e6), np.float32(1e8), np.float32(1e30)]
    cost, s, g, pas = _long_route_maps(W, costs)
    ct, st, gt, pt = _t(cost), _t(s), _t(g), _t(pas)
    B = len(costs)
    proved = torch.full((B,), -1, dtype=torch.int32, device=dev)
    word = torch.zeros(16, dtype=torch.int32).pin_memory()
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert lib.nastar_solvable_proof(ct.data_ptr(), st.data_ptr(), gt.data_ptr(), pt.data_ptr(), B, W, W, proved.data_ptr(), word.data_ptr(),
                                     counter.data_ptr(), torch.cuda.current_stream(dev).cuda_stream) == 0
    assert lib.nastar_solvable_proof_sync() == 0
    assert proved.cpu().tolist() == [1, 0, 0, 0, 0] and int(word[0]) == 2
    cells = [_summary_of_search(ct[b:b + 1], st[b:b + 1], gt[b:b + 1], pt[b:b + 1], W, g_ratio) for b in range(B)]
    print(f"summary cells per cost {[float(c) for c in costs]} at g_ratio {g_ratio}: {cells}")
    assert cells[0] == [], f"a proved map reported summary cells {cells[0]}"
    if g_ratio == 0.5:
        # what the bound is for (float32 arithmetic of the two keys, worked out by hand for this route): far above it the keys tie and the
        # search reports the note -- a proof that accepted these maps would have returned a verdict the launch contradicts
        assert cells[3] == [ops.SUMMARY_COUPLED] and cells[4] == [ops.SUMMARY_COUPLED], cells
    # forward(): the proved map alone returns on the proof, the batch that holds unproved maps does not; both equal the run without a proof
    board = ops.StatusBoard.of(dev)
    for sl in (slice(0, 1), slice(0, B)):
        res = {}
        for on in (False, True):
            da = DifferentiableAstar(g_ratio, 1.0).to(dev).eval()
            with early_verdict(on), torch.no_grad():
                out = da(ct[sl, None], st[sl, None], gt[sl, None], pt[sl, None])
            res[on] = (out.histories, out.paths, da.last_iters, da.last_status, da.last_verdict_source)
            torch.cuda.synchronize()
            board._reap(False)  # raises if the proved launch reported anything
        assert res[False][4] in ("flag", "sync") and (res[True][4] == "proof" if sl.stop == 1 else res[True][4] in ("flag", "sync"))
        for a, b in zip(res[True][:4], res[False][:4]):
            assert torch.equal(a, b)
    assert not board.proved


def test_word_is_one_for_a_batch_of_solvable_maps():
    from neural_astar import _native
    lib = _native.load()
    dev = _dev()
    pr = _mazes(40)
    for B in (1, 3, 40):
        m, s, g = (_t(x[:B]) for x in pr)
        word = torch.zeros(16, dtype=torch.int32).pin_memory()
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert lib.nastar_solvable_proof(m.data_ptr(), s.data_ptr(), g.data_ptr(), m.data_ptr(), B, 32, 32, None, word.data_ptr(),
                                         counter.data_ptr(), torch.cuda.current_stream(dev).cuda_stream) == 0
        assert lib.nastar_solvable_proof_sync() == 0
        assert int(word[0]) == 1 and int(counter.item()) == 0


# ---- 2. forward() with the proof == forward() without it ---------------------------------------------------------------------------------
def _levels(pr):
    from neural_astar.utils import synthetic as syn
    B = pr.map_designs.shape[0]
    gi = pr.goal_maps.reshape(B, -1).argmax(1)
    si = pr.start_maps.reshape(B, -1).argmax(1)
    d = syn.geodesic_distance(pr.map_designs[:, 0] > 0, gi).reshape(B, -1)
    return d[np.arange(B), si].astype(np.int32)


def _forward(va, m, s, g):
    with torch.no_grad():
        out = va(m, s, g)
    a = va.astar
    res = (out.histories, out.paths, a.last_iters, a.last_status, a.last_verdict_source)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("B,W", [(1, 32), (3, 32), (64, 32), (130, 32), (5, 64)])
@pytest.mark.parametrize("levels", [False, True], ids=["plain", "attach_levels"])
def test_forward_with_the_proof_equals_forward_without(B, W, levels):
    from neural_astar import ops
    from neural_astar.planner import VanillaAstar
    pr = _mazes(130) if W == 32 else _random_maps(5, 64, 64)
    pr = type(pr)(*(x[:B] for x in pr))
    m, s, g = (_t(x) for x in pr)
    if levels:
        ops.attach_levels(s, _t(_levels(pr)))
    va = VanillaAstar().to(_dev()).eval()
    with early_verdict(False):
        off = _forward(va, m, s, g)
    with early_verdict(True):
        on = _forward(va, m, s, g)
    assert off[4] in ("flag", "sync") and on[4] == "proof"
    for a, b in zip(on[:4], off[:4]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert int(on[3].abs().sum()) == 0


# ---- 3. an unsolvable map raises in the same call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [0, 32, 63])
def test_unsolvable_map_raises_in_the_same_call(where):
    from neural_astar.planner import VanillaAstar
    from neural_astar.planner.differentiable_astar import UnsolvableMapError
    pr = _mazes(130)
    m = pr.map_designs[:64].copy()
    s, g = np.zeros_like(m), np.zeros_like(m)
    s[:], g[:] = pr.start_maps[:64], pr.goal_maps[:64]
    m[where, 0] = 1
    m[where, 0, 16, :] = 0  # a full wall
    s[where], g[where] = 0, 0
    s[where, 0, 0, 0] = 1
    g[where, 0, 31, 31] = 1
    mt, st, gt = _t(m), _t(s), _t(g)
    seen = {}
    for on in (False, True):
        va = VanillaAstar().to(_dev()).eval()
        with early_verdict(on), torch.no_grad(), pytest.raises(UnsolvableMapError) as e:
            va(mt, st, gt)
        torch.cuda.synchronize()
        assert va.astar.last_verdict_source in ("flag", "sync")
        seen[on] = (str(e.value), va.astar.last_status.cpu().numpy())
    assert seen[True][0] == seen[False][0] and f"batch rows [{where}]" in seen[True][0]
    assert np.array_equal(seen[True][1], seen[False][1]) and seen[True][1][where] == 3 and seen[True][1].sum() == 3


# ---- 4. ineligible calls -------------------------------------------------------------------------------------------------------------------
def _ineligible(name):
    """(module, args, kwargs) of a call whose verdict is not a property of the inputs alone, or that has no proof kernel"""
    from neural_astar import ops
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    dev = _dev()
    H, W = {"size_16x16": (16, 16), "size_20x45": (20, 45)}.get(name, (32, 32))
    pr = _random_maps(8, H, W)
    m, s, g = (_t(x) for x in pr)
    da = DifferentiableAstar(0.5, 1.0).to(dev).eval()
    kw = {}
    if name == "training_Tmax":
        da = DifferentiableAstar(0.5, 0.25).to(dev).train()
    elif name == "g_ratio":
        da = DifferentiableAstar(0.2, 1.0).to(dev).eval()
        m, s, g = m[:1], s[:1], g[:1]  # (one map: the call still takes the native host lane)
    elif name == "g_ratio_above_the_bound":
        da = DifferentiableAstar(0.9, 1.0).to(dev).eval()  # (no coupling in exact arithmetic: the native host lane, but not the proof)
    elif name == "heuristic_maps":
        kw["heuristic_maps"] = torch.zeros_like(m)
    elif name == "neighbor_filter":
        with torch.no_grad():
            da.neighbor_filter.copy_(torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0], dtype=torch.float32, device=dev).reshape(1, 1, 3, 3))
        m = torch.ones_like(m)  # (4-connected: keep every map solvable)
    elif name == "unit_cost":
        da.unit_cost = True
    elif name == "untrusted_order":
        s.placement_order = ops.OrderHint(torch.arange(7, -1, -1, dtype=torch.int32, device=dev), trusted=False)
    return da, (m, s, g), kw, name == "unit_cost"


@pytest.mark.parametrize("name", ["training_Tmax", "g_ratio", "g_ratio_above_the_bound", "heuristic_maps", "neighbor_filter", "unit_cost", "size_16x16", "size_20x45",
                                  "untrusted_order"])
def test_ineligible_calls_never_take_the_proof(name):
    res = {}
    for on in (False, True):
        da, (m, s, g), kw, one_tensor = _ineligible(name)
        with early_verdict(on), torch.no_grad():
            out = da(m, s, g, m if one_tensor else m.clone(), **kw)
        res[on] = (out.histories, out.paths, da.last_iters, da.last_status)
        torch.cuda.synchronize()
        assert da.last_verdict_source in ("flag", "sync"), da.last_verdict_source
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    assert int(res[True][3].abs().sum()) == 0 and int(res[True][0].sum()) > 0


# ---- 5. row hygiene --------------------------------------------------------------------------------------------------------------------------
def test_status_rows_over_sixty_calls():
    from neural_astar import ops
    from neural_astar.planner import VanillaAstar
    from neural_astar.planner.differentiable_astar import UnsolvableMapError
    dev = _dev()
    pr = _mazes(130)
    good = tuple(_t(x[:64]) for x in pr)  # mazes with long routes: the searches outlast the return
    m = pr.map_designs[64:128].copy()
    m[17, 0] = 1
    m[17, 0, :, 16] = 0
    s, g = pr.start_maps[64:128].copy(), pr.goal_maps[64:128].copy()
    s[17], g[17] = 0, 0
    s[17, 0, 0, 0] = 1
    g[17, 0, 31, 31] = 1
    bad = (_t(m), _t(s), _t(g))
    board = ops.StatusBoard.of(dev)
    torch.cuda.synchronize()
    board._reap(False)
    free0 = len(board.free) + len(board.zombies)
    va = VanillaAstar().to(dev).eval()
    ref = _forward(va, *good)
    sources = []
    with early_verdict(True), torch.no_grad():
        for i in range(60):
            if i % 3 == 2:
                with pytest.raises(UnsolvableMapError):
                    va(*bad)
                assert va.astar.last_verdict_source in ("flag", "sync")
                assert va.astar.last_status.cpu().numpy().nonzero()[0].tolist() == [17]
            else:
                out = va(*good)
                sources.append(va.astar.last_verdict_source)
                if i % 10 == 0:  # (reading the outputs waits for the searches: most calls do not)
                    assert torch.equal(out.histories, ref[0]) and torch.equal(out.paths, ref[1])
    assert sources == ["proof"] * 40
    assert len(board.zombies) <= 40
    torch.cuda.synchronize()
    board._reap(False)  # raises if a proved launch reported a status
    assert not board.zombies and not board.proved and len(board.free) == free0
    assert not board.np.any()


# ---- 6. stream order -------------------------------------------------------------------------------------------------------------------------
def test_inputs_produced_on_the_current_stream_right_before_the_call():
    from neural_astar.planner import VanillaAstar
    dev = _dev()
    pr = _mazes(130)
    m, s, g = (_t(x[:64]) for x in pr)
    va = VanillaAstar().to(dev).eval()
    with early_verdict(True):
        ref = _forward(va, m, s, g)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            # the inputs come into being on THIS stream immediately before the call: the proof, on its own stream, must wait for them
            filler = torch.zeros(64 << 20, device=dev).add_(1.0)  # (work in front of the clones, so that they are late)
            m2, s2, g2 = m.clone(), s.clone(), g.clone()
            out = va(m2, s2, g2)
            src = va.astar.last_verdict_source
            status = va.astar.last_status
        side.synchronize()
    assert src == "proof" and float(filler[0]) == 1.0
    assert torch.equal(out.histories, ref[0]) and torch.equal(out.paths, ref[1]) and torch.equal(status, ref[3])
