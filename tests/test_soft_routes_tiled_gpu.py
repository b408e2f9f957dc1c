"""GPU: sampled routes from the tiled soft field's checkpointed tape (include/nastar_soft_routes_tiled.h, ``ops.soft_routes_tiled``).

1. the same BITS as the one-workgroup call in every output, on every case of tests/soft_routes_oracle.py, for every spacing of the
   checkpoints, from Philox and from the walkers' own uniforms, with full and with short rows;
2. above the one-workgroup limit: valid by construction, and against the float64 walker on the DEVICE'S OWN planes (the tiled forward at
   horizons 1 .. K-1); ``log_probs`` against ``(dists[start] - route_costs) / tau``;
3. ``visits / N`` against the tiled backward of a one-hot seed;
4. the far corner of the largest map (64-bit indices);
5. seeds, prefixes and the rest of the batch;  6. cold samples;  7. a BAD_COST map beside a good one;  8. the planners.
The call only enqueues, as the tiled forward does; no stream capture is tested.  The figures are printed before they are asserted.
"""
import functools

import numpy as np
import pytest
import torch

import heuristic_oracle as HO
import soft_fields_oracle as SO
import soft_fields_tiled_cases as TC
import soft_routes_oracle as RO
import soft_routes_tiled_cases as RC

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MOORE8 = SO.MOORE8
ALL_SHAPES = RO.SHAPE_CASES + (RO.BIG_CASE,)
FIELDS = ("routes", "route_lengths", "route_costs", "log_probs", "visits", "dists", "status", "map_status")


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(_dev())


def _np(out):
    return [None if x is None else x.cpu().numpy() for x in out]


def _same(got, ref, what):
    for name, x, y in zip(FIELDS, got, ref):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, name)


# ---- 1: the bits of the one-workgroup call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,seed", ALL_SHAPES, ids=lambda v: str(v))
def test_same_bits_as_the_one_workgroup_call(H, W, B, seed):
    from neural_astar import ops
    cost, passable, goal = RO.case_maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    for K, tau, mask, (S, N), sample_seed in RO.cases(H, W, B, seed):
        st = _t(RO.case_starts(sample_seed, S, passable, goal), np.int32)
        uni = _t(RO.crafted_uniforms(sample_seed, B, S, N, K))
        # (Philox with the counts; the walkers' own uniforms; rows shorter than a route: the replay)
        variants = [dict(visits=True), dict(uniforms=uni, visits=True), dict(max_route_len=1, visits=True), dict(max_route_len=5)]
        refs = [ops.soft_routes(c, g, p, st, tau, K, N, sample_seed, neighbor_mask=mask, **kw) for kw in variants]
        # one plane per slot; the default; a spacing that does not divide K; one segment with plane K as the last checkpoint; no checkpoint
        for every in (1, None, 7, K, K + 5):
            for kw, ref in zip(variants, refs):
                got = ops.soft_routes_tiled(c, g, p, st, tau, K, N, sample_seed, neighbor_mask=mask, checkpoint_every=every, **kw)
                _same(got, ref, f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x} S={S} N={N} c={every} {sorted(kw)}")


# ---- 2: above the limit --------------------------------------------------------------------------------------------------------------------------------
def _expected_status(dists, goal, passable, cost, starts):
    B, H, W = goal.shape
    st = np.zeros(starts.shape, np.int32)
    for b in range(B):
        bad = ((passable[b] != 0) & ~(cost[b] >= 0)).any()
        for s, n0 in enumerate(starts[b]):
            if not 0 <= n0 < H * W:
                st[b, s] = 1
            elif bad:
                st[b, s] = 9
            elif goal[b].reshape(-1)[n0] == 0 and not np.isfinite(dists[b].reshape(-1)[n0]):
                st[b, s] = 3
    return st


def _check_valid(out, cost, goal, passable, starts, K, mask, what):
    """the rules of tests/test_soft_routes_gpu.py's ``_check_valid`` on rows of K + 1 cells: the statuses; a failed query's outputs; the
    start, the moves, the passable cells, the FIRST goal last, -1 behind; the cost in fp64 rounded once; the counts"""
    routes, lengths, costs, logp, visits, dists, status, _ = out
    B, S, N, cap = routes.shape
    H, W = goal.shape[1:]
    assert cap == K + 1
    moves = set(HO.offsets(mask))
    assert np.array_equal(status, _expected_status(dists[:, 0], goal, passable, cost, starts)), what
    hist = np.zeros((B, S, H * W), np.int64)
    for b in range(B):
        g, ok, c64 = goal[b].reshape(-1) != 0, passable[b].reshape(-1) != 0, cost[b].reshape(-1).astype(f64)
        for s in range(S):
            for i in range(N):
                L, row = int(lengths[b, s, i]), routes[b, s, i]
                if status[b, s] != 0:
                    assert L == 0 and (row == -1).all() and np.isposinf(costs[b, s, i]) and np.isneginf(logp[b, s, i]), (what, b, s, i)
                    continue
                assert 1 <= L <= K + 1, (what, b, s, i, L)
                cells = row[:L].astype(np.int64)
                assert (row[L:] == -1).all() and cells[0] == starts[b, s] and ((0 <= cells) & (cells < H * W)).all(), (what, b, s, i)
                r, c = cells // W, cells % W
                assert all((dy, dx) in moves for dy, dx in zip(np.diff(r), np.diff(c))), (what, b, s, i)
                assert ok[cells[1:]].all() and g[cells[-1]] and not g[cells[:-1]].any(), (what, b, s, i)
                total = 0.0
                for n in cells[:-1]:
                    total += c64[n]
                assert costs[b, s, i] == f32(total), (what, b, s, i)
                assert np.isfinite(logp[b, s, i]) and logp[b, s, i] <= 0, (what, b, s, i)
                np.add.at(hist[b, s], cells[:-1], 1)
    if visits is not None:
        assert np.array_equal(visits.reshape(B, S, H * W), hist), what


@functools.lru_cache(maxsize=None)
def _device_fields(H, W, B, seed, K, tau, mask):
    """the tiled kernel's fields of horizons 1 .. K-1 -> [K-1][B,H,W] float32: V_k is a pure function of the inputs, so these are the
    planes of every tape up to the store's rounding"""
    from neural_astar import ops
    cost, passable, goal = TC.maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    fields = [ops.soft_fields_tiled_forward(c, g, p, tau, k, neighbor_mask=mask)[0].dists[:, 0] for k in range(1, K)]
    return torch.stack(fields).cpu().numpy()


@pytest.mark.parametrize("H,W,B,seed,K,tau,mask", list(RC.above_cases()), ids=lambda v: str(v))
def test_routes_above_the_limit_are_the_oracles(H, W, B, seed, K, tau, mask):
    from neural_astar import ops
    what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
    cost, passable, goal = TC.maps(H, W, B, seed)
    starts = RC.above_starts(H, W, B, seed, K, mask)
    S, N = RC.ABOVE_S, RC.ABOVE_N
    out = _np(ops.soft_routes_tiled(_t(cost), _t(goal), _t(passable), _t(starts, np.int32), tau, K, N, RC.SAMPLE_SEED, neighbor_mask=mask,
                                    visits=True))
    _check_valid(out, cost, goal, passable, starts, K, mask, what)
    routes, lengths, costs, logp, _, dists, status, _ = out
    fields = _device_fields(H, W, B, seed, K, tau, mask)
    total = flagged = 0
    gap = 0.0
    for b in range(B):
        planes = RO.recursion_planes(list(fields[:, b]) + [dists[b, 0]], goal[b], passable[b])
        groups = RC.above_groups(b, starts, B)
        ref = RO.walk_many(planes, cost[b], goal[b], passable[b], groups, tau, mask)[0]
        assert np.array_equal(ref.status.reshape(S, N), np.repeat(status[b][:, None], N, 1)), what
        live = ref.status == 0
        total += int(live.sum())
        flagged += int(ref.fragile[live].sum())
        for k in np.flatnonzero(live & ~ref.fragile):
            s, i = divmod(int(k), N)
            assert routes[b, s, i, :int(lengths[b, s, i])].tolist() == ref.cells[k], (what, b, s, i)      # cell for cell
        if live.any():
            n0 = groups[0][0]
            lp, rc = logp[b].reshape(-1)[live].astype(f64), costs[b].reshape(-1)[live].astype(f64)
            d0 = np.where(goal[b].reshape(-1)[n0[live]] != 0, 0.0, dists[b, 0].reshape(-1)[n0[live]].astype(f64))
            gap = max(gap, float(np.abs(lp - (d0 - rc) / tau).max() / RO.logp_scale(planes, tau)))
    share = flagged / total if total else 0.0
    print(f"{what}: {total} routes, {flagged} fragile ({share:.4f}), log-prob gap {gap:.3e} (bound {RC.LOGP_RTOL})")
    assert total >= 2 * N * B and share <= RO.FRAGILE_MAX_SHARE, what
    if (H, W) == TC.ABOVE[1][:2]:
        assert gap <= RC.LOGP_RTOL, what


# ---- 3: the sampler against the tiled backward ------------------------------------------------------------------------------------------------------
def test_visits_are_the_tiled_gradient_of_the_field_at_the_start():
    """4096 routes at tau 0.5 from the start 40 hops from the goal of a 130x140 map (tests/soft_routes_tiled_cases.py: the seed was checked
    on the float64 oracle's visits first)"""
    from neural_astar import ops
    cost, passable, goal, start = (a[:1] for a in TC.maxent_maps())
    H, W, K = cost.shape[1], cost.shape[2], TC.ABOVE[1][4]
    tau, N = RC.VISITS_TAU, RC.VISITS_N
    n0 = int(np.flatnonzero(start[0].reshape(-1))[0])
    c, g, p = _t(cost), _t(goal), _t(passable)
    out = ops.soft_routes_tiled(c, g, p, _t([[n0]], np.int32), tau, K, N, RC.VISITS_SEED, visits=True)
    assert out.status.tolist() == [[0]]
    routes, lengths = out.routes.cpu().numpy()[0, 0], out.route_lengths.cpu().numpy()[0, 0]
    per = np.zeros((N, H * W), f32)
    for i in range(N):
        np.add.at(per[i], routes[i, :lengths[i] - 1], 1)
    mean = out.visits.cpu().numpy().reshape(-1) / N
    assert np.array_equal(mean, per.astype(f64).mean(0))
    _, tape = ops.soft_fields_tiled_forward(c, g, p, tau, K, tape=True)
    grad, st = ops.soft_fields_tiled_backward(c, g, p, tape, _t(start), tau, K)
    grad = grad.cpu().numpy().reshape(-1).astype(f64)
    bound = RC.visits_bound(per, grad, N, SO.BWD_RTOL * np.abs(grad).max())
    ratio = np.abs(mean - grad) / bound
    print(f"visits / N against the tiled backward: worst cell at {ratio.max():.3f} of its bound, expected visits up to {grad.max():.3f}")
    assert st.tolist() == [0] and (ratio <= 1).all()


# ---- 4: the far corner ----------------------------------------------------------------------------------------------------------------------------------
def test_far_corner_of_the_largest_map():
    from neural_astar import ops
    H, W, K, tau, N = TC.CORNER_H, TC.CORNER_W, TC.CORNER_K, TC.CORNER_TAU, RC.CORNER_N
    cost, passable, goal = RC.corner_maps()
    c, g, p = _t(cost), _t(goal), _t(passable)
    starts = np.array([RC.CORNER_STARTS], np.int32)
    out = ops.soft_routes_tiled(c, g, p, _t(starts, np.int32), tau, K, N, RC.CORNER_SEED, visits=True, checkpoint_every=TC.CORNER_C)
    assert out.status.tolist() == [[0, 0]] and out.map_status.tolist() == [0]
    routes, lengths, costs, logp, visits, dists, _, _ = _np(out)
    goal_cell = TC.CORNER_GOAL[0] * W + TC.CORNER_GOAL[1]
    r0, c0 = TC.CORNER_WINDOW[0].start, TC.CORNER_WINDOW[1].start
    wh, ww = H - r0, W - c0
    inside = np.zeros((H, W), bool)
    inside[TC.CORNER_WINDOW] = True
    assert visits.any() and not visits[0][:, ~inside].any()
    # the oracle on the device planes cut to the window: the window's own cell numbers
    wc, wp, wg = (TC.corner_window(a)[0] for a in (cost, passable, goal))
    fields = [ops.soft_fields_tiled_forward(c, g, p, tau, k)[0].dists[0, 0][TC.CORNER_WINDOW].cpu().numpy() for k in range(1, K)]
    planes = RO.recursion_planes(fields + [dists[0, 0][TC.CORNER_WINDOW]], wg, wp)
    to_window = lambda n: (n // W - r0) * ww + (n % W - c0)
    u = RO.case_uniforms(RC.CORNER_SEED, 1, 2, N)
    ref = RO.walk(planes, wc, wg, wp, np.repeat([to_window(int(n)) for n in starts[0]], N), tau, MOORE8, u)
    assert (ref.status == 0).all() and ref.fragile.mean() <= RO.FRAGILE_MAX_SHARE
    for k in range(2 * N):
        s, i = divmod(k, N)
        L = int(lengths[0, s, i])
        cells = routes[0, s, i, :L].astype(np.int64)
        assert 2 <= L <= K + 1 and cells[0] == starts[0, s] and cells[-1] == goal_cell and (routes[0, s, i, L:] == -1).all(), (s, i)
        assert inside.reshape(-1)[cells].all() and passable[0].reshape(-1)[cells[1:]].all(), (s, i)
        assert max(np.abs(np.diff(cells // W)).max(), np.abs(np.diff(cells % W)).max()) == 1, (s, i)
        assert costs[0, s, i] == f32(cost[0].reshape(-1)[cells[:-1]].astype(f64).cumsum()[-1]) and logp[0, s, i] <= 0, (s, i)
        if not ref.fragile[k]:
            assert to_window(cells).tolist() == ref.cells[k], (s, i)
    hist = np.zeros(H * W, np.int64)
    for s in range(2):
        one = np.zeros(H * W, np.int64)
        for i in range(N):
            np.add.at(one, routes[0, s, i, :lengths[0, s, i] - 1], 1)
        assert np.array_equal(visits[0, s].reshape(-1), one)
    # one column more is refused
    wide = torch.ones(1, 1, H, W + 1, device=_dev())
    with pytest.raises(NotImplementedError, match="1179648"):
        ops.soft_routes_tiled(wide, wide, wide, torch.zeros(1, 1, dtype=torch.int32, device=_dev()), tau, K, seed=1)


# ---- 5: determinism ---------------------------------------------------------------------------------------------------------------------------------------
def test_seeds_prefixes_and_the_rest_of_the_batch():
    from neural_astar import ops
    H, W, B, seed, K = TC.ABOVE[0]
    S, N, tau = 3, 40, 0.5
    cost, passable, goal = TC.maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    starts = RC.above_starts(H, W, B, seed, K)[:, :S].copy()
    starts[:, 2] = starts[:, 0]                                          # two queries from one cell: other routes (q differs)
    st = _t(starts, np.int32)
    a, b = _np(ops.soft_routes_tiled(c, g, p, st, tau, K, N, 77, visits=True)), _np(ops.soft_routes_tiled(c, g, p, st, tau, K, N, 77, visits=True))
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)                      # same seed: same bits
    other = _np(ops.soft_routes_tiled(c, g, p, st, tau, K, N, 78))
    assert not np.array_equal(a[0], other[0]) and np.array_equal(a[6], other[6]) and not a[6].any()
    assert not np.array_equal(a[0][:, 0], a[0][:, 2])
    more = _np(ops.soft_routes_tiled(c, g, p, st, tau, K, 3 * N + 1, 77))    # the first N samples are a prefix
    for k in (0, 1, 2, 3):
        assert np.array_equal(more[k][:, :, :N], a[k], equal_nan=True), k
    part = _np(ops.soft_routes_tiled(c[:1], g[:1], p[:1], st[:1], tau, K, N, 77))   # q = b * S + s: map 0 alone
    for k in (0, 1, 2, 3, 6):
        assert np.array_equal(part[k], a[k][:1], equal_nan=True), k
    torch.manual_seed(3)
    r1 = ops.soft_routes_tiled(c, g, p, st, tau, K, N)
    torch.manual_seed(3)
    r2 = ops.soft_routes_tiled(c, g, p, st, tau, K, N)
    r3 = ops.soft_routes_tiled(c, g, p, st, tau, K, N)
    assert torch.equal(r1.routes, r2.routes) and not torch.equal(r1.routes, r3.routes)


# ---- 6: the hard limit ------------------------------------------------------------------------------------------------------------------------------------
def test_cold_samples_are_the_optimal_route():
    """tau = 1e-3 on the 130x140 map, from the starts whose optimal route is unique by a margin: at each of its cells the best neighbour
    beats the second best by 0.03 = 30 tau, so another move has probability below 7 exp(-30)"""
    from neural_astar import ops
    H, W, _, seed, _ = TC.ABOVE[1]
    tau, N, K = 1e-3, 3, SO.default_horizon(H, W)
    cost, passable, goal = TC.maps(H, W, 1, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    field = ops.cost_to_go_tiled(c, g, p, policies=False)[0].dists
    D = field[0, 0].cpu().numpy().astype(f64)
    hops = SO.hops(goal[0], passable[0]).reshape(-1)
    cand = np.flatnonzero((hops > 0) & (hops <= 30)).astype(np.int32)      # 1465 cells; on the float64 field 396 of them are kept
    fr = ops.field_routes(field, g, p, _t(cand[None], np.int32), max_route_len=K + 1)
    assert not fr.status.any()
    rows, lens = fr.routes[0].cpu().numpy(), fr.route_lengths[0].cpu().numpy()
    Dp = np.pad(np.where(passable[0] != 0, D, np.inf), 1, constant_values=np.inf)
    keep = []
    for s in range(cand.size):
        best = [sorted(Dp[n // W + 1 + dy, n % W + 1 + dx] for dy, dx in HO.offsets(MOORE8))[:2] for n in rows[s, :lens[s] - 1]]
        if all(np.isinf(b_) or b_ - a_ >= 0.03 for a_, b_ in best):
            keep.append(s)
    assert len(keep) > 300
    st = _t(cand[keep][None], np.int32)
    out = ops.soft_routes_tiled(c, g, p, st, tau, K, N, 17)
    assert not out.status.any()
    want = fr.routes[:, keep]
    assert torch.equal(out.routes, want[:, :, None].expand(-1, -1, N, -1)) and torch.equal(out.route_lengths, fr.route_lengths[:, keep, None].expand(-1, -1, N))
    assert out.log_probs.min().item() > -1e-6


# ---- 7: a BAD_COST map beside a good one ------------------------------------------------------------------------------------------------------------------
def test_a_bad_cost_map_fails_alone():
    from neural_astar import ops
    H, W, B, seed, K = TC.ABOVE[0]
    cost, passable, goal = (a.copy() for a in TC.maps(H, W, B, seed))
    starts = RC.above_starts(H, W, B, seed, K)
    y, x = np.argwhere(passable[1] != 0)[-1]
    cost[1, y, x] = np.nan
    N, tau = 20, 0.5
    out = ops.soft_routes_tiled(_t(cost), _t(goal), _t(passable), _t(starts, np.int32), tau, K, N, 9, visits=True)
    alone = ops.soft_routes_tiled(_t(cost[:1]), _t(goal[:1]), _t(passable[:1]), _t(starts[:1], np.int32), tau, K, N, 9, visits=True)
    assert out.map_status.tolist() == [0, 9] and (out.status[1] == 9).all() and out.status[0].tolist() == alone.status[0].tolist()
    assert not out.route_lengths[1].any() and (out.routes[1] == -1).all() and not out.visits[1].any()
    assert torch.isposinf(out.route_costs[1]).all() and torch.isneginf(out.log_probs[1]).all()
    for x_, y_ in zip(out[:5], alone[:5]):
        assert torch.equal(x_[:1], y_)
    assert (out.route_lengths[0, :3] > 0).all()


# ---- 8: the planners ---------------------------------------------------------------------------------------------------------------------------------------
def test_planners_sample_from_the_tiled_field():
    from neural_astar import ops, planner
    from neural_astar.planner.differentiable_astar import DifferentiableAstar
    H, W, _, seed, K = TC.ABOVE[1]
    cost, passable, goal = TC.maps(H, W, 1, seed)
    starts = RC.above_starts(H, W, 1, seed, K)
    c, g, p, st = _t(cost)[:, None], _t(goal)[:, None], _t(passable)[:, None], _t(starts, np.int32)
    da = DifferentiableAstar(0.5, 1.0).to(_dev())
    r = da.sample_routes_tiled(c, st, g, p, 0.5, num_samples=6, seed=9, horizon=K, visits=True, checkpoint_every=5)
    ref = ops.soft_routes_tiled(c, g, p, st, 0.5, K, 6, 9, visits=True)
    _same(r, ref, "DifferentiableAstar")
    with pytest.raises(NotImplementedError, match="soft_routes_tiled"):
        da.sample_routes(c, st, g, p, 0.5)
    va = planner.VanillaAstar().to(_dev())
    rv = va.sample_routes_tiled(p, st, g, 0.5, num_samples=6, seed=9, horizon=K)
    _same(rv, ops.soft_routes_tiled(p, g, p, st, 0.5, K, 6, 9), "VanillaAstar")
    ok = rv.status == 0
    assert ok[0, :3].all() and (rv.route_costs[ok] == (rv.route_lengths[ok] - 1)).all()       # unit costs: a route of L moves costs L
    torch.manual_seed(0)
    na = planner.NeuralAstar(encoder_input="m", encoder_arch="CNN", encoder_depth=4).to(_dev()).eval()
    rn = na.sample_routes_tiled(p, st, g, 0.1, num_samples=6, seed=9, max_route_len=12, visits=True)
    pred = na.encode(p, torch.zeros_like(g), g).detach()
    _same(rn, ops.soft_routes_tiled(pred, g, p, st, 0.1, None, 6, 9, max_route_len=12, visits=True), "NeuralAstar")
    assert tuple(rn.routes.shape) == (1, 4, 6, 12) and not rn.routes.requires_grad
    with pytest.raises(NotImplementedError, match="encoder_input"):
        planner.NeuralAstar(encoder_input="m+").to(_dev()).sample_routes_tiled(p, st, g, 0.1)
