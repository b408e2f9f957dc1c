"""GPU: sampled routes from the maximum-entropy route distribution (include/nastar_soft_routes.h, ``ops.soft_routes``).

1. valid by construction, exactly, with no oracle: starts, moves, goals, lengths, padding, costs, visits, short rows, statuses;
2. against the float64 walker of tests/soft_routes_oracle.py on the DEVICE'S OWN planes (the forward at horizons 1 .. K-1): every route the
   oracle does not flag fragile is identical, at most ``RO.FRAGILE_MAX_SHARE`` are flagged; Philox and the ``uniforms=`` path;
3. ``log_probs`` against ``(dists[start] - route_costs) / tau`` within ``RO.LOGP_RTOL``;
4. the sampler against the gradient kernel: ``visits / N`` is the backward of a one-hot ``grad_dists``;
5. determinism: seeds, prefixes, the rest of the batch;  6. the hard limit;  7. the planners and a captured graph.
Every map has 25 % obstacles and costs U(0.1, 1) unless a case says otherwise; the figures are printed before they are asserted.
"""
import functools

import numpy as np
import pytest
import torch

import field_routes_oracle as FR
import fields_oracle as FO
import heuristic_oracle as HO
import soft_fields_oracle as SO
import soft_routes_oracle as RO

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MOORE8 = SO.MOORE8
ALL_SHAPES = RO.SHAPE_CASES + (RO.BIG_CASE,)


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _t(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(_dev())


@functools.lru_cache(maxsize=None)
def _maps(H, W, B, seed):
    return RO.case_maps(H, W, B, seed)


def _np(out):
    """SoftRoutes (or the tuple of soft_routes_from_tape) -> numpy arrays, None kept"""
    return [None if x is None else x.cpu().numpy() for x in out]


# ---- 1: valid by construction ------------------------------------------------------------------------------------------------------------------
def _expected_status(dists, goal, passable, cost, starts):
    """[B,S] from the inputs and the device's own field: 1 outside the map, 9 on a BAD_COST map, 3 where the field is not finite (and the
    start is no goal)"""
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


def _check_valid(out, cost, goal, passable, starts, K, mask, what, full=None):
    """``out``: numpy (routes, lengths, costs, log_probs, visits, dists, status, map_status).  ``full``: the rows of the same call with
    rows of K + 1 cells, when ``out`` has shorter ones."""
    routes, lengths, costs, logp, visits, dists, status, _ = out
    B, S, N, cap = routes.shape
    H, W = goal.shape[1:]
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
                if full is not None:   # a short row keeps the LAST cells and reports the true length
                    whole = full[0][b, s, i][:L]
                    keep = whole[max(0, L - cap):]
                    assert np.array_equal(row[:len(keep)], keep) and (row[len(keep):] == -1).all() and L == full[1][b, s, i], (what, b, s, i)
                    continue
                cells = row[:L].astype(np.int64)
                assert (row[L:] == -1).all() and cells[0] == starts[b, s] and ((0 <= cells) & (cells < H * W)).all(), (what, b, s, i)
                r, c = cells // W, cells % W
                assert all((dy, dx) in moves for dy, dx in zip(np.diff(r), np.diff(c))), (what, b, s, i)      # every move is allowed
                assert ok[cells[1:]].all() and g[cells[-1]] and not g[cells[:-1]].any(), (what, b, s, i)    # onto passable cells; ends at its FIRST goal
                total = 0.0
                for n in cells[:-1]:
                    total += c64[n]                                                                       # fp64, travel order
                assert costs[b, s, i] == f32(total), (what, b, s, i)                                        # rounded once
                assert np.isfinite(logp[b, s, i]) and logp[b, s, i] <= 0, (what, b, s, i)
                np.add.at(hist[b, s], cells[:-1], 1)
    if visits is not None and full is None:
        assert np.array_equal(visits.reshape(B, S, H * W), hist), what


@pytest.mark.parametrize("H,W,B,seed", ALL_SHAPES, ids=lambda v: str(v))
def test_routes_are_valid_by_construction(H, W, B, seed):
    from neural_astar import ops
    cost, passable, goal = _maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    for K, tau, mask, (S, N), sample_seed in RO.cases(H, W, B, seed):
        what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x} S={S} N={N}"
        starts = RO.case_starts(sample_seed, S, passable, goal)
        out = ops.soft_routes(c, g, p, _t(starts, np.int32), tau, K, N, sample_seed, neighbor_mask=mask, visits=True)
        assert tuple(out.routes.shape) == (B, S, N, K + 1) and tuple(out.visits.shape) == (B, S, H, W) and out.routes.dtype == torch.int32
        assert not any(x.requires_grad for x in out)
        ref = _np(out)
        _check_valid(ref, cost, goal, passable, starts, K, mask, what)
        # the two kernel shapes, whichever the call above ran: the same bits
        # (the forward as ``soft_routes`` calls it: a tape at every size the forward takes)
        tape = ops._soft_forward(False, False, c, g, p, tau, K, mask, False, True, tape_limit=ops.SOFT_ROUTES_MAX_CELLS)[4]
        for shape in ("lds", "gather"):
            got = _np(ops.soft_routes_from_tape(c, g, p, tape, _t(starts, np.int32), tau, K, N, sample_seed, mask, visits=True, shape=shape))
            for a, b_ in zip(got, ref[:5] + ref[6:7]):
                assert np.array_equal(a, b_, equal_nan=True), (what, shape)
        # rows shorter than a route keep its last cells
        cap = max(1, min(3, K))
        short = _np(ops.soft_routes(c, g, p, _t(starts, np.int32), tau, K, N, sample_seed, neighbor_mask=mask, max_route_len=cap))
        assert short[0].shape[-1] == cap and short[4] is None
        _check_valid(short, cost, goal, passable, starts, K, mask, what + " short rows", full=ref)
        for k in (1, 2, 3, 6):
            assert np.array_equal(short[k], ref[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("value", [float("nan"), -0.25])
def test_statuses_failed_queries_and_goals_of_every_kind(value):
    from neural_astar import ops
    H, W, K, tau, N = 7, 9, 32, 0.5, 5
    cost, passable, goal = SO.random_maps(31, 3, H, W)
    cost[1, 2, 3], passable[1, 2, 3] = value, 1                       # a BAD_COST map between two good ones
    cost[2, 0, 0], passable[2, 0, 0] = value, 0                       # ... and a bad cost on an OBSTACLE, which is not looked at
    passable[0, 3, 4], goal[0, 3, 4] = 0, 1                            # a goal on an obstacle
    goal[0, 6, 8] = goal[0, 0, 8] = 1                                  # several goals
    passable[0, 6, 8] = passable[0, 0, 8] = 1
    wall = np.flatnonzero(passable[2].reshape(-1) == 0)
    starts = np.array([[3 * W + 4, 6 * W + 8, 5, -1, H * W, 20],       # on the obstacle goal; on a passable goal; ...; outside twice
                       [0, 2 * W + 3, int(np.flatnonzero(goal[1].reshape(-1))[0]), -7, 11, 12],
                       [int(wall[0]), 1, 2, 3, 2 ** 31 - 1, 30]], np.int32)
    out = ops.soft_routes(_t(cost), _t(goal), _t(passable), _t(starts, np.int32), tau, K, N, 5, visits=True)
    ref = _np(out)
    _check_valid(ref, cost, goal, passable, starts, K, MOORE8, f"bad cost {value}")
    routes, lengths, costs, logp, visits, dists, status, map_status = ref
    assert map_status.tolist() == [0, 9, 0] and (status[1] == np.where((starts[1] < 0) | (starts[1] >= H * W), 1, 9)).all()
    assert status[0, :2].tolist() == [0, 0] and status[0, 3:5].tolist() == [1, 1] and status[2, 0] == 3 and status[2, 4] == 1
    for s in (0, 1):                                                   # a start on a goal: [n_0], passable or not
        assert (lengths[0, s] == 1).all() and (routes[0, s, :, 0] == starts[0, s]).all() and (routes[0, s, :, 1:] == -1).all()
        assert not costs[0, s].any() and not logp[0, s].any() and not visits[0, s].any()
    assert not visits[1].any() and visits[0].any() and visits[2].any()
    assert not (routes[0] == 3 * W + 4)[:, :, 1:].any()                # the goal on the obstacle is never entered
    ends = {int(routes[0, s, i, lengths[0, s, i] - 1]) for s in range(6) for i in range(N) if lengths[0, s, i] > 1}
    assert ends <= set(np.flatnonzero(goal[0].reshape(-1)).tolist()) - {3 * W + 4}


# ---- 2, 3: against the oracle on the device's own planes ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_fields(H, W, B, seed, tau, mask):
    """the kernel's fields of horizons 1 .. 2 (H + W) - 1 -> [horizon - 1][B,H,W] float32: the header makes V_k a pure function of the
    inputs, so these are the planes of every tape up to the store's rounding"""
    from neural_astar import ops
    cost, passable, goal = _maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    fields = [ops.soft_fields_forward(c, g, p, tau, k, neighbor_mask=mask)[0].dists[:, 0] for k in range(1, SO.default_horizon(H, W))]
    return torch.stack(fields).cpu().numpy() if fields else np.zeros((0, B, H, W), f32)


def _compare(calls, cost, goal, passable, fields, K, tau, mask, what):
    """the device's routes against the float64 walker on the device's planes.  ``calls``: [(numpy outputs, starts [B,S], N, u_of), ...],
    every call of one (horizon, tau, mask); all of a map's walkers advance in ONE walk -> (routes, fragile routes, the worst log-prob gap)"""
    B = cost.shape[0]
    dists = calls[0][0][5]
    total = flagged = 0
    gap = 0.0
    for b in range(B):
        planes = RO.recursion_planes(list(fields[:K - 1, b]) + [dists[b, 0]], goal[b], passable[b])
        groups = []
        for _, starts, N, u_of in calls:
            sel = slice(b * starts.shape[1] * N, (b + 1) * starts.shape[1] * N)
            groups.append((np.repeat(starts[b], N), lambda j, u_of=u_of, sel=sel: u_of(j)[sel]))
        for (got, starts, N, _), (n0, _), ref in zip(calls, groups, RO.walk_many(planes, cost[b], goal[b], passable[b], groups, tau, mask)):
            routes, lengths, costs, logp, _, _, status, _ = got
            S = starts.shape[1]
            assert np.array_equal(ref.status.reshape(S, N), np.repeat(status[b][:, None], N, 1)), what
            live = ref.status == 0
            total += int(live.sum())
            flagged += int(ref.fragile[live].sum())
            for k in np.flatnonzero(live & ~ref.fragile):
                s, i = divmod(int(k), N)
                L = int(lengths[b, s, i])
                assert routes[b, s, i, :L].tolist() == ref.cells[k], (what, b, s, i)      # cell for cell
            if live.any():
                lp, rc = logp[b].reshape(-1)[live].astype(f64), costs[b].reshape(-1)[live].astype(f64)
                d0 = np.where(goal[b].reshape(-1)[n0[live]] != 0, 0.0, dists[b, 0].reshape(-1)[n0[live]].astype(f64))
                gap = max(gap, float(np.abs(lp - (d0 - rc) / tau).max() / RO.logp_scale(planes, tau)))
    return total, flagged, gap


@pytest.mark.parametrize("H,W,B,seed", ALL_SHAPES, ids=lambda v: str(v))
def test_routes_are_the_oracles(H, W, B, seed):
    from neural_astar import ops
    cost, passable, goal = _maps(H, W, B, seed)
    c, g, p = _t(cost), _t(goal), _t(passable)
    worst_share, worst_gap = 0.0, 0.0
    for K, tau, mask, walkers in RO.oracle_cases(H, W, B, seed):
        what = f"{B}x{H}x{W} K={K} tau={tau} mask={mask:#05x}"
        fields = _device_fields(H, W, B, seed, tau, mask)
        calls = []
        for (S, N), sample_seed in walkers:      # every walker count: from Philox, and from the walkers' own (random and crafted) uniforms
            starts = RO.case_starts(sample_seed, S, passable, goal)
            st = _t(starts, np.int32)
            calls.append((_np(ops.soft_routes(c, g, p, st, tau, K, N, sample_seed, neighbor_mask=mask)), starts, N,
                          RO.case_uniforms(sample_seed, B, S, N)))
            uni = RO.crafted_uniforms(sample_seed, B, S, N, K)
            flat = uni.reshape(-1, K).astype(f64)
            calls.append((_np(ops.soft_routes(c, g, p, st, tau, K, N, sample_seed, neighbor_mask=mask, uniforms=_t(uni))), starts, N,
                          lambda j, flat=flat: flat[:, j]))
        total, flagged, gap = _compare(calls, cost, goal, passable, fields, K, tau, mask, what)
        share = flagged / total if total else 0.0
        worst_share, worst_gap = max(worst_share, share), max(worst_gap, gap)
        print(f"{what}: {total} routes, {flagged} fragile ({share:.4f}), log-prob gap {gap:.3e}")
        assert share <= RO.FRAGILE_MAX_SHARE, what
    print(f"{B}x{H}x{W}: worst fragile share {worst_share:.4f}, worst log-prob gap {worst_gap:.3e} (bound {RO.LOGP_RTOL:.3e})")
    assert worst_gap <= RO.LOGP_RTOL


# ---- 4: the sampler against the gradient kernel ----------------------------------------------------------------------------------------------------
def test_visits_are_the_gradient_of_the_field_at_the_start():
    """4096 routes from the farthest cell of an 8x8 map (seed 4, tau = 1, sample seed 2: on the float64 oracle with these seeds the worst
    cell stands at 0.43 of the bound, and every reachable cell expects more than 3e-3 visits)"""
    from neural_astar import ops
    H = W = 8
    tau, N, K = 1.0, 4096, SO.default_horizon(8, 8)
    cost, passable, goal = SO.random_maps(4, 1, H, W)
    n0 = int(np.argmax(SO.hops(goal[0], passable[0]).reshape(-1)))
    c, g, p = _t(cost), _t(goal), _t(passable)
    out = ops.soft_routes(c, g, p, _t([[n0]], np.int32), tau, K, N, 2, visits=True)
    assert out.status.tolist() == [[0]]
    routes, lengths = out.routes.cpu().numpy()[0, 0], out.route_lengths.cpu().numpy()[0, 0]
    per = np.zeros((N, H * W), f64)
    for i in range(N):
        np.add.at(per[i], routes[i, :lengths[i] - 1], 1)
    mean = out.visits.cpu().numpy().reshape(-1) / N
    assert np.array_equal(mean, per.mean(0))
    onehot = np.zeros((1, H, W), f32)
    onehot.reshape(-1)[n0] = 1
    _, tape = ops.soft_fields_forward(c, g, p, tau, K, tape=True)
    grad, st = ops.soft_fields_backward(c, g, p, tape, _t(onehot), tau, K)
    grad = grad.cpu().numpy().reshape(-1).astype(f64)
    se = per.std(0, ddof=1) / np.sqrt(N)
    bound = 5 * se + SO.BWD_RTOL * np.abs(grad).max()
    ratio = np.abs(mean - grad) / bound
    print(f"visits / N against the backward: worst cell at {ratio.max():.3f} of its bound, expected visits {grad[grad > 0].min():.2e} .. {grad.max():.3f}")
    assert st.tolist() == [0] and (ratio <= 1).all()


# ---- 5: determinism -----------------------------------------------------------------------------------------------------------------------------------
def test_seeds_prefixes_and_the_rest_of_the_batch():
    from neural_astar import ops
    H, W, B, S, N, K, tau = 16, 16, 3, 4, 40, 64, 1.0
    cost, passable, goal = SO.random_maps(12, B, H, W)
    c, g, p = _t(cost), _t(goal), _t(passable)
    starts = RO.case_starts(5, S, passable, goal)
    starts[:, 2] = starts[:, 0]                                          # two queries from one cell: other routes (q differs)
    st = _t(starts, np.int32)
    a, b = _np(ops.soft_routes(c, g, p, st, tau, K, N, 77, visits=True)), _np(ops.soft_routes(c, g, p, st, tau, K, N, 77, visits=True))
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)                      # same seed: same bits
    other = _np(ops.soft_routes(c, g, p, st, tau, K, N, 78))
    assert not np.array_equal(a[0], other[0]) and np.array_equal(a[6], other[6])
    assert not np.array_equal(a[0][:, 0], a[0][:, 2])
    more = _np(ops.soft_routes(c, g, p, st, tau, K, 3 * N + 1, 77))      # the first N samples are a prefix
    for k in (0, 1, 2, 3):
        assert np.array_equal(more[k][:, :, :N], a[k], equal_nan=True), k
    # a sample with a constant q = b * S + s does not change with the rest of the batch: map 0 alone, and maps 0..1
    for nb in (1, 2):
        part = _np(ops.soft_routes(c[:nb], g[:nb], p[:nb], st[:nb], tau, K, N, 77))
        for k in (0, 1, 2, 3, 6):
            assert np.array_equal(part[k], a[k][:nb], equal_nan=True), (nb, k)
    # seed=None draws from torch's default generator
    torch.manual_seed(3)
    r1 = ops.soft_routes(c, g, p, st, tau, K, N)
    torch.manual_seed(3)
    r2 = ops.soft_routes(c, g, p, st, tau, K, N)
    r3 = ops.soft_routes(c, g, p, st, tau, K, N)
    assert torch.equal(r1.routes, r2.routes) and not torch.equal(r1.routes, r3.routes)


# ---- 6: the hard limit ------------------------------------------------------------------------------------------------------------------------------------
def test_cold_samples_are_the_optimal_route():
    """tau = 1e-3 on random costs, from every start whose optimal route is unique by a margin: at each of its cells the best neighbour
    beats the second best by 0.03 = 30 tau, so another move has probability below 7 exp(-30)"""
    from neural_astar import ops
    H = W = 16
    tau, N, K = 1e-3, 4, SO.default_horizon(16, 16)
    cost, passable, goal = SO.random_maps(7, 1, H, W)
    D, _, _ = FO.field(cost[0], goal[0], passable[0], MOORE8)
    every = np.flatnonzero(np.isfinite(D.reshape(-1)))
    hard = FR.routes(D, goal[0], passable[0], every, MOORE8)
    Dp = np.pad(np.where(passable[0] != 0, D, np.inf), 1, constant_values=np.inf)
    keep = []
    for s in range(every.size):
        best = [sorted(Dp[n // W + 1 + dy, n % W + 1 + dx] for dy, dx in HO.offsets(MOORE8))[:2] for n in hard.cells[s][:-1]]
        gaps = [np.inf if np.isinf(b) else b - a for a, b in best]
        if all(x >= 0.03 for x in gaps):
            keep.append(s)
    assert len(keep) > 100
    c, g, p = _t(cost), _t(goal), _t(passable)
    starts = every[keep].astype(np.int32)[None]
    out = ops.soft_routes(c, g, p, _t(starts, np.int32), tau, K, N, 17)
    fr = ops.field_routes(ops.cost_to_go(c, g, p, policies=False).dists, g, p, _t(starts, np.int32), max_route_len=K + 1)
    assert not out.status.any() and not fr.status.any()
    assert torch.equal(out.routes, fr.routes[:, :, None].expand(-1, -1, N, -1)) and torch.equal(out.route_lengths, fr.route_lengths[:, :, None].expand(-1, -1, N))
    for k, s in enumerate(keep):
        assert out.routes[0, k, 0, :hard.lengths[s]].tolist() == hard.cells[s]
    assert out.log_probs.min().item() > -1e-6


# ---- 7: the planners, and a captured graph -----------------------------------------------------------------------------------------------------------------
def test_planners_sample_end_to_end():
    from neural_astar import ops, planner
    from neural_astar.utils import synthetic as syn
    P = syn.random_obstacle_maps(4, 16, 16, 0.25, seed=3)
    maps, goals = _t(P.map_designs), _t(P.goal_maps)
    B, H, W = 4, 16, 16
    idx = RO.case_starts(1, 3, P.map_designs[:, 0], P.goal_maps[:, 0])
    starts = _t(idx, np.int32)
    va = planner.VanillaAstar().to(_dev())
    r = va.sample_routes(maps, starts, goals, 0.5, num_samples=6, seed=9, visits=True)
    ref = ops.soft_routes(maps, goals, maps, starts, 0.5, None, 6, 9, visits=True)
    for x, y in zip(r, ref):
        assert torch.equal(x, y)
    _check_valid(_np(r), P.map_designs[:, 0], P.goal_maps[:, 0], P.map_designs[:, 0], idx, 2 * (H + W), MOORE8, "VanillaAstar")
    assert (r.route_costs[r.status == 0] == (r.route_lengths[r.status == 0] - 1)).all()       # unit costs: a route of L moves costs L
    # the float start maps of the dataset, one channel per start
    smaps = torch.zeros(B, 2, H, W, device=_dev())
    for b in range(B):
        smaps[b, 0].view(-1)[int(idx[b, 0])] = 1
        smaps[b, 1].view(-1)[int(idx[b, 1])] = 1
    r2 = va.sample_routes(maps, smaps, goals, 0.5, num_samples=6, seed=9)
    ref2 = va.sample_routes(maps, starts[:, :2].contiguous(), goals, 0.5, num_samples=6, seed=9)   # (q = b * S + s: S is part of a sample's number)
    assert torch.equal(r2.routes, ref2.routes) and torch.equal(r2.log_probs, ref2.log_probs) and (r2.route_lengths[:, 0] > 0).all()
    # 4-connected moves through the module's own move set
    va4 = planner.VanillaAstar().to(_dev())
    with torch.no_grad():
        va4.astar.neighbor_filter.copy_(torch.tensor([[0., 1, 0], [1, 0, 1], [0, 1, 0]]).view(1, 1, 3, 3))
    r4 = va4.sample_routes(maps, starts, goals, 0.5, num_samples=6, seed=9)
    _check_valid(_np(r4), P.map_designs[:, 0], P.goal_maps[:, 0], P.map_designs[:, 0], idx, 2 * (H + W), HO.VON_NEUMANN, "VanillaAstar 4-connected")
    # NeuralAstar: on the predicted costs, "m" only
    torch.manual_seed(0)
    na = planner.NeuralAstar(encoder_input="m", encoder_arch="CNN", encoder_depth=4).to(_dev()).eval()
    rn = na.sample_routes(maps, starts, goals, 0.1, num_samples=6, seed=9, max_route_len=12, visits=True)
    pred = na.encode(maps, torch.zeros_like(goals), goals).detach()   # (as sample_routes encodes: the route encode() picks depends on grad mode)
    refn = ops.soft_routes(pred, goals, maps, starts, 0.1, None, 6, 9, max_route_len=12, visits=True)
    for x, y in zip(rn, refn):
        assert torch.equal(x, y)
    assert tuple(rn.routes.shape) == (B, 3, 6, 12) and (rn.status[:, 0] == 0).all() and not rn.routes.requires_grad
    full = na.sample_routes(maps, starts, goals, 0.1, num_samples=6, seed=9)
    _check_valid(_np(full), pred[:, 0].cpu().numpy(), P.goal_maps[:, 0], P.map_designs[:, 0], idx, 2 * (H + W), MOORE8, "NeuralAstar")
    with pytest.raises(NotImplementedError, match="encoder_input"):
        planner.NeuralAstar(encoder_input="m+").to(_dev()).sample_routes(maps, starts, goals, 0.1)


def test_a_captured_graph_replays_the_eager_bits():
    from neural_astar import ops
    H, W, B, S, N, K, tau = 16, 16, 2, 3, 70, 64, 0.5
    cost, passable, goal = SO.random_maps(14, B, H, W)
    c, g, p = _t(cost), _t(goal), _t(passable)
    st = _t(RO.case_starts(2, S, passable, goal), np.int32)
    _, tape = ops.soft_fields_forward(c, g, p, tau, K, tape=True)
    eager = ops.soft_routes_from_tape(c, g, p, tape, st, tau, K, N, 123, visits=True, max_route_len=9)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.soft_routes_from_tape(c, g, p, tape, st, tau, K, N, 123, visits=True, max_route_len=9)   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.soft_routes_from_tape(c, g, p, tape, st, tau, K, N, 123, visits=True, max_route_len=9)
    for _ in range(2):                                                   # (the second replay: the clearing of the rows and counts is part of the graph)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(captured, eager):
            assert torch.equal(x, y)
    whole = ops.soft_routes(c, g, p, st, tau, K, N, 123, max_route_len=9, visits=True)
    for x, y in zip((whole.routes, whole.route_lengths, whole.route_costs, whole.log_probs, whole.visits, whole.status), eager):
        assert torch.equal(x, y)
